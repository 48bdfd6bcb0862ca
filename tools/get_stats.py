#!/usr/bin/env python3
"""Writes the statistics files of a dataset (``global_means.npy``, ``global_stds.npy``, ``mins.npy``, ``maxs.npy``,
``time_means.npy``, ``time_diff_means.npy``, ``time_diff_stds.npy``) with ``makani_amd.stats.DatasetStats``: the job of
``data_process/get_stats.py``, with its arguments.

    python3 tools/get_stats.py --input_dir DIR --output_dir DIR [--quadrature_rule naive] [--batch_size 16]
                               [--wind_angle --channel_names '["u10m", "v10m", ...]'] [--carry] [--device cuda:0]
    torchrun --nproc_per_node N tools/get_stats.py ...        # the samples are sharded over the ranks

``--input_dir`` holds ``*.npy`` files of shape ``[T, C, H, W]`` (read through ``np.load(mmap_mode="r")``) or ``*.h5`` files
with a ``fields`` dataset of that shape (read only when ``h5py`` imports; the tool says so and exits when it does not).  The
files, sorted by name, form one sequence of samples.  Under ``torchrun`` rank r takes the r-th chunk of
``ceil(total / ranks)`` consecutive samples and ``DatasetStats.all_reduce`` combines the ranks; there is no MPI.  Batches go
to the device from pinned memory with non-blocking copies, two buffers in turn.  ``--channel_names`` (a JSON list) names the
channels for ``--wind_angle``, which pairs every ``u<level>`` with its ``v<level>``.  ``--carry`` forms the time difference
across batch and file boundaries too (the files are then taken as consecutive in time); without it a difference is formed
within a batch only, as in the reference.  What the files hold, and where they deviate from the reference's, is in the
docstring of ``makani_amd/stats.py``."""
import argparse
import glob
import json
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RULES = {"naive": "naive", "clenshaw-curtiss": "clenshaw-curtiss", "gauss-legendre": "legendre-gauss", "legendre-gauss": "legendre-gauss"}


def open_files(input_dir):
    """[(name, array-like [T, C, H, W])] of the ``*.npy`` and ``*.h5`` files of the directory, sorted by name."""
    names = sorted(glob.glob(os.path.join(input_dir, "*.npy")) + glob.glob(os.path.join(input_dir, "*.h5")))
    if not names:
        raise FileNotFoundError(f"get_stats: no *.npy or *.h5 file in {input_dir}")
    h5py = None
    if any(n.endswith(".h5") for n in names):
        try:
            import h5py
        except ImportError:
            sys.exit("get_stats: the directory holds *.h5 files and h5py is not installed; convert them to *.npy "
                     "([T, C, H, W] fp32) or install h5py")
    out = []
    for n in names:
        data = h5py.File(n, "r")["fields"] if n.endswith(".h5") else np.load(n, mmap_mode="r")
        if len(data.shape) != 4 or (out and tuple(data.shape[1:]) != tuple(out[0][1].shape[1:])):
            raise ValueError(f"get_stats: {n} has shape {tuple(data.shape)}, expected [T, C, H, W] alike in every file")
        out.append((n, data))
    return out


def local_ranges(counts, rank, size):
    """[(file index, first, one past the last)] of this rank's chunk of ``ceil(total / size)`` consecutive samples."""
    total = sum(counts)
    chunk = (total + size - 1) // size
    start, end = chunk * rank, min(chunk * rank + chunk, total)
    out, offset = [], 0
    for i, n in enumerate(counts):
        a, b = max(start, offset), min(end, offset + n)
        if a < b:
            out.append((i, a - offset, b - offset))
        offset += n
    return out


class Feeder:
    """Host slices -> device tensors: through two pinned buffers and non-blocking copies on a HIP device."""

    def __init__(self, device, shape):
        self.device = device
        self.pinned = self.events = None
        if device.type == "cuda":
            self.pinned = [torch.empty(shape, dtype=torch.float32).pin_memory() for _ in range(2)]
            self.events = [None, None]
        self.turn = 0

    def __call__(self, host):
        if self.pinned is None:
            return torch.from_numpy(np.array(host, dtype=np.float32))
        i, self.turn = self.turn, 1 - self.turn
        if self.events[i] is not None:
            self.events[i].synchronize()               # the copy that last used this buffer is done
        stage = self.pinned[i][:host.shape[0]]
        np.copyto(stage.numpy(), host, casting="same_kind")      # the file (or its mapping) straight into pinned memory
        out = stage.to(self.device, non_blocking=True)
        self.events[i] = torch.cuda.Event()
        self.events[i].record()
        return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--input_dir", type=str, required=True, help="Directory with input files.")
    ap.add_argument("--output_dir", type=str, required=True, help="Directory for saving stats files.")
    ap.add_argument("--quadrature_rule", type=str, default="naive", choices=sorted(RULES), help="Quadrature rule of the spatial averages.")
    ap.add_argument("--wind_angle", action="store_true")
    ap.add_argument("--batch_size", type=int, default=16, help="Samples read and reduced at a time.")
    ap.add_argument("--channel_names", type=str, default=None, help="JSON list of the channel names (needed by --wind_angle).")
    ap.add_argument("--carry", action="store_true", help="Form the time difference across batch and file boundaries too.")
    ap.add_argument("--device", type=str, default=None, help="Default: the local rank's HIP device, or cpu without one.")
    args = ap.parse_args(argv)
    if args.batch_size < 1:
        ap.error("--batch_size must be positive")

    from makani_amd.stats import DatasetStats, get_wind_channels

    rank, size = 0, int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.device is None:
        args.device = f"cuda:{local_rank}" if torch.cuda.is_available() else "cpu"
    device = torch.device(args.device)
    started_dist = False
    if size > 1 and not dist.is_initialized():
        if device.type == "cuda":
            torch.cuda.set_device(device)
        dist.init_process_group(backend="nccl" if device.type == "cuda" else "gloo")
        started_dist = True
    if dist.is_initialized():
        rank, size = dist.get_rank(), dist.get_world_size()

    files = open_files(args.input_dir)
    counts = [int(d.shape[0]) for _, d in files]
    C, H, W = (int(s) for s in files[0][1].shape[1:])
    wind = None
    if args.wind_angle:
        if args.channel_names is None:
            ap.error("--wind_angle needs --channel_names")
        names = json.loads(args.channel_names)
        if not isinstance(names, list) or len(names) != C:
            ap.error(f"--channel_names must be a JSON list of the {C} channel names")
        wind = get_wind_channels(names)
    if rank == 0:
        print(f"Found {len(files)} files with a total of {sum(counts)} samples. Each sample has the shape {C}x{H}x{W} (CxHxW).")

    stats = DatasetStats(C, (H, W), quadrature_rule=RULES[args.quadrature_rule], wind_pairs=wind, carry=args.carry)
    feed = Feeder(device, (args.batch_size, C, H, W))
    start, seen = time.time(), 0
    for i, first, last in local_ranges(counts, rank, size):
        data = files[i][1]
        for a in range(first, last, args.batch_size):
            b = min(a + args.batch_size, last)
            stats.update(feed(data[a:b]))
            seen += b - a
    if device.type == "cuda":
        torch.cuda.synchronize(device)
    print(f"Rank {rank} done. Duration for {seen} samples: {time.time() - start:.2f}s", flush=True)

    if size > 1:
        stats.all_reduce()
    if rank == 0:
        out = stats.save(args.output_dir)
        print("means: ", out["global_means"].reshape(-1))
        print("stds: ", out["global_stds"].reshape(-1))
    if size > 1:
        dist.barrier()
    if started_dist:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
