#!/usr/bin/env python3
"""Writes the per-channel value histograms of a dataset (``histograms.npz``, and ``histograms.h5`` when ``h5py`` imports) with
``makani_amd.histograms.DatasetHistograms``: the job of ``data_process/get_histograms.py``, with its arguments.

    python3 tools/get_histograms.py --input_dir DIR --output_dir DIR [--nbins 100] [--metadata_file data.json]
                                    [--stats_dir DIR | --write_stats] [--batch_size 16] [--device cuda:0]
    torchrun --nproc_per_node N tools/get_histograms.py ...        # the samples are sharded over the ranks

The histogram of channel c is ``np.histogram(x_c, bins=nbins, range=(min_c, max_c))`` over the whole dataset: ``edges
[C, nbins + 1]`` (fp32, what numpy picks for fp32 data) and ``data [C, nbins]`` (int64).  The range comes from

* ``--stats_dir``: ``mins.npy`` / ``maxs.npy`` as ``tools/get_stats.py`` writes them; the dataset is then read once;
* otherwise a first sweep with ``DatasetStats`` (its mins and maxs are those of ``np.min`` / ``np.max``), as the reference
  does; ``--write_stats`` saves the seven statistics files of that sweep into ``--output_dir`` too.

``--nbins <= 0`` means ``round(sqrt(points per channel))``, which is what the reference intends.  More than 4096 bins run
the torch formulation of ``ops.field_hist``; the tool says so.  ``--metadata_file`` (optional) is read for the channel names
of the printout only (``coords.channel``).  Input files, the sharding over ranks and the pinned-memory staging are those of
``tools/get_stats.py``; ranks are combined with ``all_reduce``, there is no MPI.  ``outside`` in the ``.npz`` counts the
points of each channel that no bin holds (below the range, above it, NaN): all zero when the range is the data's own."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from get_stats import Feeder, local_ranges, open_files  # noqa: E402


def sweep(acc, files, ranges, feed, batch_size):
    """Feed this rank's samples to ``acc.update`` in batches; returns how many there were."""
    seen = 0
    for i, first, last in ranges:
        data = files[i][1]
        for a in range(first, last, batch_size):
            b = min(a + batch_size, last)
            acc.update(feed(data[a:b]))
            seen += b - a
    return seen


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--input_dir", type=str, required=True, help="Directory with input files.")
    ap.add_argument("--metadata_file", type=str, default=None, help="File containing dataset metadata (channel names of the printout).")
    ap.add_argument("--output_dir", type=str, required=True, help="Directory for saving the histogram files.")
    ap.add_argument("--nbins", type=int, default=100, help="Number of bins for histograms; <= 0: sqrt of the points per channel.")
    ap.add_argument("--batch_size", type=int, default=16, help="Samples read and binned at a time.")
    ap.add_argument("--stats_dir", type=str, default=None, help="Directory with mins.npy and maxs.npy: skips the first sweep.")
    ap.add_argument("--write_stats", action="store_true", help="Save the statistics files of the first sweep as well.")
    ap.add_argument("--device", type=str, default=None, help="Default: the local rank's HIP device, or cpu without one.")
    args = ap.parse_args(argv)
    if args.batch_size < 1:
        ap.error("--batch_size must be positive")
    if args.write_stats and args.stats_dir is not None:
        ap.error("--write_stats needs the first sweep, which --stats_dir skips")

    from makani_amd import ops
    from makani_amd.histograms import DatasetHistograms
    from makani_amd.stats import DatasetStats

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
    names = [str(c) for c in range(C)]
    if args.metadata_file is not None:
        with open(args.metadata_file) as f:
            names = json.load(f)["coords"]["channel"]
        if len(names) != C:
            ap.error(f"--metadata_file names {len(names)} channels, the data has {C}")
    if rank == 0:
        print(f"Found {len(files)} files with a total of {sum(counts)} samples. Each sample has the shape {C}x{H}x{W} (CxHxW).")
    ranges = local_ranges(counts, rank, size)
    feed = Feeder(device, (args.batch_size, C, H, W))

    def sync():
        if device.type == "cuda":
            torch.cuda.synchronize(device)

    if args.stats_dir is not None:
        mins, maxs = (np.load(os.path.join(args.stats_dir, n + ".npy")).reshape(-1) for n in ("mins", "maxs"))
        if mins.size != C or maxs.size != C:
            ap.error(f"--stats_dir holds mins / maxs of {mins.size} / {maxs.size} channels, the data has {C}")
    else:
        start = time.time()
        stats = DatasetStats(C, (H, W))
        seen = sweep(stats, files, ranges, feed, args.batch_size)
        sync()
        print(f"Rank {rank} stats done. Duration for {seen} samples: {time.time() - start:.2f}s", flush=True)
        if size > 1:
            stats.all_reduce()
        out = stats.save(args.output_dir) if (args.write_stats and rank == 0) else stats.finalize()
        mins, maxs = out["mins"].reshape(-1), out["maxs"].reshape(-1)
    count = sum(counts) * H * W
    if rank == 0:
        print(f"Data range overview on {count} datapoints:")
        for c, mi, ma in zip(names, mins.tolist(), maxs.tolist()):
            print(f"{c}: min = {mi}, max = {ma}")

    nbins = args.nbins if args.nbins > 0 else max(1, int(round(np.sqrt(count))))
    if rank == 0 and nbins > ops.HIST_MAX_BINS:
        print(f"{nbins} bins are more than the {ops.HIST_MAX_BINS} of the HIP kernel: running the torch formulation")

    start = time.time()
    hist = DatasetHistograms(C, mins, maxs, nbins=nbins)
    seen = sweep(hist, files, ranges, feed, args.batch_size)
    sync()
    print(f"Rank {rank} histograms done. Duration for {seen} samples: {time.time() - start:.2f}s", flush=True)

    if size > 1:
        hist.all_reduce()
    if rank == 0:
        out = hist.save(args.output_dir)
        if out["outside"].any():
            print("Points that no bin holds (below the range, above it, NaN):")
            for c, (lo, hi, nan) in zip(names, out["outside"].tolist()):
                if lo or hi or nan:
                    print(f"{c}: below = {lo}, above = {hi}, nan = {nan}")
    if size > 1:
        dist.barrier()
    if started_dist:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
