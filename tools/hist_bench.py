#!/usr/bin/env python3
"""Times the dataset histograms (csrc/hist.hip through ``makani_amd.histograms.DatasetHistograms``) on one MI355X.

    python3 tools/hist_bench.py [--window 0.1] [--rounds 3] [--part update,kernel,host] [--samples 16,4] [--out FILE.json]

At 73 x 721 x 1440, with 100, 1000 and 4096 bins over each channel's own range, for three data sets:

* ``gaussian``: per-channel normal values with their own scale and offset (the realistic case: smooth and peaked);
* ``uniform``: every bin of the range equally likely (the least contention);
* ``constant``: every point of a channel holds one value, so all of them land in ONE bin (the contention worst case);

the rows are

* ``DatasetHistograms.update`` on a batch of 16 and of 4 samples, ``MK_HIST=hip`` against ``MK_HIST=torch`` (the same call on
  the same batch, alternated in one process);
* the kernel alone (``ops.field_hist`` on preallocated tensors) against its algorithmic bytes, the batch read once, in TB/s;
* ``np.histogram`` of one batch of 4 samples on the host, channel by channel, timed once (gaussian, 100 bins): what the
  reference spends per batch.

Each sample is a window of back-to-back calls between one pair of device events, sized from a warm-up estimate to last at
least ``--window`` seconds; per row the median over ``--rounds`` windows (``event_timing.py``).  Before a row is timed the
counts of the two paths are compared: they must be EQUAL.  It fails when no GPU is found.  The default of ``MK_HIST``
follows DESIGN section 19: ``hip`` only if no row here is slower than the torch path; the table of DESIGN section 36 is this
tool's output.  ``MK_LIB_OVERRIDE`` runs the kernel rows on another build (the replica / merge A/B of section 36).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from event_timing import timed, window, with_knob  # noqa: E402

C, H, W = 73, 721, 1440
NBINS = (100, 1000, 4096)
DATA = ("gaussian", "uniform", "constant")


def make(kind, T, dev, g):
    scale = 1.0 + 9.0 * torch.rand(1, C, 1, 1, device=dev, generator=g)
    offset = 100.0 * torch.randn(1, C, 1, 1, device=dev, generator=g)
    if kind == "gaussian":
        return torch.randn(T, C, H, W, device=dev, generator=g) * scale + offset
    if kind == "uniform":
        return (torch.rand(T, C, H, W, device=dev, generator=g) - 0.5) * scale + offset
    return (offset + torch.zeros(T, C, H, W, device=dev)).contiguous()


def host_baseline(x, lo, hi, nbins):
    """``np.histogram`` per channel over one batch on the host; seconds."""
    t0 = time.perf_counter()
    total = 0
    for c in range(x.shape[1]):
        total += int(np.histogram(x[:, c], bins=nbins, range=(float(lo[c]), float(hi[c])))[0].sum())
    assert total == x.size
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--part", default="update,kernel,host", help="comma-separated groups of rows to run")
    ap.add_argument("--samples", default="16,4", help="comma-separated batch sizes")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("hist_bench: no GPU found")
    parts = set(args.part.split(","))
    assert parts <= {"update", "kernel", "host"}, args.part
    from makani_amd import ops
    from makani_amd.histograms import DatasetHistograms
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    rows, kernels = [], []
    print(f"{'row':>34} {'T':>3} {'hip ms':>10} {'torch ms':>10} {'torch/hip':>9}")
    for T in (int(t) for t in args.samples.split(",")):
        for kind in DATA:
            x = make(kind, T, dev, g)
            lo, hi = x.amin((0, 2, 3)).cpu().numpy(), x.amax((0, 2, 3)).cpu().numpy()
            for nbins in NBINS:
                name = f"{kind}, {nbins} bins"
                acc = {m: DatasetHistograms(C, lo, hi, nbins=nbins) for m in ("hip", "torch")}
                calls = {m: with_knob("MK_HIST", m, (lambda a: lambda: a.update(x))(acc[m])) for m in acc}
                for m in acc:
                    calls[m]()
                fin = {m: acc[m].finalize() for m in acc}
                for key in ("edges", "data", "outside"):
                    assert np.array_equal(fin["hip"][key], fin["torch"][key]), (name, T, key)
                assert int(fin["hip"]["data"].sum()) == T * C * H * W and not fin["hip"]["outside"].any(), (name, T)
                if "update" in parts:
                    t_hip, t_torch = timed([calls["hip"], calls["torch"]], args.window, args.rounds)
                    r = dict(row=name, T=T, hip_ms=round(t_hip * 1e3, 4), torch_ms=round(t_torch * 1e3, 4), ratio=round(t_torch / t_hip, 3))
                    rows.append(r)
                    print(f"{name:>34} {T:>3} {r['hip_ms']:>10.3f} {r['torch_ms']:>10.3f} {r['ratio']:>9.2f}", flush=True)
                if "kernel" in parts:
                    a = acc["hip"]
                    call = with_knob("MK_HIST", "hip", lambda: ops.field_hist(x, a.edges64, a.counts, a.outside))
                    for _ in range(2):
                        call()
                    torch.cuda.synchronize()
                    est = window(call, 2)
                    sec = float(np.median([window(call, max(10, int(args.window / est))) for _ in range(args.rounds)]))
                    by = T * C * H * W * 4
                    k = dict(kernel=name, T=T, ms=round(sec * 1e3, 4), bytes=by, TBs=round(by / sec / 1e12, 2))
                    kernels.append(k)
                    print(f"{'kernel: ' + name:>34} {T:>3} {k['ms']:>10.3f} ms {k['TBs']:>6.2f} TB/s (algorithmic)", flush=True)
                del acc, calls
            if T == 4 and kind == "gaussian" and "host" in parts:
                sec = host_baseline(x.cpu().numpy(), lo, hi, 100)
                print(f"{'host, np.histogram, one batch':>34} {T:>3} {sec * 1e3:>10.0f} ms", flush=True)
                rows.append(dict(row="host, np.histogram, one batch, 100 bins", T=T, host_ms=round(sec * 1e3, 1)))
            del x
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(dict(tool="hist_bench", window_s=args.window, rounds=args.rounds, rows=rows, kernels=kernels), fh, indent=1)
    losing = [r for r in rows if r.get("ratio", 1.0) < 1.0]
    print(f"hist_bench: done, {len(losing)} of {len([r for r in rows if 'ratio' in r])} rows slower than the torch path")
    for r in losing:
        print(f"  slower: {r['row']} T={r['T']} ({r['ratio']:.2f})")


if __name__ == "__main__":
    main()
