#!/usr/bin/env python3
"""Times the dataset statistics (csrc/stats.hip through ``makani_amd.stats.DatasetStats``) on one MI355X.

    python3 tools/stats_bench.py [--window 0.1] [--rounds 3] [--part update,kernel,host] [--out FILE.json]

At 73 x 721 x 1440:

* ``DatasetStats.update`` on a batch of 16 and of 4 samples, ``MK_STATS=hip`` against ``MK_STATS=torch`` (the same call on
  the same batch, alternated in one process), with and without the 15 wind pairs of a 73-channel set and with and without
  the carry of the last sample;
* the kernel alone (``ops.field_stats`` on preallocated inputs) against its algorithmic bytes in TB/s: the batch once, the
  time sum twice (read and written), the previous sample once when it is given.  The v channel of a wind pair is read a
  second time; that is not counted, so the rows with pairs show it as lost bandwidth;
* the float64 numpy formulation of one batch of 4 samples on the host (mean, squared deviation, difference, its squared
  deviation, min, max, time mean), timed once, as a sanity figure of what the reference script spends per batch.

Each sample is a window of back-to-back calls between one pair of device events, sized from a warm-up estimate to last at
least ``--window`` seconds; per row the median over ``--rounds`` windows (``event_timing.py``).  Before a row is timed the two
paths are compared on its inputs.  It fails when no GPU is found.  The default of ``MK_STATS`` follows DESIGN section 19:
``hip`` only if no row here is slower than the torch path; the table of DESIGN section 35 is this tool's output.
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
PAIRS = ([2 * k for k in range(15)], [2 * k + 1 for k in range(15)])


def host_baseline(x, q):
    """The per-batch passes of the reference in float64 numpy; seconds."""
    t0 = time.perf_counter()
    data = x.astype(np.float64)
    quad = lambda a: (a * q).sum((-2, -1))
    mean = quad(data).mean(0)
    var = quad((data - mean[None, :, None, None]) ** 2).mean(0)
    e = data[1:] - data[:-1]
    emean = quad(e).mean(0)
    evar = quad((e - emean[None, :, None, None]) ** 2).mean(0)
    out = (data.max((0, 2, 3)), data.min((0, 2, 3)), data.mean(0), mean, var, emean, evar)
    assert all(np.isfinite(o).all() for o in out)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--part", default="update,kernel,host", help="comma-separated groups of rows to run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("stats_bench: no GPU found")
    parts = set(args.part.split(","))
    assert parts <= {"update", "kernel", "host"}, args.part
    from makani_amd import ops
    from makani_amd.stats import DatasetStats
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    scale = 1.0 + 9.0 * torch.rand(1, C, 1, 1, device=dev, generator=g)
    offset = 100.0 * torch.randn(1, C, 1, 1, device=dev, generator=g)
    rows, kernels = [], []
    print(f"{'row':>34} {'T':>3} {'hip ms':>10} {'torch ms':>10} {'torch/hip':>9}")
    for T in (16, 4):
        x = torch.randn(T, C, H, W, device=dev, generator=g) * scale + offset
        for wind in (None, PAIRS):
            for carry in (False, True):
                name = f"update{', 15 wind pairs' if wind else ''}{', carry' if carry else ''}"
                stats = {m: DatasetStats(C, (H, W), wind_pairs=wind, carry=carry) for m in ("hip", "torch")}
                calls = {m: with_knob("MK_STATS", m, (lambda s: lambda: s.update(x))(stats[m])) for m in stats}
                for m in stats:
                    calls[m]()
                    calls[m]()                                     # the second call has the carried sample
                fin = {m: stats[m].finalize() for m in stats}
                for key, v in fin["hip"].items():
                    same = np.array_equal(v, fin["torch"][key]) if key in ("mins", "maxs", "time_means") else \
                        np.allclose(v, fin["torch"][key], rtol=1e-9, atol=1e-9)
                    assert same, (name, T, key)
                if "update" in parts:
                    t_hip, t_torch = timed([calls["hip"], calls["torch"]], args.window, args.rounds)
                    r = dict(row=name, T=T, hip_ms=round(t_hip * 1e3, 4), torch_ms=round(t_torch * 1e3, 4), ratio=round(t_torch / t_hip, 3))
                    rows.append(r)
                    print(f"{name:>34} {T:>3} {r['hip_ms']:>10.3f} {r['torch_ms']:>10.3f} {r['ratio']:>9.2f}", flush=True)
                if "kernel" in parts:
                    st = stats["hip"]
                    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
                    kw = dict(prev=x[-1].clone() if carry else None, pivot=st.pivot, wind_u=i32(wind[0]) if wind else None,
                              wind_v=i32(wind[1]) if wind else None)
                    call = with_knob("MK_STATS", "hip", lambda: ops.field_stats(x, st.wrow, st.tsum, **kw))
                    for _ in range(2):
                        call()
                    sec = window(call, 10)
                    by = T * C * H * W * 4 + 2 * C * H * W * 8 + (C * H * W * 4 if carry else 0)
                    k = dict(kernel=name, T=T, ms=round(sec * 1e3, 4), bytes=by, TBs=round(by / sec / 1e12, 2))
                    kernels.append(k)
                    print(f"{'kernel: ' + name:>34} {T:>3} {k['ms']:>10.3f} ms {k['TBs']:>6.2f} TB/s (algorithmic)", flush=True)
                del stats, calls
                torch.cuda.empty_cache()
        if T == 4 and "host" in parts:
            q = DatasetStats(C, (H, W)).wrow.double().numpy().reshape(H, 1)
            sec = host_baseline(x.cpu().numpy(), q)
            print(f"{'host, float64 numpy, one batch':>34} {T:>3} {sec * 1e3:>10.0f} ms", flush=True)
            rows.append(dict(row="host, float64 numpy, one batch", T=T, host_ms=round(sec * 1e3, 1)))
        del x
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(dict(tool="stats_bench", window_s=args.window, rounds=args.rounds, rows=rows, kernels=kernels), fh, indent=1)
    losing = [r for r in rows if r.get("ratio", 1.0) < 1.0]
    print(f"stats_bench: done, {len(losing)} of {len([r for r in rows if 'ratio' in r])} rows slower than the torch path")
    for r in losing:
        print(f"  slower: {r['row']} T={r['T']} ({r['ratio']:.2f})")


if __name__ == "__main__":
    main()
