#!/usr/bin/env python3
"""Times the ensemble forecast products (csrc/ens_products.hip through ``makani_amd.ensemble.EnsembleProducts``) on one MI355X.

    python3 tools/ens_products_bench.py [--window 0.1] [--rounds 3] [--cases 1x4,2x4,1x16,1x50] [--out FILE.json]

At 73 x 721 x 1440, for (B, E) = (1, 4), (2, 4), (1, 16), (1, 50), with fp32 and with bf16 members (a temperature-like offset
of 250 on every third channel), the product set is mean, std, q10, median, q90 and ``above`` on every channel, de-normalised
by per-channel statistics, fp32 out.  The rows are

* ``EnsembleProducts.__call__`` with ``MK_ENS_PRODUCTS=hip`` against ``MK_ENS_PRODUCTS=torch`` (the same call on the same tensors,
  alternated in one process);
* the kernel alone (``ops.ensemble_products`` into a preallocated output) against its algorithmic bytes, the E members read once
  and the K planes written once, in TB/s;
* one line with the pinned-host bytes per step of the products against those of the members, at fp32.

Each sample is a window of back-to-back calls between one pair of device events, sized from a warm-up estimate to last at
least ``--window`` seconds; per row the median over ``--rounds`` windows (``event_timing.py``).  Before a row is timed the two
paths are compared on the plain table (no statistics) extended by the bracketing ranks ``x_(k)``, ``x_(k+1)`` of every quantile:
the exact planes (those ranks, ``above``) must be EQUAL bit for bit, the others must agree within twice the bounds of
tests/ens_products_checks.py, formed here on the device (each path is within the bound of the exact value).  It fails when no
GPU is found.  The default of ``MK_ENS_PRODUCTS`` follows DESIGN section 19: ``hip`` only if no row here is slower than the
torch path; the table of DESIGN section 46 is this tool's output.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from event_timing import timed, window, with_knob  # noqa: E402

C, H, W = 73, 721, 1440
QUANTILES = (0.1, 0.5, 0.9)


def make(B, E, dtype, dev, g):
    """members ``[B, E, C, H, W]``: draws around one centre per point"""
    off = (250.0 * (torch.arange(C, device=dev) % 3 == 0)).view(1, C, 1, 1)
    centre = torch.randn(B, C, H, W, device=dev, generator=g) + off
    ens = torch.empty(B, E, C, H, W, device=dev, dtype=dtype)
    for e in range(E):
        ens[:, e] = centre + 0.5 * torch.randn(B, C, H, W, device=dev, generator=g)
    return ens


def agree(ops, ens, thr, E):
    """The two paths on the plain table plus the bracketing ranks; returns the worst difference over twice the bound."""
    pos = [ops.quantile_position(q, E) for q in QUANTILES]
    kinds = [0, 1] + [2] * 3 + [3] + [2] * 6
    orders = [0, 0] + [k for k, _ in pos] + [0] + [r for k, t in pos for r in (k, min(k + 1, E - 1))]
    fracs = [0.0, 0.0] + [t for _, t in pos] + [0.0] * 7
    full = torch.cat([thr, torch.zeros(6, C, device=thr.device)])
    got = {}
    for mode in ("hip", "torch"):
        os.environ["MK_ENS_PRODUCTS"] = mode
        got[mode] = ops.ensemble_products(ens, kinds, orders, fracs, thr=full)
    a, b = got["hip"], got["torch"]
    for i in [5] + list(range(6, 12)) + [2 + j for j, (_, t) in enumerate(pos) if t == 0.0]:
        assert torch.equal(a[:, i].view(torch.int32), b[:, i].view(torch.int32)), ("an exact plane differs", i)
    u = 2.0 ** -53
    M = ens.abs().amax(dim=1).double()
    worst = 0.0
    for i in range(5):
        r = b[:, i].double().abs()
        lim = (2.0 ** -24 + 2.0 ** -40) * r
        if i == 0:
            lim += (E + 2) * u * M
        elif i == 1:
            lim += (E + 6) * u * r + 4 * (E + 2) * u * M
        else:
            lim += 2.0 ** -52 * (a[:, 6 + 2 * (i - 2)].double().abs() + a[:, 7 + 2 * (i - 2)].double().abs())
        worst = max(worst, float(((a[:, i].double() - b[:, i].double()).abs() / (2 * lim)).max()))
    assert worst <= 1.0, ("the two paths differ by more than twice the bound", worst)
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cases", default="1x4,2x4,1x16,1x50", help="comma-separated BxE")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ens_products_bench: no GPU found")
    from makani_amd import ops
    from makani_amd.ensemble import EnsembleProducts
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    means = [250.0 * (c % 3 == 0) + 0.01 * c for c in range(C)]
    stds = [1.0 + 0.05 * c for c in range(C)]
    rows, kernels = [], []
    print(f"{'row':>26} {'hip ms':>10} {'torch ms':>10} {'torch/hip':>9} {'diff/2bound':>11}")
    for B, E in (tuple(int(v) for v in c.split("x")) for c in args.cases.split(",")):
        for dtype in (torch.float32, torch.bfloat16):
            ens = make(B, E, dtype, dev, g)
            name = f"B={B} E={E} {str(dtype).split('.')[-1]}"
            # the event: half a standard deviation above the channel's mean, in physical units
            mod = EnsembleProducts(E, ["mean", "std"] + [("quantile", q) for q in QUANTILES]
                                   + [("above", {c: means[c] + 0.5 * stds[c] for c in range(C)})], stats=(means, stds))
            K = len(mod.names)
            worst = agree(ops, ens, mod.thresholds(C).to(dev), E)
            calls = {m: with_knob("MK_ENS_PRODUCTS", m, lambda: mod(ens)) for m in ("hip", "torch")}
            t_hip, t_torch = timed([calls["hip"], calls["torch"]], args.window, args.rounds)
            r = dict(row=name, B=B, E=E, hip_ms=round(t_hip * 1e3, 4), torch_ms=round(t_torch * 1e3, 4), ratio=round(t_torch / t_hip, 3),
                     diff_over_2bound=worst)
            rows.append(r)
            print(f"{name:>26} {r['hip_ms']:>10.3f} {r['torch_ms']:>10.3f} {r['ratio']:>9.2f} {worst:>11.2e}", flush=True)
            out = torch.empty(B, K, C, H, W, device=dev)
            call = with_knob("MK_ENS_PRODUCTS", "hip", lambda: mod(ens, out=out))
            for _ in range(2):
                call()
            torch.cuda.synchronize()
            est = window(call, 2)
            sec = float(np.median([window(call, max(10, int(args.window / est))) for _ in range(args.rounds)]))
            by = B * C * H * W * (E * ens.element_size() + K * 4)
            k = dict(kernel=name, B=B, E=E, ms=round(sec * 1e3, 4), bytes=by, TBs=round(by / sec / 1e12, 2))
            kernels.append(k)
            print(f"{'kernel: ' + name:>26} {k['ms']:>10.3f} ms {k['TBs']:>6.2f} TB/s (algorithmic)", flush=True)
            if dtype == torch.float32:
                pb, mb = B * K * C * H * W * 4, B * E * C * H * W * 4
                print(f"{'host: ' + name:>26} {pb / 1e9:>10.3f} GB of products per step against {mb / 1e9:.3f} GB of members "
                      f"({mb / pb:.1f}x)", flush=True)
            del ens, out, calls, call, mod
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(dict(tool="ens_products_bench", window_s=args.window, rounds=args.rounds, rows=rows, kernels=kernels), fh, indent=1)
    losing = [r for r in rows if r["ratio"] < 1.0]
    print(f"ens_products_bench: done, {len(losing)} of {len(rows)} rows slower than the torch path")
    for r in losing:
        print(f"  slower: {r['row']} ({r['ratio']:.2f})")


if __name__ == "__main__":
    main()
