#!/usr/bin/env python3
"""Times the ensemble scores (csrc/ens.hip through ``makani_amd.ensemble.EnsembleScores``) on one MI355X.

    python3 tools/ens_bench.py [--window 0.1] [--rounds 3] [--part update,kernel] [--cases 1x4,2x4,1x16,1x50] [--out FILE.json]

At 73 x 721 x 1440, for E = 4, 16 and 50 members at B = 1 and E = 4 at B = 2, with fp32 and with bf16 members (a
temperature-like offset of 250 on every third channel), the rows are

* ``EnsembleScores.update`` (the pass, the epilogue on ``[B, C]`` and the rank counts), ``MK_ENSEMBLE=hip`` against
  ``MK_ENSEMBLE=torch`` (the same call on the same tensors, alternated in one process);
* the kernel alone (``ops.ensemble_sums`` on preallocated count tensors) against its algorithmic bytes, the E members and the
  target read once, in TB/s.

Each sample is a window of back-to-back calls between one pair of device events, sized from a warm-up estimate to last at
least ``--window`` seconds; per row the median over ``--rounds`` windows (``event_timing.py``).  Before a row is timed the two
paths are compared: the sums must agree within twice the derived bound of the tests (each path is within it of the exact
value: ``4 (n + 2E + 8) 2^-53 sum w M`` for a and g, ``8 (...) sum w M^2`` for q and v, formed here on the device) and the rank
counts must be EQUAL.  It fails when no GPU is found.  The default of ``MK_ENSEMBLE`` follows DESIGN section 19: ``hip`` only if
no row here is slower than the torch path; the table of DESIGN section 38 is this tool's output.
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


class Params:
    valid_autoreg_steps, N_out_channels = 0, C
    img_shape_x = img_crop_shape_x = H
    img_shape_y = img_crop_shape_y = W
    img_crop_offset_x = img_crop_offset_y = 0
    model_grid_type, split_data_channels = "equiangular", False


def make(B, E, dtype, dev, g):
    """members ``[B * E, C, H, W]`` (the model's output layout) and the target: draws around one centre per point"""
    off = (250.0 * (torch.arange(C, device=dev) % 3 == 0)).view(1, C, 1, 1)
    centre = torch.randn(B, C, H, W, device=dev, generator=g) + off
    tar = centre + 0.5 * torch.randn(B, C, H, W, device=dev, generator=g)
    ens = torch.empty(B, E, C, H, W, device=dev, dtype=dtype)
    for e in range(E):
        ens[:, e] = centre + 0.5 * torch.randn(B, C, H, W, device=dev, generator=g)
    return ens.view(B * E, C, H, W), tar


def bound(ens, tar, wrow, B, E):
    """[B, C, 4] float64 on the device: the bound of tests/ens_checks.py"""
    M = ens.view(B, E, C, H, W).abs().amax(dim=1).double() + tar.abs().double()
    w = wrow.double().view(1, 1, H, 1)
    k = (H * W + 2 * E + 8) * 2.0 ** -53
    s1, s2 = (w * M).sum((-2, -1)), (w * M * M).sum((-2, -1))
    return torch.stack([4 * k * s1, 4 * k * s1, 8 * k * s2, 8 * k * s2], dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--part", default="update,kernel", help="comma-separated groups of rows to run")
    ap.add_argument("--cases", default="1x4,2x4,1x16,1x50", help="comma-separated BxE")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ens_bench: no GPU found")
    parts = set(args.part.split(","))
    assert parts <= {"update", "kernel"}, args.part
    from makani_amd import ops
    from makani_amd.ensemble import EnsembleScores
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    rows, kernels = [], []
    print(f"{'row':>26} {'hip ms':>10} {'torch ms':>10} {'torch/hip':>9} {'err/bound':>10}")
    for B, E in (tuple(int(v) for v in c.split("x")) for c in args.cases.split(",")):
        for dtype in (torch.float32, torch.bfloat16):
            ens, tar = make(B, E, dtype, dev, g)
            name = f"B={B} E={E} {str(dtype).split('.')[-1]}"
            acc = {m: EnsembleScores(Params, E, dev) for m in ("hip", "torch")}
            calls = {m: with_knob("MK_ENSEMBLE", m, (lambda a: lambda: a.update(ens, tar, 0))(acc[m])) for m in acc}
            for m in acc:
                calls[m]()
            lim = bound(ens, tar, acc["hip"].wrow, B, E)
            worst = float(((acc["hip"].last_sums - acc["torch"].last_sums).abs() / (2 * lim)).max())
            assert worst <= 1.0, (name, "the sums of the two paths differ by more than twice the bound", worst)
            assert torch.equal(acc["hip"].rank_histogram, acc["torch"].rank_histogram), (name, "rank counts")
            assert int(acc["hip"].rank_histogram.sum()) == B * C * H * W and not acc["hip"].skipped.any(), name
            if "update" in parts:
                t_hip, t_torch = timed([calls["hip"], calls["torch"]], args.window, args.rounds)
                r = dict(row=name, B=B, E=E, hip_ms=round(t_hip * 1e3, 4), torch_ms=round(t_torch * 1e3, 4), ratio=round(t_torch / t_hip, 3),
                         err_over_bound=worst)
                rows.append(r)
                print(f"{name:>26} {r['hip_ms']:>10.3f} {r['torch_ms']:>10.3f} {r['ratio']:>9.2f} {worst:>10.2e}", flush=True)
            if "kernel" in parts:
                a = acc["hip"]
                call = with_knob("MK_ENSEMBLE", "hip", lambda: ops.ensemble_sums(ens, tar, a.wrow, a.rank_histogram[0], a.skipped[0]))
                for _ in range(2):
                    call()
                torch.cuda.synchronize()
                est = window(call, 2)
                sec = float(np.median([window(call, max(10, int(args.window / est))) for _ in range(args.rounds)]))
                by = B * C * H * W * (E * ens.element_size() + 4)
                k = dict(kernel=name, B=B, E=E, ms=round(sec * 1e3, 4), bytes=by, TBs=round(by / sec / 1e12, 2))
                kernels.append(k)
                print(f"{'kernel: ' + name:>26} {k['ms']:>10.3f} ms {k['TBs']:>6.2f} TB/s (algorithmic)", flush=True)
            del acc, calls, ens, tar, lim
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(dict(tool="ens_bench", window_s=args.window, rounds=args.rounds, rows=rows, kernels=kernels), fh, indent=1)
    losing = [r for r in rows if r["ratio"] < 1.0]
    print(f"ens_bench: done, {len(losing)} of {len(rows)} rows slower than the torch path")
    for r in losing:
        print(f"  slower: {r['row']} ({r['ratio']:.2f})")


if __name__ == "__main__":
    main()
