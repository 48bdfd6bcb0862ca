#!/usr/bin/env python3
"""Times the ensemble CRPS training loss (csrc/ens.hip through ``LossHandler("fair ensemble crps")``) on one MI355X.

    python3 tools/ens_loss_bench.py [--window 0.1] [--rounds 3] [--part loss,kernel] [--cases 1x2,1x4,2x4,1x8,1x16] [--out FILE.json]

At 73 x 721 x 1440, for (B, E) = (1, 2), (1, 4), (2, 4), (1, 8), (1, 16), with fp32 and with bf16 members (a temperature-like
offset of 250 on every third channel), the rows are

* ``LossHandler("fair ensemble crps")`` forward + backward on a ``[B * E, C, H, W]`` leaf, ``MK_ENS_LOSS=hip`` against
  ``MK_ENS_LOSS=torch`` (the same call on the same tensors, alternated in one process);
* the kernels alone through the C ABI on the same operands: ``mk_ens_crps_bwd`` against its algorithmic bytes, the E members
  and the target read once and the E gradients written once, beside ``mk_ens_sums`` (the forward: members and target read
  once), both in TB/s.

Each sample is a window of back-to-back calls between one pair of device events, sized from a warm-up estimate to last at
least ``--window`` seconds; per row the median over ``--rounds`` windows (``event_timing.py``).  Before a row is timed the two
paths are compared by the bounds of the tests: the losses are fp32 roundings of float64 sums and may differ by one fp32 ulp;
every gradient element is one rounding of a float64 value on either path, so two elements differ by at most
``2 (u + 2^-40) |r|`` (u = 2^-24 for fp32, 2^-8 for bf16) plus twice the float64 bound of the tests.  It fails when no
GPU is found.  The default of ``MK_ENS_LOSS`` follows DESIGN section 19: ``hip`` only if no row here is slower than the torch
path; the table of DESIGN section 39 is this tool's output.
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
from ens_bench import make  # noqa: E402

C, H, W = 73, 721, 1440


class Params:
    loss, n_future, N_out_channels = "fair ensemble crps", 0, C
    img_shape_x = img_crop_shape_x = H
    img_shape_y = img_crop_shape_y = W
    img_crop_offset_x = img_crop_offset_y = 0
    model_grid_type = "equiangular"


def compare(gh, gt, u, floor):
    """worst |hip - torch| / (2 (u + 2^-40) |torch| + floor) over the elements, one member row at a time (float64 temporaries).
    ``floor`` ``[C, H, 1]``: twice the float64 bound of the tests, ``16 2^-53 w (|gs0| / E + 2 |gs1| / E)``, for the elements where
    the two terms cancel (fair CRPS, E = 4: the top member above the target has 1/4 - 3/12) and either path leaves its rounding."""
    worst = 0.0
    for a, b in zip(gh, gt):
        a, b = a.double(), b.double()
        err, lim = (a - b).abs(), 2 * (u + 2.0 ** -40) * b.abs() + floor
        assert bool((err[lim == 0] == 0).all()), "the paths differ where the bound is zero (a row of weight 0)"
        ratio = float((err / lim.clamp_min(1e-300)).max())
        assert ratio == ratio, "NaN in a gradient"
        worst = max(worst, ratio)
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--part", default="loss,kernel", help="comma-separated groups of rows to run")
    ap.add_argument("--cases", default="1x2,1x4,2x4,1x8,1x16", help="comma-separated BxE")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ens_loss_bench: no GPU found")
    parts = set(args.part.split(","))
    assert parts <= {"loss", "kernel"}, args.part
    from makani_amd import _lib
    from makani_amd.losses import LossHandler
    lib = _lib.load()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    rows, kernels = [], []
    print(f"{'row':>26} {'hip ms':>10} {'torch ms':>10} {'torch/hip':>9} {'err/bound':>10}")
    for B, E in (tuple(int(v) for v in c.split("x")) for c in args.cases.split(",")):
        for dtype in (torch.float32, torch.bfloat16):
            ens, tar = make(B, E, dtype, dev, g)
            name = f"B={B} E={E} {str(dtype).split('.')[-1]}"
            Params.ensemble_size = E
            handler = LossHandler(Params).to(dev).train()
            x = ens.requires_grad_(True)

            def step():
                x.grad = None
                loss = handler(x, tar, None)
                loss.backward()
                return loss.detach()

            calls = {m: with_knob("MK_ENS_LOSS", m, step) for m in ("hip", "torch")}
            res = {}
            for m in calls:
                res[m] = (float(calls[m]()), x.grad)
            ulp = float(np.spacing(np.float32(abs(res["torch"][0]))))
            assert abs(res["hip"][0] - res["torch"][0]) <= ulp, (name, "the losses of the two paths differ by more than an fp32 ulp", res)
            cw = handler.channel_weights.double().view(C, 1, 1)
            floor = 32 * 2.0 ** -53 * handler.loss_obj.wrow32.double().view(1, H, 1) * cw * (1 + handler.loss_obj.kappa) / E
            worst = compare(res["hip"][1], res["torch"][1], 2.0 ** -24 if dtype == torch.float32 else 2.0 ** -8, floor)
            assert worst <= 1.0, (name, "the gradients of the two paths differ by more than twice the bound", worst)
            del res
            if "loss" in parts:
                t_hip, t_torch = timed([calls["hip"], calls["torch"]], args.window, args.rounds)
                r = dict(row=name, B=B, E=E, hip_ms=round(t_hip * 1e3, 4), torch_ms=round(t_torch * 1e3, 4), ratio=round(t_torch / t_hip, 3),
                         err_over_bound=worst)
                rows.append(r)
                print(f"{name:>26} {r['hip_ms']:>10.3f} {r['torch_ms']:>10.3f} {r['ratio']:>9.2f} {worst:>10.2e}", flush=True)
            if "kernel" in parts:
                x.grad = None
                wrow = handler.loss_obj.wrow32
                gs = torch.randn(B, C, 2, dtype=torch.float64, device=dev, generator=g)
                gens = torch.empty_like(ens)
                ws = torch.empty(lib.mk_ens_workspace(B, C, H), dtype=torch.float64, device=dev)
                sums = torch.empty(B, C, 4, dtype=torch.float64, device=dev)
                code, chw, st = (0 if dtype == torch.float32 else 1), C * H * W, torch.cuda.current_stream().cuda_stream
                fns = {"mk_ens_crps_bwd": lambda: lib.mk_ens_crps_bwd(ens.data_ptr(), code, E * chw, chw, tar.data_ptr(), wrow.data_ptr(),
                                                                      gs.data_ptr(), gens.data_ptr(), E * chw, chw, B, E, C, H, W, st),
                       "mk_ens_sums": lambda: lib.mk_ens_sums(ens.data_ptr(), code, E * chw, chw, tar.data_ptr(), wrow.data_ptr(),
                                                              ws.data_ptr(), sums.data_ptr(), None, None, B, E, C, H, W, st)}
                nby = {"mk_ens_crps_bwd": B * chw * (2 * E * ens.element_size() + 4), "mk_ens_sums": B * chw * (E * ens.element_size() + 4)}
                for kname, call in fns.items():
                    assert call() == 0, (kname, lib.mk_last_error())
                    call()
                    torch.cuda.synchronize()
                    est = window(call, 2)
                    sec = float(np.median([window(call, max(10, int(args.window / est))) for _ in range(args.rounds)]))
                    k = dict(kernel=kname, row=name, B=B, E=E, ms=round(sec * 1e3, 4), bytes=nby[kname], TBs=round(nby[kname] / sec / 1e12, 2))
                    kernels.append(k)
                    print(f"{kname + ': ' + name:>42} {k['ms']:>10.3f} ms {k['TBs']:>6.2f} TB/s (algorithmic)", flush=True)
                del gens, ws, sums, gs
            x.grad = None
            del handler, calls, x, ens, tar
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(dict(tool="ens_loss_bench", window_s=args.window, rounds=args.rounds, rows=rows, kernels=kernels), fh, indent=1)
    losing = [r for r in rows if r["ratio"] < 1.0]
    print(f"ens_loss_bench: done, {len(losing)} of {len(rows)} rows slower than the torch path")
    for r in losing:
        print(f"  slower: {r['row']} ({r['ratio']:.2f})")


if __name__ == "__main__":
    main()
