#!/usr/bin/env python3
"""Times the spectral ensemble CRPS training loss (csrc/spec_crps.hip through ``LossHandler("fair spectral ensemble crps")``) on
one MI355X.

    python3 tools/spec_crps_bench.py [--window 0.1] [--rounds 3] [--part loss,kernel,transform] [--cases 1x2,1x4,2x4,1x8,1x16]
                                     [--out profiles/spec_crps_bench.txt]

At 73 channels on 721 x 1440 (the handler's transform is untruncated, as ``GeometricH1Loss``'s: ``lmax`` = ``mmax`` = 721), for (B, E) = (1, 2), (1, 4), (2, 4), (1, 8), (1, 16), with fp32 and with
bf16 members (a temperature-like offset of 250 on every third channel), the rows are

* ``LossHandler("fair spectral ensemble crps")`` forward + backward on a ``[B * E, C, H, W]`` leaf, ``MK_SPEC_CRPS=hip`` against
  ``MK_SPEC_CRPS=torch`` (the same call on the same tensors, alternated in one process);
* the two kernels alone through the C ABI on the spectra of the same fields, against their algorithmic bytes over the stored
  triangle only: ``mk_spec_crps_sums`` reads the E members and the target once (8 bytes each), ``mk_spec_crps_bwd`` reads
  them once and writes the E gradients once; both in TB/s;
* the transforms alone (the two ``forward_packed`` and the backward of the members' one), and their share of the hip row.

Each sample is a window of back-to-back calls between one pair of device events, sized from a warm-up estimate to last at
least ``--window`` seconds; per row the median over ``--rounds`` windows (``event_timing.py``).  Before a row is timed the two
paths are compared on the same spectra within twice the bounds of the tests: the per-degree sums within
``2 (n + 4) 2^-53 |S|``, every gradient component within ``2 (2^-24 + 2^-40) |r|`` plus twice a float64 floor for the components
whose two terms cancel, and the losses within two fp32 ulps.  It fails when no GPU is found.  The default of ``MK_SPEC_CRPS``
follows DESIGN section 19: ``hip`` only if no row here is slower than the torch path; the table of DESIGN section 43 is this
tool's output.
"""
import argparse
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
    loss, n_future, N_out_channels = "fair spectral ensemble crps", 0, C
    img_shape_x = img_crop_shape_x = H
    img_shape_y = img_crop_shape_y = W
    img_crop_offset_x = img_crop_offset_y = 0
    model_grid_type = "equiangular"


def stored(L, M, dev):
    return torch.arange(L, device=dev).reshape(L, 1) >= torch.arange(M, device=dev).reshape(1, M)


def compare(cp, ct, B, E, dev, g):
    """(worst sum error, worst gradient error) of hip against torch on the same spectra, each over TWICE the bound of the tests."""
    from makani_amd import ops
    L, M, BC = ct.shape
    gs = torch.randn(BC, L, 2, dtype=torch.float64, device=dev, generator=g)
    res = {}
    for mode in ("hip", "torch"):
        os.environ["MK_SPEC_CRPS"] = mode
        x = cp.detach().clone().requires_grad_(True)
        s = ops.spectral_crps_sums(x, ct, E, 0, 0, B)
        (s * gs).sum().backward()
        res[mode] = (s.detach(), x.grad)
    nm = stored(L, M, dev).sum(dim=1).double()
    n = torch.stack([2 * E * nm, E * (E - 1) * nm], dim=-1).reshape(1, L, 2)
    (sh, gh), (st, gt) = res["hip"], res["torch"]
    lim = 2 * (n + 4) * 2.0 ** -53 * st.abs()
    assert bool(torch.isfinite(sh).all()) and bool(torch.isfinite(gh.real).all())
    worst_s = float(((sh - st).abs() / lim.clamp_min(1e-300)).max())
    w = torch.where(torch.arange(M, device=dev) == 0, 1.0, 2.0).double().reshape(1, M, 1)
    k = (gs[..., 0].abs() / E + 2 * gs[..., 1].abs() / E).t().reshape(L, 1, B, 1, BC // B).expand(L, 1, B, E, BC // B).reshape(L, 1, B * E * (BC // B))
    floor = 32 * 2.0 ** -53 * w * k
    worst_g = 0.0
    for a, b in ((gh.real, gt.real), (gh.imag, gt.imag)):
        a, b = a.double(), b.double()
        worst_g = max(worst_g, float(((a - b).abs() / (2 * (2.0 ** -24 + 2.0 ** -40) * b.abs() + floor)).max()))
    return worst_s, worst_g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--part", default="loss,kernel,transform", help="comma-separated groups of rows to run")
    ap.add_argument("--cases", default="1x2,1x4,2x4,1x8,1x16", help="comma-separated BxE")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spec_crps_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("spec_crps_bench: no GPU found")
    parts = set(args.part.split(","))
    assert parts <= {"loss", "kernel", "transform"}, args.part
    from makani_amd import _lib
    from makani_amd.losses import LossHandler
    lib = _lib.load()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    rows = []
    say(f"spec_crps_bench: {C} x {H} x {W} (lmax {H}, mmax {W // 2 + 1}), window {args.window} s, median of {args.rounds}; device {torch.cuda.get_device_name(0)}")
    say(f"{'row':>22} {'hip ms':>9} {'torch ms':>9} {'torch/hip':>9} {'sums ms':>8} {'TB/s':>6} {'bwd ms':>8} {'TB/s':>6} {'transf ms':>9} {'share':>6} "
        f"{'S err':>8} {'g err':>8}")
    for B, E in (tuple(int(v) for v in c.split("x")) for c in args.cases.split(",")):
        for dtype in (torch.float32, torch.bfloat16):
            ens, tar = make(B, E, dtype, dev, g)
            name = f"B={B} E={E} {str(dtype).split('.')[-1]}"
            Params.ensemble_size = E
            handler = LossHandler(Params).to(dev).train()
            sht = handler.spectral_obj.sht
            L, M = sht.lmax, sht.mmax
            x = ens.requires_grad_(True)

            def step():
                x.grad = None
                loss = handler(x, tar, None)
                loss.backward()
                return loss.detach()

            calls = {m: with_knob("MK_SPEC_CRPS", m, step) for m in ("hip", "torch")}
            losses = {m: float(calls[m]()) for m in calls}
            x.grad = None
            ulp = float(np.spacing(np.float32(abs(losses["torch"]))))
            assert abs(losses["hip"] - losses["torch"]) <= 2 * ulp, (name, "the losses of the two paths differ by more than two fp32 ulps", losses)
            with torch.no_grad():
                cp = sht.forward_packed(ens.detach().reshape(-1, H, W))
                ct = sht.forward_packed(tar.reshape(-1, H, W))
            worst_s, worst_g = compare(cp, ct, B, E, dev, g)
            assert worst_s <= 1.0 and worst_g <= 1.0, (name, "the two paths differ by more than twice the bounds of the tests", worst_s, worst_g)
            r = dict(row=name, B=B, E=E, s_err=worst_s, g_err=worst_g)
            if "loss" in parts:
                t_hip, t_torch = timed([calls["hip"], calls["torch"]], args.window, args.rounds)
                r.update(hip_ms=t_hip * 1e3, torch_ms=t_torch * 1e3, ratio=t_torch / t_hip)
            x.grad = None
            if "transform" in parts:
                gc = torch.randn(cp.shape, dtype=torch.float32, device=dev, generator=g).to(torch.complex64)

                def transforms():
                    x.grad = None
                    c = sht.forward_packed(x.reshape(-1, H, W))
                    with torch.no_grad():
                        sht.forward_packed(tar.reshape(-1, H, W))
                    c.backward(gc)

                r["transform_ms"] = timed([transforms], args.window, args.rounds)[0] * 1e3
                x.grad = None
                del gc
            if "kernel" in parts:
                BC = B * C
                ncoef = int(stored(L, M, dev).sum())
                gs = torch.randn(L, BC, 2, dtype=torch.float64, device=dev, generator=g)
                gcp = torch.empty_like(cp)
                ws = torch.empty(lib.mk_spec_crps_workspace(L, M, BC), dtype=torch.float64, device=dev)
                S = torch.empty(L, BC, 2, dtype=torch.float64, device=dev)
                st = torch.cuda.current_stream().cuda_stream
                fns = {"sums": lambda: lib.mk_spec_crps_sums(cp.data_ptr(), ct.data_ptr(), ws.data_ptr(), S.data_ptr(), L, M, B, E, C, 0, 0, st),
                       "bwd": lambda: lib.mk_spec_crps_bwd(cp.data_ptr(), ct.data_ptr(), gs.data_ptr(), gcp.data_ptr(), L, M, B, E, C, 0, 0, st)}
                nby = {"sums": ncoef * BC * 8 * (E + 1), "bwd": ncoef * BC * 8 * (2 * E + 1)}
                for kname, call in fns.items():
                    assert call() == 0, (kname, lib.mk_last_error())
                    call()
                    torch.cuda.synchronize()
                    est = window(call, 2)
                    sec = float(np.median([window(call, max(10, int(args.window / est))) for _ in range(args.rounds)]))
                    r[kname + "_ms"], r[kname + "_TBs"] = sec * 1e3, nby[kname] / sec / 1e12
                del gs, gcp, ws, S
            rows.append(r)
            f = lambda key, fmt: format(r[key], fmt) if key in r else "-"
            share = format(r["transform_ms"] / r["hip_ms"], ".2f") if "transform_ms" in r and "hip_ms" in r else "-"
            say(f"{name:>22} {f('hip_ms', '9.3f'):>9} {f('torch_ms', '9.3f'):>9} {f('ratio', '9.2f'):>9} {f('sums_ms', '8.4f'):>8} {f('sums_TBs', '6.2f'):>6} "
                f"{f('bwd_ms', '8.4f'):>8} {f('bwd_TBs', '6.2f'):>6} {f('transform_ms', '9.3f'):>9} {share:>6} {worst_s:>8.1e} {worst_g:>8.1e}")
            del handler, calls, x, ens, tar, cp, ct
            torch.cuda.empty_cache()
    timed_rows = [r for r in rows if "ratio" in r]
    losing = [r for r in timed_rows if r["ratio"] < 1.0]
    say(f"spec_crps_bench: done, {len(losing)} of {len(timed_rows)} rows slower than the torch path")
    for r in losing:
        say(f"  slower: {r['row']} ({r['ratio']:.2f})")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
