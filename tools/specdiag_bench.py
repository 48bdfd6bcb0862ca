#!/usr/bin/env python3
"""Times the linear diagonal spectral filter (``SpectralConv(operator_type="diagonal")``) on one MI355X: the fused path on the
private spectrum (``MK_SPEC_DIAG=fused``) against the public path (``MK_SPEC_DIAG=public``, the default).

    python3 tools/specdiag_bench.py [--window 0.1] [--rounds 3] [--pairs planar,sht] [--grids down,low] [--batches 1,2] [--out FILE.json]
    rocprofv3 --kernel-trace --stats ... -- python3 tools/specdiag_bench.py --trace-steps 3

``SpectralConv`` with 64 channels and 180 x 180 modes (the filter of the reference's ``fno_linear_*`` configs): ``down`` =
721 x 1440 in, 360 x 720 out (the first block: a scaled residual), ``low`` = 360 x 720 in and out (an inner block); the planar
pair (``RealFFT2`` / ``InverseRealFFT2``, ``MK_PLANAR_FFT=hip``) and the SHT pair (equiangular outer, Legendre-Gauss inner grid).
fp32 and bf16 rows, B = 1 and 2, forward alone and forward + backward (input and weight):

* ``fused``: ``forward_packed``, ``ops.spec_diag`` (``mk_spec_diag_*``), ``inverse_packed``;
* ``public``: the modules' public ``forward`` (a layout pass each way), ``ops.diag_contract`` (``mk_diag_*``).

The two are alternated in one process.  Each sample is a window of back-to-back calls between one pair of device events, sized
from a warm-up estimate to last at least ``--window`` seconds; per row the median over ``--rounds`` windows.  Before a row is
timed the two paths are compared on its inputs.

The kernels alone are timed against their algorithmic bytes, computed here from the shapes: the weight (or its gradient) once,
``cin * cout * n_pos * 8`` with ``n_pos`` all 180 x 180 positions (dense) or those with l >= m (triangle), and the spectra once
each way.  ``mk_diag_*`` runs on the same operands in the public layout and is charged the same bytes.  It fails when no GPU is
found.

The tables of DESIGN section 33 are the output of ``python3 tools/specdiag_bench.py --window 0.1 --rounds 3``.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from event_timing import rel, timed, with_knob  # noqa: E402

E, LMAX, MMAX = 64, 180, 180
GRIDS = {"down": ((721, 1440), (360, 720)), "low": ((360, 720), (360, 720))}

TRACE_NET = dict(inp_shape=(240, 480), out_shape=(240, 480), scale_factor=2, inp_chans=8, out_chans=8, embed_dim=32, num_layers=2,
                 operator_type="diagonal", max_modes=(60, 60))


def trace_steps(n):
    """``n`` steps (forward + backward, batch 1, fp32) of a two-block diagonal FNO with ``MK_SPEC_DIAG=fused``: what a kernel trace
    of the fused path should list -- ``spec_diag_*`` kernels, no ``diag_*`` kernel, no ``spec_pack`` / ``spec_unpack``."""
    from makani_amd.sfnonet import FourierNeuralOperatorNet
    os.environ["MK_SPEC_DIAG"] = "fused"
    os.environ["MK_PLANAR_FFT"] = "hip"
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    net = FourierNeuralOperatorNet(**TRACE_NET).to(dev)
    x, tar = torch.randn(1, 8, 240, 480, device=dev), torch.randn(1, 8, 240, 480, device=dev)
    for _ in range(n):
        net.zero_grad(set_to_none=True)
        loss = ((net(x) - tar) ** 2).mean()
        loss.backward()
    torch.cuda.synchronize()
    print(f"specdiag_bench: {n} traced steps, loss {loss.item():.6f}")


def _pair(kind, inp, out, dev):
    from makani_amd.layers import InverseRealFFT2, RealFFT2
    from makani_amd.sht import InverseRealSHT, RealSHT
    if kind == "planar":
        return RealFFT2(*inp, lmax=LMAX, mmax=MMAX).to(dev), InverseRealFFT2(*out, lmax=LMAX, mmax=MMAX).to(dev)
    grid = lambda s: "equiangular" if s[0] % 2 else "legendre-gauss"        # 721: the model grid; 360: the inner grid
    return (RealSHT(*inp, lmax=LMAX, mmax=MMAX, grid=grid(inp)).to(dev),
            InverseRealSHT(*out, lmax=LMAX, mmax=MMAX, grid=grid(out)).to(dev))


def crandn(*shape, dev):
    return torch.complex(torch.randn(*shape, device=dev), torch.randn(*shape, device=dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pairs", default="planar,sht")
    ap.add_argument("--grids", default="down,low")
    ap.add_argument("--batches", default="1,2")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-steps", type=int, default=0,
                    help="run only that many steps of a small diagonal FNO (for rocprofv3 --kernel-trace --stats) and exit")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("specdiag_bench: no GPU found")
    if args.trace_steps:
        trace_steps(args.trace_steps)
        return
    os.environ["MK_PLANAR_FFT"] = "hip"
    from makani_amd import ops
    from makani_amd.spectral_convolution import SpectralConv
    dev = torch.device("cuda:0")
    batches = [int(b) for b in args.batches.split(",")]
    rows, kernels = [], []
    print(f"{'pair':>6} {'grid':>5} {'rows':>5} {'B':>2} {'pass':>7} {'fused ms':>9} {'public ms':>9} {'public/fused':>12}")
    for kind in [k for k in args.pairs.split(",") if k]:
        for name in [g for g in args.grids.split(",") if g]:
            inp, out = GRIDS[name]
            torch.manual_seed(1)
            mod = SpectralConv(*_pair(kind, inp, out, dev), E, E, operator_type="diagonal").to(dev)
            for dtype in (torch.float32, torch.bfloat16):
                for B in batches:
                    x = torch.randn(B, E, *inp, device=dev).to(dtype).requires_grad_(True)
                    g = torch.randn(B, E, *out, device=dev).to(dtype)

                    def fwd():
                        with torch.no_grad():
                            return mod(x)[0]

                    def fwd_bwd():
                        return torch.autograd.grad(mod(x)[0], [x, mod.weight], g)

                    f_f, p_f = with_knob("MK_SPEC_DIAG", "fused", fwd), with_knob("MK_SPEC_DIAG", "public", fwd)
                    f_fb, p_fb = with_knob("MK_SPEC_DIAG", "fused", fwd_bwd), with_knob("MK_SPEC_DIAG", "public", fwd_bwd)
                    err = rel(f_f(), p_f())          # the same function on these inputs, before any timing
                    gf, gp = f_fb(), p_fb()
                    gerr, werr = rel(gf[0], gp[0]), rel(gf[1], gp[1])
                    del gf, gp
                    tol = 1e-5 if dtype == torch.float32 else 2e-2
                    assert err < tol and gerr < tol and werr < tol, (kind, name, dtype, B, err, gerr, werr)
                    for label, fns in (("fwd", (f_f, p_f)), ("fwd+bwd", (f_fb, p_fb))):
                        t_f, t_p = timed(fns, args.window, args.rounds)
                        r = dict(pair=kind, grid=name, shape_in=[B, E, *inp], shape_out=[B, E, *out], dtype=str(dtype).split(".")[-1],
                                 batch=B, what=label, fused_ms=round(t_f * 1e3, 4), public_ms=round(t_p * 1e3, 4),
                                 ratio=round(t_p / t_f, 3), out_err=err, grad_err=gerr, wgrad_err=werr)
                        rows.append(r)
                        print(f"{kind:>6} {name:>5} {r['dtype'][:5]:>5} {B:>2} {label:>7} {r['fused_ms']:>9.3f} {r['public_ms']:>9.3f} "
                              f"{r['ratio']:>12.2f}", flush=True)
                    del x, g
                    torch.cuda.empty_cache()
            del mod
            torch.cuda.empty_cache()
    # the kernels alone, E -> E channels on the 180 x 180 spectrum
    I = O = E
    tri = sum(min(l + 1, MMAX) for l in range(LMAX))
    w = crandn(I, O, LMAX, MMAX, dev=dev)
    for B in batches:
        x, gy = crandn(LMAX, MMAX, B * I, dev=dev), crandn(LMAX, MMAX, B * O, dev=dev)
        y, gx, gw = torch.empty_like(gy), torch.empty_like(x), torch.empty_like(w)
        # the same operands in the public layout for mk_diag_*
        xs = x.view(LMAX, MMAX, B, I).permute(2, 3, 0, 1).contiguous()
        gys = gy.view(LMAX, MMAX, B, O).permute(2, 3, 0, 1).contiguous()
        ys, gxs = torch.empty_like(gys), torch.empty_like(xs)
        P = LMAX * MMAX
        for dense in (True, False):
            npos = P if dense else tri
            nbytes = 8 * npos * (I * O + B * (I + O))
            cases = [("mk_spec_diag_fwd", lambda: ops.spec_diag_fwd_raw(x, w, B, 0, 0, dense, out=y)),
                     ("mk_spec_diag_dgrad", lambda: ops.spec_diag_dgrad_raw(gy, w, B, 0, 0, dense, out=gx)),
                     ("mk_spec_diag_wgrad", lambda: ops.spec_diag_wgrad_raw(x, gy, B, 0, 0, dense, out=gw))]
            if dense:       # the public kernels have no triangle: one set of rows
                cases += [("mk_diag_fwd", lambda: ops._diag_launch("mk_diag_fwd", xs, w, ys, B, I, O, P)),
                          ("mk_diag_dgrad", lambda: ops._diag_launch("mk_diag_dgrad", gys, w, gxs, B, I, O, P)),
                          ("mk_diag_wgrad", lambda: ops._diag_launch("mk_diag_wgrad", xs, gys, gw, B, I, O, P))]
            times = timed([c[1] for c in cases], args.window, args.rounds)
            for (what, _), t in zip(cases, times):
                k = dict(kernel=what, dense=dense, batch=B, cin=I, cout=O, positions=npos, ms=round(t * 1e3, 4), bytes=nbytes,
                         TBs=round(nbytes / t / 1e12, 3))
                kernels.append(k)
                print(f"B={B} {'dense' if dense else 'triangle':>8} {what:>19}: {k['ms']:>8.3f} ms  {k['TBs']:.3f} TB/s (algorithmic bytes "
                      f"{nbytes / 1e9:.3f} GB)", flush=True)
        del x, gy, y, gx, gw, xs, gys, ys, gxs
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(dict(tool="specdiag_bench", window_s=args.window, rounds=args.rounds, rows=rows, kernels=kernels), fh, indent=1)
    losing = [r for r in rows if r["ratio"] < 1.0]
    print(f"specdiag_bench: done, {len(losing)} of {len(rows)} rows slower than the public path")


if __name__ == "__main__":
    main()
