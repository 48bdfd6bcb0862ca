#!/usr/bin/env python3
"""Times the planar transforms (RealFFT2 / InverseRealFFT2) on one MI355X: the HIP path against the torch formulation.

    python3 tools/fft2_bench.py [--window 0.3] [--rounds 3] [--grids full,low] [--out FILE.json]

Grids ``384 x 721 x 1440`` and ``384 x 240 x 480`` (channels x nlat x nlon), both with ``lmax`` 240 and ``mmax`` 241, fp32 and bf16
rows, forward alone and forward + backward, per module:

* ``hip``: ``module.forward`` with ``MK_PLANAR_FFT=hip`` -- HIP real FFT, MFMA latitude DFT and the layout pass to / from the
  public ``[B, C, lmax, mmax]`` spectrum (``packed``: ``forward_packed`` / ``inverse_packed``, the private layout the fused
  ``SpectralConv`` path uses, without that pass);
* ``torch``: ``module._forward_torch`` (``torch.fft.rfft2`` / ``irfft2`` with the ``cat`` / ``pad`` copies of the mode truncation), with
  the casts a bf16 field needs around it (``.float()`` in front of the analysis, ``.to(bfloat16)`` behind the synthesis).

The two are alternated in one process.  Each sample is a window of back-to-back calls between one pair of device events, sized
from a warm-up estimate to last at least ``--window`` seconds; per row the median over ``--rounds`` windows.  Before a row is
timed the two paths are compared on its inputs.

The latitude kernels alone (``mk_latdft_fwd`` / ``mk_latdft_inv``) are timed against their algorithmic work, both computed here
from the shapes: ``8 * lmax * nlat * mmax * BC`` flops (a complex multiply-add per table entry and column) and the bytes of one
read of the input rows, one write of the output rows and one read of the table.  It fails when no GPU is found.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRIDS = {"full": (384, 721, 1440, 240, 241), "low": (384, 240, 480, 240, 241)}      # BC, nlat, nlon, lmax, mmax


def window(fn, calls):
    """``calls`` back-to-back calls between two device events -> seconds per call."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / calls


def timed(fns, seconds, rounds):
    """Alternates the callables; per callable the median seconds per call over ``rounds`` windows of >= ``seconds``."""
    calls = []
    for f in fns:
        for _ in range(2):
            f()
        torch.cuda.synchronize()
        est = window(f, 2)
        calls.append(max(2, int(np.ceil(1.1 * seconds / est))))
    out = [[] for _ in fns]
    for _ in range(rounds):
        for f, n, ts in zip(fns, calls, out):
            ts.append(window(f, n))
    return [float(np.median(ts)) for ts in out]


def latdft_work(nlat, lmax, mmax, bc):
    """(flops, bytes) of one latitude DFT launch, either direction."""
    flops = 8 * lmax * nlat * mmax * bc
    table = 4 * 2 * lmax * ((nlat + 3) // 4 * 4)
    return flops, 8 * (nlat + lmax) * mmax * bc + table


def rel(a, b):
    a, b = a.float() if not a.is_complex() else a, b.float() if not b.is_complex() else b
    return (torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b)).item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--grids", default="full,low")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fft2_bench: no GPU found")
    os.environ["MK_PLANAR_FFT"] = "hip"        # read at call time; the torch side is called through _forward_torch
    from makani_amd import ops
    from makani_amd.layers import InverseRealFFT2, RealFFT2
    dev = torch.device("cuda:0")
    rows, kernels = [], []
    print(f"{'grid':>14} {'dtype':>5} {'module':>7} {'pass':>7} {'hip ms':>8} {'packed ms':>9} {'torch ms':>9} {'torch/hip':>9}")
    for name in args.grids.split(","):
        bc, nlat, nlon, lmax, mmax = GRIDS[name]
        f = RealFFT2(nlat, nlon, lmax=lmax, mmax=mmax).to(dev)
        fi = InverseRealFFT2(nlat, nlon, lmax=lmax, mmax=mmax).to(dev)
        torch.manual_seed(1)
        c = torch.complex(torch.randn(1, bc, lmax, mmax, device=dev), torch.randn(1, bc, lmax, mmax, device=dev)).requires_grad_(True)
        cp = ops.spec_pack_raw(c.detach().view(bc, lmax, mmax)).requires_grad_(True)
        gc = torch.complex(torch.randn(1, bc, lmax, mmax, device=dev), torch.randn(1, bc, lmax, mmax, device=dev))
        gcp = ops.spec_pack_raw(gc.view(bc, lmax, mmax))
        for dtype in (torch.float32, torch.bfloat16):
            x = torch.randn(1, bc, nlat, nlon, device=dev).to(dtype).requires_grad_(True)
            x3 = x.detach().view(bc, nlat, nlon).requires_grad_(True)
            gx = torch.randn(1, bc, nlat, nlon, device=dev).to(dtype)
            bf = dtype == torch.bfloat16

            def a_torch(v):
                return f._forward_torch(v.float() if bf else v)

            def s_hip(v):
                return fi.inverse_packed(ops.spec_pack(v.view(bc, lmax, mmax), mmax, 0), dtype).view(1, bc, nlat, nlon)

            def s_torch(v):
                y = fi._forward_torch(v)
                return y.to(dtype) if bf else y

            cases = [
                ("rfft2", lambda: f(x), lambda: f.forward_packed(x3), lambda: a_torch(x),
                 lambda: torch.autograd.grad(f(x), x, gc), lambda: torch.autograd.grad(f.forward_packed(x3), x3, gcp),
                 lambda: torch.autograd.grad(a_torch(x), x, gc)),
                ("irfft2", lambda: s_hip(c), lambda: fi.inverse_packed(cp, dtype), lambda: s_torch(c),
                 lambda: torch.autograd.grad(s_hip(c), c, gx), lambda: torch.autograd.grad(fi.inverse_packed(cp, dtype), cp, gx.view(bc, nlat, nlon)),
                 lambda: torch.autograd.grad(s_torch(c), c, gx)),
            ]
            for module, hip_f, pk_f, torch_f, hip_fb, pk_fb, torch_fb in cases:
                with torch.no_grad():       # same function on these inputs, before any timing
                    err = rel(hip_f(), torch_f())
                gerr = rel(hip_fb()[0], torch_fb()[0])
                tol = 1e-5 if not bf else 2e-2
                assert err < tol and gerr < tol, (module, err, gerr)

                def nograd(fn):
                    def run():
                        with torch.no_grad():
                            return fn()
                    return run
                for label, fns in (("fwd", (nograd(hip_f), nograd(pk_f), nograd(torch_f))), ("fwd+bwd", (hip_fb, pk_fb, torch_fb))):
                    t_hip, t_pk, t_torch = timed(fns, args.window, args.rounds)
                    r = dict(grid=[bc, nlat, nlon], lmax=lmax, mmax=mmax, dtype=str(dtype).split(".")[-1], module=module, what=label,
                             hip_ms=round(t_hip * 1e3, 4), packed_ms=round(t_pk * 1e3, 4), torch_ms=round(t_torch * 1e3, 4),
                             ratio=round(t_torch / t_hip, 3), out_err=err, grad_err=gerr)
                    rows.append(r)
                    print(f"{bc:>4}x{nlat}x{nlon:<5} {r['dtype'][:5]:>5} {module:>7} {label:>7} {r['hip_ms']:>8.3f} {r['packed_ms']:>9.3f} "
                          f"{r['torch_ms']:>9.3f} {r['ratio']:>9.2f}", flush=True)
            del x, x3, gx
            torch.cuda.empty_cache()
        # the latitude kernels alone
        xf = torch.complex(torch.randn(nlat, mmax, bc, device=dev), torch.randn(nlat, mmax, bc, device=dev))
        cs = cp.detach()
        flops, nbytes = latdft_work(nlat, lmax, mmax, bc)
        t_f, t_i = timed((lambda: ops.lat_dft_raw(xf, f.dft_table, lmax), lambda: ops.lat_idft_raw(cs, fi.dft_table, nlat)),
                         args.window, args.rounds)
        for what, t in (("mk_latdft_fwd", t_f), ("mk_latdft_inv", t_i)):
            k = dict(grid=[bc, nlat, nlon], lmax=lmax, mmax=mmax, kernel=what, ms=round(t * 1e3, 4), flops=flops, bytes=nbytes,
                     TFLOPs=round(flops / t / 1e12, 2), GBs=round(nbytes / t / 1e9, 1))
            kernels.append(k)
            print(f"{bc:>4}x{nlat}x{nlon:<5} {what}: {k['ms']:.3f} ms  {k['TFLOPs']:.2f} TFLOP/s (algorithmic)  {k['GBs']:.1f} GB/s", flush=True)
        del xf, c, cp, gc, gcp, cs, f, fi
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(dict(tool="fft2_bench", window_s=args.window, rounds=args.rounds, rows=rows, kernels=kernels), fh, indent=1)
    print("fft2_bench: done")


if __name__ == "__main__":
    main()
