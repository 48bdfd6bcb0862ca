#!/usr/bin/env python3
"""Times the non-linear spectral filter (SpectralAttention) on one MI355X: the fused HIP path against the torch formulation.

    python3 tools/specattn_bench.py [--window 0.2] [--rounds 3] [--grids down,low] [--batches 1,2] [--out FILE.json]
    rocprofv3 --kernel-trace --stats ... -- python3 tools/specattn_bench.py --trace-steps 3

``SpectralAttention`` with 384 channels, ``hidden_size_factor`` 2, one spectral layer, bias, ``cartesian`` activation, on the
240 x 241 spectrum: ``down`` = 721 x 1440 equiangular in, 240 x 480 Legendre-Gauss out (the first block of the SFNO), ``low`` =
240 x 480 in and out (an inner block).  Both operator types, fp32 and bf16 rows, B = 1 and 2, forward alone and forward + backward
(input and every parameter):

* ``hip``: ``MK_SPEC_ATTN=hip`` -- ``forward_packed``, ``ops.spec_channel_mlp`` (``mk_spec_cmlp_*``), ``inverse_packed``;
* ``torch``: ``MK_SPEC_ATTN=torch`` -- the public transforms around complex ``torch.einsum``s, bias and ``ComplexReLU`` passes.

The two are alternated in one process.  Each sample is a window of back-to-back calls between one pair of device events, sized
from a warm-up estimate to last at least ``--window`` seconds; per row the median over ``--rounds`` windows.  Before a row is
timed the two paths are compared on its inputs.

The kernels alone (384 -> 768 channels) are timed against their algorithmic work, both computed here from the shapes:
``8 * rows * I * O`` flops over the ``rows`` = B * 28,920 coefficients of the triangle, and the bytes of one read of the operand
rows, one write of the result rows and one read of the weight; the shared weight gradient also writes its partial panels and
reads them once more (twice ``mk_spec_cmlp_wgrad_workspace``).  It fails when no GPU is found.

The table of DESIGN section 20 is the output of ``python3 tools/specattn_bench.py --window 0.1 --rounds 3``.
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

E, FACTOR, LMAX, MMAX = 384, 2, 240, 241
GRIDS = {"down": ((721, 1440, "equiangular"), (240, 480, "legendre-gauss")),
         "low": ((240, 480, "legendre-gauss"), (240, 480, "legendre-gauss"))}


TRACE_NET = dict(inp_shape=(240, 480), out_shape=(240, 480), scale_factor=2, inp_chans=8, out_chans=8, embed_dim=32, num_layers=2,
                 filter_type="non-linear", operator_type="diagonal")


def trace_steps(n):
    """``n`` steps (forward + backward, batch 1, fp32) of a two-block non-linear SFNO with ``MK_SPEC_ATTN=hip``: what a kernel
    trace of the fused path should list -- no vendor GEMM, no ``spec_pack`` / ``spec_unpack``."""
    from makani_amd.sfnonet import SphericalFourierNeuralOperatorNet
    os.environ["MK_SPEC_ATTN"] = "hip"
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    net = SphericalFourierNeuralOperatorNet(**TRACE_NET).to(dev)
    x, tar = torch.randn(1, 8, 240, 480, device=dev), torch.randn(1, 8, 240, 480, device=dev)
    for _ in range(n):
        net.zero_grad(set_to_none=True)
        loss = ((net(x) - tar) ** 2).mean()
        loss.backward()
    torch.cuda.synchronize()
    print(f"specattn_bench: {n} traced steps, loss {loss.item():.6f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--grids", default="down,low")
    ap.add_argument("--batches", default="1,2")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-steps", type=int, default=0,
                    help="run only that many steps of a small non-linear SFNO (for rocprofv3 --kernel-trace --stats) and exit")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("specattn_bench: no GPU found")
    if args.trace_steps:
        trace_steps(args.trace_steps)
        return
    from makani_amd import _lib, ops
    from makani_amd.sht import InverseRealSHT, RealSHT
    from makani_amd.spectral_convolution import SpectralAttention
    dev = torch.device("cuda:0")
    batches = [int(b) for b in args.batches.split(",")]
    rows, kernels = [], []
    print(f"{'grid':>5} {'operator':>11} {'rows':>5} {'B':>2} {'pass':>7} {'hip ms':>8} {'torch ms':>9} {'torch/hip':>9}")
    for name in args.grids.split(","):
        (nlat, nlon, grid), (olat, olon, ogrid) = GRIDS[name]
        ft = RealSHT(nlat, nlon, lmax=LMAX, mmax=MMAX, grid=grid).to(dev)
        it = InverseRealSHT(olat, olon, lmax=LMAX, mmax=MMAX, grid=ogrid).to(dev)
        for operator_type in ("diagonal", "l-dependant"):
            torch.manual_seed(1)
            mod = SpectralAttention(ft, it, E, E, operator_type=operator_type, hidden_size_factor=FACTOR,
                                    complex_activation="cartesian", bias=True, spectral_layers=1).to(dev)
            params = list(mod.parameters())
            for dtype in (torch.float32, torch.bfloat16):
                for B in batches:
                    x = torch.randn(B, E, nlat, nlon, device=dev).to(dtype).requires_grad_(True)
                    g = torch.randn(B, E, olat, olon, device=dev).to(dtype)

                    def fwd():
                        with torch.no_grad():
                            return mod(x)[0]

                    def fwd_bwd():
                        return torch.autograd.grad(mod(x)[0], [x] + params, g)

                    hip_f, torch_f = with_knob("MK_SPEC_ATTN", "hip", fwd), with_knob("MK_SPEC_ATTN", "torch", fwd)
                    hip_fb, torch_fb = with_knob("MK_SPEC_ATTN", "hip", fwd_bwd), with_knob("MK_SPEC_ATTN", "torch", fwd_bwd)
                    err = rel(hip_f(), torch_f())          # the same function on these inputs, before any timing
                    gerr = rel(hip_fb()[0], torch_fb()[0])
                    # (the gradient: of the 4e7 pre-activation components a few dozen lie within fp32 rounding of zero, where the
                    # two evaluations may take different sides of the ReLU -- a sanity bound, not a parity one; tests/ has those)
                    tol = 1e-5 if dtype == torch.float32 else 2e-2
                    assert err < tol and gerr < 2e-2, (name, operator_type, dtype, B, err, gerr)
                    for label, fns in (("fwd", (hip_f, torch_f)), ("fwd+bwd", (hip_fb, torch_fb))):
                        t_hip, t_torch = timed(fns, args.window, args.rounds)
                        r = dict(grid=name, shape_in=[B, E, nlat, nlon], shape_out=[B, E, olat, olon], operator_type=operator_type,
                                 dtype=str(dtype).split(".")[-1], batch=B, what=label, hip_ms=round(t_hip * 1e3, 4),
                                 torch_ms=round(t_torch * 1e3, 4), ratio=round(t_torch / t_hip, 3), out_err=err, grad_err=gerr)
                        rows.append(r)
                        print(f"{name:>5} {operator_type:>11} {r['dtype'][:5]:>5} {B:>2} {label:>7} {r['hip_ms']:>8.3f} "
                              f"{r['torch_ms']:>9.3f} {r['ratio']:>9.2f}", flush=True)
                    del x, g
                    torch.cuda.empty_cache()
            del mod, params
            torch.cuda.empty_cache()
        del ft, it
    # the kernels alone: one layer 384 -> 768 on the triangle of the 240 x 241 spectrum
    I, O = E, E * FACTOR
    tri = sum(min(l + 1, MMAX) for l in range(LMAX))
    for B in batches:
        nrows = B * tri
        x = torch.complex(torch.randn(LMAX, MMAX, B * I, device=dev), torch.randn(LMAX, MMAX, B * I, device=dev))
        gy = torch.complex(torch.randn(LMAX, MMAX, B * O, device=dev), torch.randn(LMAX, MMAX, B * O, device=dev))
        bias = torch.complex(torch.randn(O, device=dev), torch.randn(O, device=dev))
        for per_degree in (False, True):
            w = torch.complex(torch.randn(*((LMAX,) if per_degree else ()), I, O, device=dev),
                              torch.randn(*((LMAX,) if per_degree else ()), I, O, device=dev))
            wbytes = 8 * w.numel()
            # the shared weight gradient writes its partial panels and the fixed-order pass reads them again
            pbytes = 2 * _lib.load().mk_spec_cmlp_wgrad_workspace(LMAX, I, O, int(per_degree))
            flops = 8 * nrows * I * O
            cases = [("mk_spec_cmlp_fwd", lambda: ops.spec_cmlp_fwd_raw(x, w, bias, B, 2), flops, 8 * nrows * (I + O) + wbytes),
                     ("mk_spec_cmlp_dgrad", lambda: ops.spec_cmlp_dgrad_raw(gy, w, x, B, 2), flops, 8 * nrows * (2 * I + O) + wbytes),
                     ("mk_spec_cmlp_wgrad", lambda: ops.spec_cmlp_wgrad_raw(x, gy, B, per_degree), flops,
                      8 * nrows * (I + O) + wbytes + pbytes)]
            if not per_degree:
                cases.append(("mk_spec_cmlp_bgrad", lambda: ops.spec_cmlp_bgrad_raw(gy, B), 2 * nrows * O, 8 * nrows * O))
            times = timed([c[1] for c in cases], args.window, args.rounds)
            for (what, _, fl, nb), t in zip(cases, times):
                k = dict(kernel=what, per_degree=per_degree, batch=B, cin=I, cout=O, rows=nrows, ms=round(t * 1e3, 4), flops=fl, bytes=nb,
                         TFLOPs=round(fl / t / 1e12, 2), GBs=round(nb / t / 1e9, 1))
                kernels.append(k)
                print(f"B={B} {'per-degree' if per_degree else 'shared':>10} {what}: {k['ms']:.3f} ms  {k['TFLOPs']:.2f} TFLOP/s "
                      f"(algorithmic)  {k['GBs']:.1f} GB/s", flush=True)
            del w
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(dict(tool="specattn_bench", window_s=args.window, rounds=args.rounds, rows=rows, kernels=kernels), fh, indent=1)
    losing = [r for r in rows if r["ratio"] < 1.0]
    print(f"specattn_bench: done, {len(losing)} of {len(rows)} rows slower than the torch path")


if __name__ == "__main__":
    main()
