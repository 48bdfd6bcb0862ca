#!/usr/bin/env python3
"""Times the channels-last AFNO filter and block on one MI355X: the fused HIP path against the reference's formulation in torch ops.

    python3 tools/afnov1_bench.py [--window 0.2] [--rounds 3] [--batches 1,2,4] [--out FILE.json]
    rocprofv3 --kernel-trace --stats ... -- python3 tools/afnov1_bench.py --trace-steps 3

``AFNO2D`` (``makani_amd/afnonet_v1.py``) on fp32 tokens and one ``Block`` (layer norms, mlp_ratio 4) under bf16 autocast, at 768
channels in 8 blocks of 96 on the 90 x 180 grid (720 x 1440 with 8 x 8 patches), soft-shrink threshold 0.01, fp32 tokens, B = 1, 2
and 4, forward alone and forward + backward (input and every parameter):

* ``hip``: ``MK_AFNOV1=hip`` -- ``mk_tokens_to_fields``, ``forward_packed`` on the window table, ``ops.spec_block_mlp`` with biases,
  ``inverse_packed``, ``mk_fields_to_tokens`` with the addend;
* ``torch``: ``MK_AFNOV1=torch`` -- ``AFNO2D._forward_torch``: ``rfft2`` over the middle axes, the reference's eight real einsums,
  the zeros buffers and slice assignments, ``softshrink``, ``irfft2``, one add.  This is the baseline, pinned to the reference by
  ``tests/test_afnov1_cpu.py``.

``MK_PLANAR_FFT=hip`` is set for the whole run (the fused path needs the HIP transform pair); ``MK_TOKEN_NORM`` / ``MK_TOKEN_LINEAR``
stay as given, the same for both paths.  The two paths are alternated in one process.  Each sample is a window of back-to-back
calls between one pair of device events, sized from a warm-up estimate to last at least ``--window`` seconds; per row the median
over ``--rounds`` windows.  Before a row is timed the two paths are compared on its inputs.

The two layout kernels alone are timed against their algorithmic bytes, computed here from the shape: one read and one write of
the ``B x 16200 x 768`` fp32 operand (``mk_fields_to_tokens`` with its addend: one read more).  It fails when no GPU is found.

The table of DESIGN section 27 is the output of ``python3 tools/afnov1_bench.py --window 0.1 --rounds 3``.
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

E, NB, H, W, LAM = 768, 8, 90, 180, 0.01


TRACE_NET = dict(inp_shape=(96, 192), patch_size=(4, 4), inp_chans=4, out_chans=4, embed_dim=32, num_layers=2, num_blocks=4,
                 sparsity_threshold=LAM)


def trace_steps(n):
    """``n`` steps (forward + backward, batch 1, fp32) of a two-block AFNOv1 with ``MK_AFNOV1=hip``: what a kernel trace of the fused
    path should list -- the layout passes, the FFT rows, the latitude DFT, ``spec_bdmlp_*``, the bias-gradient sums and no vendor
    GEMM or FFT inside the filter."""
    from makani_amd.afnonet_v1 import AdaptiveFourierNeuralOperatorNet
    os.environ["MK_AFNOV1"] = "hip"
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    net = AdaptiveFourierNeuralOperatorNet(**TRACE_NET).to(dev)
    x, tar = torch.randn(1, 4, 96, 192, device=dev), torch.randn(1, 4, 96, 192, device=dev)
    for _ in range(n):
        net.zero_grad(set_to_none=True)
        loss = ((net(x) - tar) ** 2).mean()
        loss.backward()
    torch.cuda.synchronize()
    print(f"afnov1_bench: {n} traced steps, loss {loss.item():.6f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", default="1,2,4")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-steps", type=int, default=0,
                    help="run only that many steps of a small AFNOv1 (for rocprofv3 --kernel-trace --stats) and exit")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("afnov1_bench: no GPU found")
    os.environ["MK_PLANAR_FFT"] = "hip"
    if args.trace_steps:
        trace_steps(args.trace_steps)
        return
    from makani_amd import ops
    from makani_amd.afnonet_v1 import AFNO2D, Block
    dev = torch.device("cuda:0")
    batches = [int(b) for b in args.batches.split(",")]
    rows, kernels = [], []
    torch.manual_seed(1)
    mods = {"AFNO2D": AFNO2D(E, NB, LAM, 1.0).to(dev), "Block": Block(E, num_blocks=NB, sparsity_threshold=LAM).to(dev)}
    with torch.no_grad():       # the init's 0.02 leaves every coefficient below the threshold: weights that keep the filter active
        for m in (mods["AFNO2D"], mods["Block"].filter):
            for p, std in ((m.w1, 0.1), (m.w2, 0.1), (m.b1, 0.3), (m.b2, 0.3)):
                p.copy_(torch.randn_like(p) * std)
    print(f"{'module':>7} {'B':>2} {'pass':>7} {'hip ms':>8} {'torch ms':>9} {'torch/hip':>9}")
    for name, mod in mods.items():
        params = list(mod.parameters())
        autocast = name == "Block"
        for B in batches:
            x = torch.randn(B, H, W, E, device=dev).requires_grad_(True)
            g = torch.randn(B, H, W, E, device=dev)

            def call():
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                    return mod(x)

            def fwd():
                with torch.no_grad():
                    return call()

            def fwd_bwd():
                y = call()
                return torch.autograd.grad(y, [x] + params, g.to(y.dtype))

            hip_f, torch_f = with_knob("MK_AFNOV1", "hip", fwd), with_knob("MK_AFNOV1", "torch", fwd)
            hip_fb, torch_fb = with_knob("MK_AFNOV1", "hip", fwd_bwd), with_knob("MK_AFNOV1", "torch", fwd_bwd)
            err = rel(hip_f(), torch_f())          # the same function on these inputs, before any timing
            gerr = rel(hip_fb()[0], torch_fb()[0])
            # (sanity bounds, not parity ones -- tests/ has those: under autocast the torch path's einsums run in bf16, and of the
            # 1e7 masked components a few lie within rounding of an edge, where the two evaluations may take different sides)
            assert err < (1e-1 if autocast else 1e-5) and gerr < (1e-1 if autocast else 3e-2), (name, B, err, gerr)
            for label, fns in (("fwd", (hip_f, torch_f)), ("fwd+bwd", (hip_fb, torch_fb))):
                t_hip, t_torch = timed(fns, args.window, args.rounds)
                r = dict(module=name, shape=[B, H, W, E], autocast=autocast, batch=B, what=label, hip_ms=round(t_hip * 1e3, 4),
                         torch_ms=round(t_torch * 1e3, 4), ratio=round(t_torch / t_hip, 3), out_err=err, grad_err=gerr)
                rows.append(r)
                print(f"{name:>7} {B:>2} {label:>7} {r['hip_ms']:>8.3f} {r['torch_ms']:>9.3f} {r['ratio']:>9.2f}", flush=True)
            del x, g
            torch.cuda.empty_cache()
    del mods
    torch.cuda.empty_cache()
    # the layout kernels alone
    N = H * W
    for B in batches:
        tok, fld, add = torch.randn(B, N, E, device=dev), torch.randn(B, E, N, device=dev), torch.randn(B, N, E, device=dev)
        out_f, out_t = torch.empty_like(fld), torch.empty_like(tok)
        field = 4 * B * N * E
        cases = [("mk_tokens_to_fields", lambda: ops.tokens_to_fields_raw(tok, out_f), 2 * field),
                 ("mk_fields_to_tokens", lambda: ops.fields_to_tokens_raw(fld, None, out_t), 2 * field),
                 ("mk_fields_to_tokens+addend", lambda: ops.fields_to_tokens_raw(fld, add, out_t), 3 * field)]
        times = timed([c[1] for c in cases], args.window, args.rounds)
        for (what, _, nbytes), t in zip(cases, times):
            k = dict(kernel=what, batch=B, n=N, c=E, ms=round(t * 1e3, 4), bytes=nbytes, GBs=round(nbytes / t / 1e9, 1))
            kernels.append(k)
            print(f"B={B} {what}: {k['ms']:.3f} ms  {k['GBs']:.1f} GB/s (algorithmic)", flush=True)
        del tok, fld, add, out_f, out_t
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(dict(tool="afnov1_bench", window_s=args.window, rounds=args.rounds, rows=rows, kernels=kernels), fh, indent=1)
    losing = [r for r in rows if r["ratio"] < 1.0]
    print(f"afnov1_bench: done, {len(losing)} of {len(rows)} rows slower than the torch path")


if __name__ == "__main__":
    main()
