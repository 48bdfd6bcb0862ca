#!/usr/bin/env python3
"""Times the AFNO filter and block on one MI355X: the fused HIP path against the reference's formulation in torch ops.

    python3 tools/afno_bench.py [--window 0.2] [--rounds 3] [--batches 1,2,4] [--out FILE.json]
    rocprofv3 --kernel-trace --stats ... -- python3 tools/afno_bench.py --trace-steps 3

``AFNO2D`` and one ``Block`` (instance norm, linear skip, mlp_ratio 4) at 768 channels in 8 blocks of 96 on the 90 x 180 grid
(720 x 1440 with 8 x 8 patches), soft-shrink threshold 0.01, fp32 and bf16 inputs (the block under bf16 autocast), B = 1, 2 and 4,
forward alone and forward + backward (input and every parameter):

* ``hip``: ``MK_AFNO=hip`` -- ``forward_packed``, ``ops.spec_block_mlp`` (``mk_spec_bdmlp_*``), ``inverse_packed``, one
  ``mk_affine_add`` pass;
* ``torch``: ``MK_AFNO=torch`` -- ``AFNO2D._forward_torch``: ``rfft2``, the reference's einsums, the zeros buffer and slice
  assignments, ``softshrink``, ``irfft2``, two adds.  This is the baseline, pinned to the reference by ``tests/test_afno_cpu.py``.

``MK_PLANAR_FFT=hip`` is set for the whole run (the fused path needs the HIP transform pair).  The two paths are alternated in
one process.  Each sample is a window of back-to-back calls between one pair of device events, sized from a warm-up estimate to
last at least ``--window`` seconds; per row the median over ``--rounds`` windows.  Before a row is timed the two paths are
compared on its inputs.

The kernels alone (8 blocks of 96 -> 96) are timed against their algorithmic work, both computed here from the shapes:
``8 * rows * ib * ob * nb`` flops over the ``rows`` = B * 90 * 91 coefficients, and the bytes of one read of the operand rows, one
write of the result rows and one read of the weights; the masked data gradient also reads the saved activation, the weight
gradient also writes its partial panels and reads them once more (twice ``mk_spec_bdmlp_wgrad_workspace``), the mask pass reads
two fields and writes one.  It fails when no GPU is found.

The table of DESIGN section 22 is the output of ``python3 tools/afno_bench.py --window 0.1 --rounds 3``.
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
    """``n`` steps (forward + backward, batch 1, fp32) of a two-block AFNO with ``MK_AFNO=hip``: what a kernel trace of the fused
    path should list -- the FFT rows, the latitude DFT, ``spec_bdmlp_*`` and no vendor GEMM or FFT inside the filter."""
    from makani_amd.afnonet import AdaptiveFourierNeuralOperatorNet
    os.environ["MK_AFNO"] = "hip"
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    net = AdaptiveFourierNeuralOperatorNet(**TRACE_NET).to(dev)
    x, tar = torch.randn(1, 4, 96, 192, device=dev), torch.randn(1, 4, 96, 192, device=dev)
    for _ in range(n):
        net.zero_grad(set_to_none=True)
        loss = ((net(x) - tar) ** 2).mean()
        loss.backward()
    torch.cuda.synchronize()
    print(f"afno_bench: {n} traced steps, loss {loss.item():.6f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", default="1,2,4")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-steps", type=int, default=0,
                    help="run only that many steps of a small AFNO (for rocprofv3 --kernel-trace --stats) and exit")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("afno_bench: no GPU found")
    os.environ["MK_PLANAR_FFT"] = "hip"
    if args.trace_steps:
        trace_steps(args.trace_steps)
        return
    from functools import partial
    from makani_amd import _lib, ops
    from makani_amd.afnonet import AFNO2D, Block
    from makani_amd.layers import InstanceNorm2d
    dev = torch.device("cuda:0")
    batches = [int(b) for b in args.batches.split(",")]
    rows, kernels = [], []
    torch.manual_seed(1)
    norm = partial(InstanceNorm2d, num_features=E, eps=1e-6, affine=True, track_running_stats=False)
    mods = {"AFNO2D": AFNO2D(E, NB, LAM, 1.0, use_complex_kernels=True).to(dev),
            "Block": Block(H, W, E, norm_layer=norm, num_blocks=NB, sparsity_threshold=LAM, verbose=False).to(dev)}
    with torch.no_grad():       # the init's 0.02 leaves every coefficient below the threshold: weights that keep the filter active
        for m in (mods["AFNO2D"], mods["Block"].filter):
            m.w1.copy_(torch.randn_like(m.w1) * 0.1)
            m.w2.copy_(torch.randn_like(m.w2) * 0.1)
    print(f"{'module':>7} {'rows':>5} {'B':>2} {'pass':>7} {'hip ms':>8} {'torch ms':>9} {'torch/hip':>9}")
    for name, mod in mods.items():
        params = list(mod.parameters())
        for dtype in (torch.float32, torch.bfloat16):
            autocast = name == "Block" and dtype == torch.bfloat16
            for B in batches:
                x = torch.randn(B, E, H, W, device=dev).to(dtype).requires_grad_(True)
                g = torch.randn(B, E, H, W, device=dev)

                def call():
                    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                        return mod(x)

                def fwd():
                    with torch.no_grad():
                        return call()

                def fwd_bwd():
                    y = call()
                    return torch.autograd.grad(y, [x] + params, g.to(y.dtype))

                hip_f, torch_f = with_knob("MK_AFNO", "hip", fwd), with_knob("MK_AFNO", "torch", fwd)
                hip_fb, torch_fb = with_knob("MK_AFNO", "hip", fwd_bwd), with_knob("MK_AFNO", "torch", fwd_bwd)
                err = rel(hip_f(), torch_f())          # the same function on these inputs, before any timing
                gerr = rel(hip_fb()[0], torch_fb()[0])
                # (the gradient: of the 1e7 masked components a few lie within fp32 rounding of an edge, where the two evaluations
                # may take different sides -- a sanity bound, not a parity one; tests/ has those)
                tol = 1e-5 if dtype == torch.float32 else 3e-2
                assert err < tol and gerr < 3e-2, (name, dtype, B, err, gerr)
                for label, fns in (("fwd", (hip_f, torch_f)), ("fwd+bwd", (hip_fb, torch_fb))):
                    t_hip, t_torch = timed(fns, args.window, args.rounds)
                    r = dict(module=name, shape=[B, E, H, W], dtype=str(dtype).split(".")[-1], batch=B, what=label,
                             hip_ms=round(t_hip * 1e3, 4), torch_ms=round(t_torch * 1e3, 4), ratio=round(t_torch / t_hip, 3),
                             out_err=err, grad_err=gerr)
                    rows.append(r)
                    print(f"{name:>7} {r['dtype'][:5]:>5} {B:>2} {label:>7} {r['hip_ms']:>8.3f} {r['torch_ms']:>9.3f} "
                          f"{r['ratio']:>9.2f}", flush=True)
                del x, g
                torch.cuda.empty_cache()
    del mods
    torch.cuda.empty_cache()
    # the kernels alone: 8 blocks of 96 -> 96 on the 90 x 91 spectrum
    ib = ob = E // NB
    L, M = H, W // 2 + 1
    for B in batches:
        nrows = B * L * M

        def crand(*s):
            return torch.complex(torch.randn(*s, device=dev), torch.randn(*s, device=dev))

        x, gy, w = crand(L, M, B * E), crand(L, M, B * E), crand(NB, ib, ob)
        s = ops.spec_bdmlp_fwd_raw(x, w, 3, 10.0)
        flops, field, wbytes = 8 * nrows * ib * ob * NB, 8 * nrows * E, 8 * w.numel()
        pbytes = 2 * _lib.load().mk_spec_bdmlp_wgrad_workspace(nrows, NB, ib, ob)
        cases = [("mk_spec_bdmlp_fwd", lambda: ops.spec_bdmlp_fwd_raw(x, w, 3, LAM), flops, 2 * field + wbytes),
                 ("mk_spec_bdmlp_dgrad", lambda: ops.spec_bdmlp_dgrad_raw(gy, w, a=x), flops, 3 * field + wbytes),
                 ("mk_spec_bdmlp_wgrad", lambda: ops.spec_bdmlp_wgrad_raw(x, gy, B, NB), flops, 2 * field + wbytes + pbytes),
                 ("mk_spec_bdmlp_mask", lambda: ops.spec_bdmlp_mask_raw(gy, s), 0, 3 * field)]
        times = timed([c[1] for c in cases], args.window, args.rounds)
        for (what, _, fl, nbytes), t in zip(cases, times):
            k = dict(kernel=what, batch=B, nb=NB, ib=ib, ob=ob, rows=nrows, ms=round(t * 1e3, 4), flops=fl, bytes=nbytes,
                     TFLOPs=round(fl / t / 1e12, 2), GBs=round(nbytes / t / 1e9, 1))
            kernels.append(k)
            print(f"B={B} {what}: {k['ms']:.3f} ms  {k['TFLOPs']:.2f} TFLOP/s (algorithmic)  {k['GBs']:.1f} GB/s", flush=True)
        del x, gy, w, s
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(dict(tool="afno_bench", window_s=args.window, rounds=args.rounds, rows=rows, kernels=kernels), fh, indent=1)
    losing = [r for r in rows if r["ratio"] < 1.0]
    print(f"afno_bench: done, {len(losing)} of {len(rows)} rows slower than the torch path")


if __name__ == "__main__":
    main()
