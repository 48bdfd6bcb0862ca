#!/usr/bin/env python3
"""Times scaled-dot-product attention on one MI355X: the ``mk_attn_*`` kernels against ``F.scaled_dot_product_attention``.

    python3 tools/attn_bench.py [--window 0.1] [--rounds 3] [--out FILE.json]

The op alone (``ops.attention_packed`` on a bf16 ``[B, N, 3 H D]`` projection output, the layout the ViT attention module hands
over), forward and forward + backward, at

    (B, H, N, D) = (1, 8, 18540, 48)    vit_73ch: 721 x 1440 with 7 x 8 patches, embed_dim 384
                   (1, 8, 18540, 128)   vit_73ch_big
                   (2, 12, 4050, 64)    the reference's default width on 720 x 1440 with 16 x 16 patches

and one ``Attention`` module and one ``Block`` (mlp_ratio 4, bf16 autocast) at the first shape:

* ``hip``: ``MK_ATTN=hip`` -- the kernels read q, k, v in place and write the output and the gradient in their final layouts;
* ``torch``: ``MK_ATTN=torch`` -- the reference's call on the permuted views.

The two paths are alternated in one process.  Each sample is a window of back-to-back calls between one pair of device events,
sized from a warm-up estimate to last at least ``--window`` seconds; per row the median over ``--rounds`` windows.  Before a row
is timed the two paths are compared on its inputs.

The four kernels alone are printed against their algorithmic work: ``4 B H N^2 D`` flops forward and ``10 B H N^2 D`` backward,
the count of the five-product backward pass, split 6 : 4 between the dK / dV and the dQ kernel.  The kernels here recompute the
scores and dP in both (seven products): they are priced by the five-product count all the same, so the figure is comparable with
any other backward pass.  It fails when no GPU is found.

The table of DESIGN section 24 is the output of ``python3 tools/attn_bench.py --window 0.1 --rounds 3``.
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

SHAPES = [(1, 8, 18540, 48), (1, 8, 18540, 128), (2, 12, 4050, 64)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attn_bench: no GPU found")
    from makani_amd import ops
    from makani_amd.vit import Attention, Block
    dev = torch.device("cuda:0")
    rows, kernels = [], []
    torch.manual_seed(1)

    def row(name, shape, call, inputs, params, g):
        def fwd():
            with torch.no_grad():
                return call()

        def fwd_bwd():
            return torch.autograd.grad(call(), inputs + params, g)

        hip_f, torch_f = with_knob("MK_ATTN", "hip", fwd), with_knob("MK_ATTN", "torch", fwd)
        hip_fb, torch_fb = with_knob("MK_ATTN", "hip", fwd_bwd), with_knob("MK_ATTN", "torch", fwd_bwd)
        err = rel(hip_f(), torch_f())          # the same function on these inputs, before any timing (a sanity bound; tests/ has parity)
        gerr = rel(hip_fb()[0], torch_fb()[0])
        assert err < 3e-2 and gerr < 3e-2, (name, shape, err, gerr)
        for label, fns in (("fwd", (hip_f, torch_f)), ("fwd+bwd", (hip_fb, torch_fb))):
            t_hip, t_torch = timed(fns, args.window, args.rounds)
            r = dict(module=name, shape=list(shape), what=label, hip_ms=round(t_hip * 1e3, 4), torch_ms=round(t_torch * 1e3, 4),
                     ratio=round(t_torch / t_hip, 3), out_err=err, grad_err=gerr)
            rows.append(r)
            print(f"{name:>9} {str(tuple(shape)):>20} {label:>7} {r['hip_ms']:>9.3f} {r['torch_ms']:>9.3f} {r['ratio']:>9.2f}", flush=True)

    print(f"{'module':>9} {'(B, H, N, D)':>20} {'pass':>7} {'hip ms':>9} {'torch ms':>9} {'torch/hip':>9}")
    for B, H, N, D in SHAPES:
        qkv = torch.randn(B, N, 3 * H * D, device=dev).bfloat16().requires_grad_(True)
        g = torch.randn(B, N, H * D, device=dev).bfloat16()
        row("op", (B, H, N, D), lambda: ops.attention_packed(qkv, H), [qkv], [], g)
        del qkv, g
        torch.cuda.empty_cache()
    B, H, N, D = SHAPES[0]
    for name, mod in (("Attention", Attention(H * D, num_heads=H, qkv_bias=True)), ("Block", Block(H * D, H, mlp_ratio=4.0, qkv_bias=True))):
        mod = mod.to(dev)
        with torch.no_grad():
            for n, p in mod.named_parameters():
                if n.endswith("qkv.weight"):
                    p.mul_(4.0)             # scores of order 1
        x = torch.randn(B, N, H * D, device=dev).requires_grad_(True)
        g = torch.randn(B, N, H * D, device=dev)

        def call():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                return mod(x).float()

        row(name, (B, H, N, D), call, [x], list(mod.parameters()), g)
        del mod, x, g
        torch.cuda.empty_cache()
    # the kernels alone, against the five-product flop count
    for B, H, N, D in SHAPES:
        qkv = torch.randn(B, N, 3 * H * D, device=dev).bfloat16()
        q, k, v = ops._qkv_views(qkv, B, N, H, D)
        view = lambda t: t.view(B, N, H, D).permute(0, 2, 1, 3)
        o, go = (view(torch.randn(B, N, H * D, device=dev).bfloat16()) for _ in range(2))
        dq, dk, dv = ops._qkv_views(torch.empty_like(qkv), B, N, H, D)
        lse = torch.empty(B, H, N, dtype=torch.float32, device=dev)
        delta = torch.empty_like(lse)
        scale = D ** -0.5
        ops.attn_fwd_raw(q, k, v, o, lse, scale)
        lib, st = ops._lib.load(), ops._stream
        sa = ops._attn_stride_array
        s_delta, s_dkv, s_dq = sa(o, go), sa(q, k, v, go, dk, dv), sa(q, k, v, go, dq)
        import ctypes
        ptr = lambda *ts: [t.data_ptr() for t in ts]
        unit = B * H * N * N * D
        cases = [("mk_attn_fwd", lambda: ops.attn_fwd_raw(q, k, v, o, lse, scale), 4 * unit),
                 ("mk_attn_bwd_delta", lambda: lib.mk_attn_bwd_delta(*ptr(o, go, delta), B, H, N, D, ctypes.addressof(s_delta), st()), 0),
                 ("mk_attn_bwd_dkv", lambda: lib.mk_attn_bwd_dkv(*ptr(q, k, v, go, lse, delta, dk, dv), B, H, N, N, D,
                                                                 ctypes.addressof(s_dkv), scale, st()), 6 * unit),
                 ("mk_attn_bwd_dq", lambda: lib.mk_attn_bwd_dq(*ptr(q, k, v, go, lse, delta, dq), B, H, N, N, D,
                                                               ctypes.addressof(s_dq), scale, st()), 4 * unit)]
        times = timed([c[1] for c in cases], args.window, args.rounds)
        for (what, _, fl), t in zip(cases, times):
            kr = dict(kernel=what, shape=[B, H, N, D], ms=round(t * 1e3, 4), flops=fl, TFLOPs=round(fl / t / 1e12, 1))
            kernels.append(kr)
            print(f"{(B, H, N, D)} {what}: {kr['ms']:.3f} ms  {kr['TFLOPs']:.1f} TFLOP/s (algorithmic, five-product count)", flush=True)
        del qkv, o, go, dq, dk, dv
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(dict(tool="attn_bench", window_s=args.window, rounds=args.rounds, rows=rows, kernels=kernels), fh, indent=1)
    losing = [r for r in rows if r["ratio"] < 1.0]
    print(f"attn_bench: done, {len(losing)} of {len(rows)} rows slower than the torch path")


if __name__ == "__main__":
    main()
