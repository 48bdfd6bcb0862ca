#!/usr/bin/env python3
"""Times fp32 attention on one MI355X: the ``mk_attn_x3_*`` kernels (fp32 operands on the bf16x3 arithmetic) against
``F.scaled_dot_product_attention`` on the same fp32 operands WITHOUT autocast -- what runs with the knob at ``torch``.  The fp32
sibling of tools/attn_bench.py.

    python3 tools/attn_fp32_bench.py [--window 0.1] [--rounds 3] [--out FILE.json]
    rocprofv3 --kernel-trace --stats ... -- python3 tools/attn_fp32_bench.py --trace-steps 3

Rows, each forward and forward + backward, everything fp32:

* ``ops.attention_packed`` at (B, H, N, D) = (1, 8, 18540, 48) (``vit_73ch``), (1, 8, 18540, 128) (``vit_73ch_big``; a head size
  the kernels decline runs the torch call on both sides and is marked so) and (2, 12, 4050, 64);
* one ViT ``Attention`` and one ``Block`` at 18 540 x 384, 8 heads, with ``MK_TOKEN_LINEAR_FP32=hip`` on both sides.

``hip``: ``MK_ATTN_FP32=hip``; ``torch``: ``MK_ATTN_FP32=torch``.  The two paths are alternated in one process, timed as
tools/event_timing.py does; before a row is timed the two paths are compared on its inputs.  Then the four kernels alone, against
``4 B H N^2 D`` flops forward (dQ the same, dK / dV ``6 B H N^2 D``: ``10 B H N^2 D`` backward).  It fails when no GPU is found.

The table of DESIGN section 31 is the output of ``python3 tools/attn_fp32_bench.py --window 0.05 --rounds 3``.
"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from event_timing import rel, timed, with_knob  # noqa: E402

KNOB = "MK_ATTN_FP32"
SHAPES = [(1, 8, 18540, 48), (1, 8, 18540, 128), (2, 12, 4050, 64)]
MODULE = (1, 18540, 384, 8)             # B, N, C, heads


def trace_steps(n):
    """``n`` fp32 training steps (no autocast) of a two-block ViT with ``MK_ATTN_FP32=hip``, ``MK_TOKEN_LINEAR_FP32=hip`` and
    ``MK_PATCH=hip``: what a kernel trace of the path should list -- ``x3_attn_*`` and ``toklinear_x3_*`` kernels and no vendor
    GEMM, convolution or attention kernel."""
    from makani_amd.vit import VisionTransformer
    os.environ[KNOB] = "hip"
    os.environ["MK_TOKEN_LINEAR_FP32"] = "hip"
    os.environ["MK_PATCH"] = "hip"
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    net = VisionTransformer(inp_shape=[112, 128], patch_size=(7, 8), inp_chans=8, out_chans=8, embed_dim=384, depth=2, num_heads=8).to(dev)
    x, tar = torch.randn(1, 8, 112, 128, device=dev), torch.randn(1, 8, 112, 128, device=dev)
    for _ in range(n):
        net.zero_grad(set_to_none=True)
        loss = ((net(x) - tar) ** 2).mean()
        loss.backward()
    torch.cuda.synchronize()
    print(f"attn_fp32_bench: {n} traced steps, loss {loss.item():.6f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-steps", type=int, default=0,
                    help="run only that many steps of a small fp32 ViT (for rocprofv3 --kernel-trace --stats) and exit")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attn_fp32_bench: no GPU found")
    if args.trace_steps:
        trace_steps(args.trace_steps)
        return
    from makani_amd import ops
    from makani_amd.vit import Attention, Block
    os.environ["MK_TOKEN_LINEAR_FP32"] = "hip"
    dev = torch.device("cuda:0")
    rows, kernels = [], []
    torch.manual_seed(1)

    def row(name, shape, call, leaves, g, runs_hip=True):
        def fwd():
            with torch.no_grad():
                return call()

        def fwd_bwd():
            return torch.autograd.grad(call(), leaves, g)

        hip_f, torch_f = with_knob(KNOB, "hip", fwd), with_knob(KNOB, "torch", fwd)
        hip_fb, torch_fb = with_knob(KNOB, "hip", fwd_bwd), with_knob(KNOB, "torch", fwd_bwd)
        err = rel(hip_f(), torch_f())          # a sanity bound before any timing; tests/ has the criterion
        gh, gt = hip_fb(), torch_fb()
        gerr = max(rel(a, b) for a, b in zip(gh, gt))
        assert err < 1e-4 and gerr < 1e-4, (name, shape, err, gerr)
        del gh, gt
        for label, fns in (("fwd", (hip_f, torch_f)), ("fwd+bwd", (hip_fb, torch_fb))):
            t_hip, t_torch = timed(fns, args.window, args.rounds)
            r = dict(module=name, shape=list(shape), what=label, hip_ms=round(t_hip * 1e3, 4), torch_ms=round(t_torch * 1e3, 4),
                     ratio=round(t_torch / t_hip, 3), out_err=err, grad_err=gerr, runs_hip=runs_hip)
            rows.append(r)
            print(f"{name:>28} {str(tuple(shape)):>20} {label:>7} {r['hip_ms']:>9.3f} {r['torch_ms']:>9.3f} {r['ratio']:>9.2f}"
                  + ("" if runs_hip else "   declined: the torch call on both sides"), flush=True)

    print(f"{'row':>28} {'shape':>20} {'pass':>7} {'hip ms':>9} {'torch ms':>9} {'torch/hip':>9}")
    for B, H, N, D in SHAPES:
        qkv = torch.randn(B, N, 3 * H * D, device=dev).requires_grad_(True)
        g = torch.randn(B, N, H * D, device=dev)
        taken = ops.attention_x3_supported(*ops._qkv_views(qkv.detach(), B, N, H, D))
        row("attention_packed", (B, H, N, D), lambda: ops.attention_packed(qkv, H), [qkv], g, taken)
        del qkv, g
        torch.cuda.empty_cache()
    B, N, C, heads = MODULE
    for name, mod in (("Attention", Attention(C, num_heads=heads, qkv_bias=True)), ("Block", Block(C, heads, mlp_ratio=4.0, qkv_bias=True))):
        mod = mod.to(dev)
        x = torch.randn(B, N, C, device=dev).requires_grad_(True)
        g = torch.randn(B, N, C, device=dev)
        row(f"vit {name} (x3 linears)", (B, N, C), lambda: mod(x), [x] + list(mod.parameters()), g)
        del mod, x, g
        torch.cuda.empty_cache()

    # the kernels alone
    for B, H, N, D in SHAPES:
        if D > ops.ATTN_X3_MAX_HEAD:
            continue
        qkv = torch.randn(B, N, 3 * H * D, device=dev)
        q, k, v = ops._qkv_views(qkv, B, N, H, D)
        o = torch.empty(B, N, H, D, device=dev).permute(0, 2, 1, 3)
        go = torch.randn(B, N, H, D, device=dev).permute(0, 2, 1, 3)
        lse, delta = torch.empty(B, H, N, device=dev), torch.empty(B, H, N, device=dev)
        dq, dk, dv = ops._qkv_views(torch.empty_like(qkv), B, N, H, D)
        scale = D ** -0.5
        ops.attn_x3_fwd_raw(q, k, v, o, lse, scale)
        lib, st, cs = ops._lib.load(), ops._attn_stride_array, ops._stream
        sizes = (B, H, N, N, D)

        def delta_k():
            s = st(o, go)
            lib.mk_attn_x3_bwd_delta(o.data_ptr(), go.data_ptr(), delta.data_ptr(), B, H, N, D, ctypes.addressof(s), cs())

        def dkv_k():
            s = st(q, k, v, go, dk, dv)
            lib.mk_attn_x3_bwd_dkv(q.data_ptr(), k.data_ptr(), v.data_ptr(), go.data_ptr(), lse.data_ptr(), delta.data_ptr(),
                                   dk.data_ptr(), dv.data_ptr(), *sizes, ctypes.addressof(s), scale, cs())

        def dq_k():
            s = st(q, k, v, go, dq)
            lib.mk_attn_x3_bwd_dq(q.data_ptr(), k.data_ptr(), v.data_ptr(), go.data_ptr(), lse.data_ptr(), delta.data_ptr(),
                                  dq.data_ptr(), *sizes, ctypes.addressof(s), scale, cs())

        unit = B * H * N * N * D
        runs = [("fwd", lambda: ops.attn_x3_fwd_raw(q, k, v, o, lse, scale), 4 * unit), ("bwd_delta", delta_k, 0),
                ("bwd_dkv", dkv_k, 6 * unit), ("bwd_dq", dq_k, 4 * unit)]
        delta_k()
        times = timed([c[1] for c in runs], args.window, args.rounds)
        for (what, _, fl), t in zip(runs, times):
            kr = dict(kernel=what, shape=[B, H, N, D], ms=round(t * 1e3, 4), TFLOPs=round(fl / t / 1e12, 1))
            kernels.append(kr)
            print(f"(B, H, N, D) = {(B, H, N, D)} mk_attn_x3_{what}: {kr['ms']:.4f} ms" + (f"  {kr['TFLOPs']:.1f} TFLOP/s" if fl else ""),
                  flush=True)
        tb = sum(t for (w, _, _), t in zip(runs, times) if w != "fwd")
        print(f"(B, H, N, D) = {(B, H, N, D)} backward, three kernels: {tb * 1e3:.4f} ms  {10 * unit / tb / 1e12:.1f} TFLOP/s", flush=True)
        del qkv, o, go, lse, delta, dq, dk, dv
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(dict(tool="attn_fp32_bench", window_s=args.window, rounds=args.rounds, rows=rows, kernels=kernels), fh, indent=1)
    losing = [r for r in rows if r["ratio"] < 1.0 and r["runs_hip"]]
    print(f"attn_fp32_bench: done, {len(losing)} of {sum(r['runs_hip'] for r in rows)} rows on the kernels slower than the torch path")
    for r in losing:
        print(f"  slower: {r['module']} {r['shape']} {r['what']} ({r['ratio']:.2f})")


if __name__ == "__main__":
    main()
