#!/usr/bin/env python3
"""Times the fp32 token-major linears on one MI355X: the ``mk_token_linear_x3_*`` kernels (the bf16x3 engine) against ``F.linear``
(and ``F.gelu``, the residual add) on fp32 rows WITHOUT autocast -- the vendor fp32 GEMM, which is what runs with the knob at
``torch``.  The fp32 sibling of tools/toklinear_bench.py.

    python3 tools/toklinear_fp32_bench.py [--window 0.1] [--rounds 3] [--out FILE.json]
    rocprofv3 --kernel-trace --stats ... -- python3 tools/toklinear_fp32_bench.py --trace-steps 3

Rows, each forward and forward + backward (gradients of the input, the weight and the bias), everything fp32:

* the four linears of a ViT block at 18 540 tokens, C = 384 (``vit_73ch``) and at 2 x 4050 tokens, C = 768: qkv, proj, fc1 with
  the GELU, fc2 with the residual add; and one ViT ``Block`` at both (attention stays ``F.scaled_dot_product_attention``);
* the AFNOv1 ``Mlp`` at 16 200 tokens, 768 -> 3072 -> 768, with the block's residual as addend;
* the head 384 -> 4088 at 18 540 tokens.

``hip``: ``MK_TOKEN_LINEAR_FP32=hip``; ``torch``: ``MK_TOKEN_LINEAR_FP32=torch``.  The two paths are alternated in one process, timed
as tools/event_timing.py does; before a row is timed the two paths are compared on its inputs.  Then every entry point alone
against ``2 R I O`` flops.  It fails when no GPU is found.

The table of DESIGN section 30 is the output of ``python3 tools/toklinear_fp32_bench.py --window 0.05 --rounds 3``.
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
from event_timing import rel, timed, with_knob  # noqa: E402

KNOB = "MK_TOKEN_LINEAR_FP32"
SHAPES = [("vit_73ch", (1, 18540), 384, 8), ("2x4050", (2, 4050), 768, 12)]        # name, leading shape, C, heads
HEAD = ("head", (1, 18540), 384, 4088)
AFNO_MLP = ("afnov1 Mlp", (1, 16200), 768, 3072)


def block_linears(C):
    return [("qkv", C, 3 * C, "plain"), ("proj", C, C, "plain"), ("fc1", C, 4 * C, "gelu"), ("fc2", 4 * C, C, "addend")]


def trace_steps(n):
    """``n`` fp32 training steps (no autocast) of a two-block ViT with ``MK_TOKEN_LINEAR_FP32=hip`` and ``MK_PATCH=hip``: what a kernel
    trace of the path should list -- ``toklinear_x3_*`` kernels and no vendor GEMM for a linear or the patch embedding (the
    attention products of ``F.scaled_dot_product_attention`` remain)."""
    from makani_amd.vit import VisionTransformer
    os.environ[KNOB] = "hip"
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
    print(f"toklinear_fp32_bench: {n} traced steps, loss {loss.item():.6f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-steps", type=int, default=0,
                    help="run only that many steps of a small fp32 ViT (for rocprofv3 --kernel-trace --stats) and exit")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("toklinear_fp32_bench: no GPU found")
    if args.trace_steps:
        trace_steps(args.trace_steps)
        return
    from makani_amd import afnonet_v1, ops
    from makani_amd.vit import Block
    dev = torch.device("cuda:0")
    rows, kernels = [], []
    torch.manual_seed(1)

    def row(name, shape, call, inputs, params, g):
        def fwd():
            with torch.no_grad():
                return call()

        def fwd_bwd():
            return torch.autograd.grad(call(), inputs + params, g)

        hip_f, torch_f = with_knob(KNOB, "hip", fwd), with_knob(KNOB, "torch", fwd)
        hip_fb, torch_fb = with_knob(KNOB, "hip", fwd_bwd), with_knob(KNOB, "torch", fwd_bwd)
        err = rel(hip_f(), torch_f())          # a sanity bound before any timing; tests/ has the criterion
        gh, gt = hip_fb(), torch_fb()
        gerr = max(rel(a, b) for a, b in zip(gh, gt))
        assert err < 1e-3 and gerr < 1e-3, (name, shape, err, gerr)
        del gh, gt
        for label, fns in (("fwd", (hip_f, torch_f)), ("fwd+bwd", (hip_fb, torch_fb))):
            t_hip, t_torch = timed(fns, args.window, args.rounds)
            r = dict(module=name, shape=list(shape), what=label, hip_ms=round(t_hip * 1e3, 4), torch_ms=round(t_torch * 1e3, 4),
                     ratio=round(t_torch / t_hip, 3), out_err=err, grad_err=gerr)
            rows.append(r)
            print(f"{name:>22} {str(tuple(shape)):>22} {label:>7} {r['hip_ms']:>9.3f} {r['torch_ms']:>9.3f} {r['ratio']:>9.2f}", flush=True)

    def linear_row(tag, lead, I, O, kind):
        x = torch.randn(*lead, I, device=dev).requires_grad_(True)
        w = (torch.randn(O, I, device=dev) * I ** -0.5).requires_grad_(True)
        b = torch.randn(O, device=dev).mul_(0.1).requires_grad_(True)
        res = torch.randn(*lead, O, device=dev)
        g = torch.randn(*lead, O, device=dev)

        def call():
            if kind == "gelu":
                return ops.token_linear(x, w, b, gelu=True)
            if kind == "addend":
                return ops.token_linear(x, w, b, addend=res)
            return ops.token_linear(x, w, b)

        row(tag, lead + (I, O), call, [x], [w, b], g)

    print(f"{'row':>22} {'(rows..., I, O) / shape':>22} {'pass':>7} {'hip ms':>9} {'torch ms':>9} {'torch/hip':>9}")
    for name, lead, C, heads in SHAPES:
        for lin, I, O, kind in block_linears(C):
            linear_row(f"{name} {lin}", lead, I, O, kind)
            torch.cuda.empty_cache()
        mod = Block(C, heads, mlp_ratio=4.0, qkv_bias=True).to(dev)
        x = torch.randn(*lead, C, device=dev).requires_grad_(True)
        g = torch.randn(*lead, C, device=dev)
        row(f"{name} Block", lead + (C,), lambda: mod(x), [x], list(mod.parameters()), g)
        del mod, x, g
        torch.cuda.empty_cache()
    name, lead, C, Hd = AFNO_MLP
    mod = afnonet_v1.Mlp(C, Hd).to(dev)
    x = torch.randn(*lead, C, device=dev).requires_grad_(True)
    res, g = torch.randn(*lead, C, device=dev), torch.randn(*lead, C, device=dev)
    row(name, lead + (C, Hd, C), lambda: mod(x, addend=res), [x], list(mod.parameters()), g)
    del mod, x, res, g
    torch.cuda.empty_cache()
    linear_row(HEAD[0], HEAD[1], HEAD[2], HEAD[3], "plain")
    torch.cuda.empty_cache()

    # the entry points alone, against 2 R I O flops
    cases = [(lead, I, O) for _, lead, C, _ in SHAPES for _, I, O, _ in block_linears(C)]
    cases += [(AFNO_MLP[1], AFNO_MLP[2], AFNO_MLP[3]), (AFNO_MLP[1], AFNO_MLP[3], AFNO_MLP[2]), HEAD[1:]]
    lib = ops._lib.load()
    for lead, I, O in cases:
        R = int(np.prod(lead))
        x, w, b = torch.randn(R, I, device=dev), torch.randn(O, I, device=dev) * I ** -0.5, torch.randn(O, device=dev)
        dy, aux, res = (torch.randn(R, O, device=dev) for _ in range(3))
        y, pre, dx = torch.empty(R, O, device=dev), torch.empty(R, O, device=dev), torch.empty(R, I, device=dev)
        fl = 2 * R * I * O
        runs = [("fwd bias", lambda: ops.token_linear_x3_fwd_raw(x, I, w, b, R, O, I, y=y)),
                ("fwd bias gelu pre", lambda: ops.token_linear_x3_fwd_raw(x, I, w, b, R, O, I, y=y, pre=pre, gelu=True)),
                ("fwd bias addend", lambda: ops.token_linear_x3_fwd_raw(x, I, w, b, R, O, I, y=y, addend=res, addend_ld=O)),
                ("dgrad (k-major w)", lambda: ops.token_linear_x3_fwd_raw(dy, O, w, None, R, I, O, kmajor=True, y=dx)),
                ("dgrad gelu'", lambda: ops.token_linear_x3_fwd_raw(x, I, w, None, R, O, I, y=y, aux=aux, aux_ld=O)),
                ("wgrad", lambda: ops.token_linear_x3_wgrad_raw(dy, O, x, I, R, O, I, False)),
                ("wgrad + db", lambda: ops.token_linear_x3_wgrad_raw(dy, O, x, I, R, O, I, True)),
                ("torch F.linear", lambda: torch.nn.functional.linear(x, w, b))]
        times = timed([c[1] for c in runs], args.window, args.rounds)
        slabs = max(1, (lib.mk_token_linear_x3_wgrad_workspace(R, O, I, 0) - (R + 127) // 128 * O * 8) // (O * I * 4))
        for (what, _), t in zip(runs, times):
            kr = dict(kernel=what, shape=[R, I, O], ms=round(t * 1e3, 4), TFLOPs=round(fl / t / 1e12, 1))
            if what.startswith("wgrad"):
                kr["slabs"] = int(slabs)
            kernels.append(kr)
            print(f"(R, I, O) = {(R, I, O)} {what}: {kr['ms']:.4f} ms  {kr['TFLOPs']:.1f} TFLOP/s"
                  + (f"  slabs {slabs}" if what.startswith("wgrad") else ""), flush=True)
        del x, w, b, dy, aux, res, y, pre, dx
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(dict(tool="toklinear_fp32_bench", window_s=args.window, rounds=args.rounds, rows=rows, kernels=kernels), fh, indent=1)
    losing = [r for r in rows if r["ratio"] < 1.0]
    print(f"toklinear_fp32_bench: done, {len(losing)} of {len(rows)} rows slower than the torch path")
    for r in losing:
        print(f"  slower: {r['module']} {r['what']} ({r['ratio']:.2f})")


if __name__ == "__main__":
    main()
