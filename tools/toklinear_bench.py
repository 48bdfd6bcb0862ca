#!/usr/bin/env python3
"""Times the token-major linears on one MI355X: the ``mk_token_linear_*`` kernels against ``F.linear`` (and ``F.gelu``, the residual
add) under bf16 autocast.

    python3 tools/toklinear_bench.py [--window 0.1] [--rounds 3] [--out FILE.json]
    rocprofv3 --kernel-trace --stats ... -- python3 tools/toklinear_bench.py --trace-steps 3

Rows, each forward and forward + backward (gradients of the input, the weight and the bias), bf16 rows and fp32 parameters:

* the four linears of a ViT block at R = 18 540 tokens -- ``vit_73ch`` (C = 384): 384 -> 1152 (qkv), 384 -> 384 (proj),
  384 -> 1536 with the GELU (fc1), 1536 -> 384 with the fp32 residual add (fc2); ``vit_73ch_big`` (C = 1024) likewise;
* the head 384 -> 4088;
* the same four linears at 2 x 4050 rows, C = 768;
* the traditional ``MLP`` and one ViT ``Block`` (fp32 tokens, mlp_ratio 4) at the first and the third shape.

* ``hip``: ``MK_TOKEN_LINEAR=hip``; ``torch``: ``MK_TOKEN_LINEAR=torch``, the vendor GEMM with torch's casts and pointwise passes.

The two paths are alternated in one process.  Each sample is a window of back-to-back calls between one pair of device events,
sized from a warm-up estimate to last at least ``--window`` seconds; per row the median over ``--rounds`` windows.  Before a row
is timed the two paths are compared on its inputs.

The kernels alone are printed against ``2 R I O`` flops and their algorithmic bytes (every operand read once, every result
written once).  It fails when no GPU is found.

The table of DESIGN section 26 is the output of ``python3 tools/toklinear_bench.py --window 0.1 --rounds 3``.
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

# (name, leading shape, C): the linears of a block follow from C
SHAPES = [("vit_73ch", (1, 18540), 384), ("vit_73ch_big", (1, 18540), 1024), ("2x4050", (2, 4050), 768)]
HEAD = ("head", (1, 18540), 384, 4088)


def block_linears(C):
    """(name, I, O, epilogue) of the four linears of a block of width C."""
    return [("qkv", C, 3 * C, "plain"), ("proj", C, C, "plain"), ("fc1", C, 4 * C, "gelu"), ("fc2", 4 * C, C, "addend")]


def trace_steps(n):
    """``n`` training steps (forward + backward, bf16 autocast) of a two-block ViT with ``MK_TOKEN_LINEAR=hip``: what a kernel trace
    of the path should list -- ``toklinear_*`` and ``attn_*`` kernels and no vendor GEMM apart from ``PatchEmbed``'s convolution."""
    from makani_amd.vit import VisionTransformer
    os.environ["MK_TOKEN_LINEAR"] = "hip"
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    net = VisionTransformer(inp_shape=[112, 128], patch_size=(7, 8), inp_chans=8, out_chans=8, embed_dim=384, depth=2, num_heads=8).to(dev)
    x, tar = torch.randn(1, 8, 112, 128, device=dev), torch.randn(1, 8, 112, 128, device=dev)
    for _ in range(n):
        net.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = ((net(x).float() - tar) ** 2).mean()
        loss.backward()
    torch.cuda.synchronize()
    print(f"toklinear_bench: {n} traced steps, loss {loss.item():.6f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-steps", type=int, default=0,
                    help="run only that many steps of a small ViT (for rocprofv3 --kernel-trace --stats) and exit")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("toklinear_bench: no GPU found")
    if args.trace_steps:
        trace_steps(args.trace_steps)
        return
    from makani_amd import layers, ops
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

        hip_f, torch_f = with_knob("MK_TOKEN_LINEAR", "hip", fwd), with_knob("MK_TOKEN_LINEAR", "torch", fwd)
        hip_fb, torch_fb = with_knob("MK_TOKEN_LINEAR", "hip", fwd_bwd), with_knob("MK_TOKEN_LINEAR", "torch", fwd_bwd)
        err = rel(hip_f(), torch_f())          # the same function on these inputs, before any timing (a sanity bound; tests/ has parity)
        gh, gt = hip_fb(), torch_fb()
        gerr = max(rel(a, b) for a, b in zip(gh, gt))
        assert err < 3e-2 and gerr < 3e-2, (name, shape, err, gerr)
        del gh, gt
        for label, fns in (("fwd", (hip_f, torch_f)), ("fwd+bwd", (hip_fb, torch_fb))):
            t_hip, t_torch = timed(fns, args.window, args.rounds)
            r = dict(module=name, shape=list(shape), what=label, hip_ms=round(t_hip * 1e3, 4), torch_ms=round(t_torch * 1e3, 4),
                     ratio=round(t_torch / t_hip, 3), out_err=err, grad_err=gerr)
            rows.append(r)
            print(f"{name:>22} {str(tuple(shape)):>20} {label:>7} {r['hip_ms']:>9.3f} {r['torch_ms']:>9.3f} {r['ratio']:>9.2f}", flush=True)

    def linear_row(tag, lead, I, O, kind):
        x = torch.randn(*lead, I, device=dev).bfloat16().requires_grad_(True)
        w = (torch.randn(O, I, device=dev) * I ** -0.5).requires_grad_(True)
        b = torch.randn(O, device=dev).mul_(0.1).requires_grad_(True)
        res = torch.randn(*lead, O, device=dev)
        g = torch.randn(*lead, O, device=dev)
        g = g if kind == "addend" else g.bfloat16()

        def call():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                if kind == "gelu":
                    return ops.token_linear(x, w, b, gelu=True)
                if kind == "addend":
                    return ops.token_linear(x, w, b, addend=res)
                return ops.token_linear(x, w, b)

        row(tag, lead + (I, O), call, [x], [w, b], g)

    print(f"{'row':>22} {'(rows..., I, O) / shape':>20} {'pass':>7} {'hip ms':>9} {'torch ms':>9} {'torch/hip':>9}")
    for name, lead, C in SHAPES[:2]:
        for lin, I, O, kind in block_linears(C):
            linear_row(f"{name} {lin}", lead, I, O, kind)
            torch.cuda.empty_cache()
    linear_row(HEAD[0], HEAD[1], HEAD[2], HEAD[3], "plain")
    name, lead, C = SHAPES[2]
    for lin, I, O, kind in block_linears(C):
        linear_row(f"{name} {lin}", lead, I, O, kind)
        torch.cuda.empty_cache()

    for name, lead, C in (SHAPES[0], SHAPES[2]):
        H = C // 48 if C == 384 else 12
        for tag, mod in (("MLP", layers.MLP(C, 4 * C, C, input_format="traditional")), ("Block", Block(C, H, mlp_ratio=4.0, qkv_bias=True))):
            mod = mod.to(dev)
            x = torch.randn(*lead, C, device=dev).requires_grad_(True)
            g = torch.randn(*lead, C, device=dev)

            def call():
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    return mod(x).float()

            row(f"{name} {tag}", lead + (C,), call, [x], list(mod.parameters()), g)
            del mod, x, g
            torch.cuda.empty_cache()

    # the kernels alone, against 2 R I O flops and their algorithmic bytes
    cases = [(n, lead, I, O) for n, lead, C in SHAPES for _, I, O, _ in block_linears(C)] + [HEAD]
    seen = set()
    for name, lead, I, O in cases:
        R = int(np.prod(lead))
        if (R, I, O) in seen:
            continue
        seen.add((R, I, O))
        x = torch.randn(R, I, device=dev).bfloat16()
        w = torch.randn(O, I, device=dev) * I ** -0.5
        b = torch.randn(O, device=dev)
        dy, aux = torch.randn(R, O, device=dev).bfloat16(), torch.randn(R, O, device=dev).bfloat16()
        res = torch.randn(R, O, device=dev)
        y, act, pre = (torch.empty(R, O, dtype=torch.bfloat16, device=dev) for _ in range(3))
        out = torch.empty(R, O, device=dev)
        dx = torch.empty(R, I, dtype=torch.bfloat16, device=dev)
        wimg = ops.token_linear_pack_raw(w)
        wt = ops.token_linear_pack_raw(wimg, transpose=True)
        gemm = 2 * (R * I + O * I + R * O)
        runs = [("pack fp32", lambda: ops.token_linear_pack_raw(w), 0, 6 * O * I),
                ("pack transposed", lambda: ops.token_linear_pack_raw(wimg, transpose=True), 0, 4 * O * I),
                ("fwd bias", lambda: ops.token_linear_fwd_raw(x, I, wimg, b, R, y=y), 2 * R * I * O, gemm),
                ("fwd bias gelu pre", lambda: ops.token_linear_fwd_raw(x, I, wimg, b, R, act=act, pre=pre), 2 * R * I * O, gemm + 2 * R * O),
                ("fwd bias addend", lambda: ops.token_linear_fwd_raw(x, I, wimg, b, R, addend=res, addend_ld=O, out_f32=out), 2 * R * I * O,
                 gemm + 6 * R * O),
                ("dgrad", lambda: ops.token_linear_fwd_raw(dy, O, wt, None, R, y=dx), 2 * R * I * O, gemm),
                ("dgrad gelu'", lambda: ops.token_linear_fwd_raw(x, I, wimg, None, R, y=y, aux=aux, aux_ld=O), 2 * R * I * O, gemm + 2 * R * O),
                ("wgrad + db", lambda: ops.token_linear_wgrad_raw(dy, O, x, I, R, O, I, True), 2 * R * I * O, 2 * R * (I + O) + 4 * O * I)]
        times = timed([c[1] for c in runs], args.window, args.rounds)
        slabs = ops._lib.load().mk_token_linear_wgrad_workspace(R, O, I, 0) // ((O * I + O) * 4) or 1
        for (what, _, fl, by), t in zip(runs, times):
            kr = dict(kernel=what, shape=[R, I, O], ms=round(t * 1e3, 4), TFLOPs=round(fl / t / 1e12, 1), TBs=round(by / t / 1e12, 2))
            if what.startswith("wgrad"):
                kr["slabs"] = int(slabs)
            kernels.append(kr)
            print(f"(R, I, O) = {(R, I, O)} {what}: {kr['ms']:.4f} ms  {kr['TFLOPs']:.1f} TFLOP/s  {kr['TBs']:.2f} TB/s (algorithmic)"
                  + (f"  slabs {slabs}" if what.startswith("wgrad") else ""), flush=True)
        del x, w, b, dy, aux, res, y, act, pre, out, dx, wimg, wt
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(dict(tool="toklinear_bench", window_s=args.window, rounds=args.rounds, rows=rows, kernels=kernels), fh, indent=1)
    losing = [r for r in rows if r["ratio"] < 1.0]
    print(f"toklinear_bench: done, {len(losing)} of {len(rows)} rows slower than the torch path")
    for r in losing:
        print(f"  slower: {r['module']} {r['what']} ({r['ratio']:.2f})")


if __name__ == "__main__":
    main()
