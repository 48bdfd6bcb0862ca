#!/usr/bin/env python3
"""Times the trailing-axis layer norm on one MI355X: the ``mk_token_layernorm_*`` kernels against the torch formulation.

    python3 tools/toknorm_bench.py [--window 0.5] [--rounds 5] [--out FILE.json]

The op alone (``ops.token_layer_norm`` against ``F.layer_norm`` with the add and the cast around it as separate torch ops, which
is what a ViT block does under bf16 autocast), forward and forward + backward, at (rows, L) = (18 540, 384) -- the tokens of
``config/vit.yaml`` -- and (8 100, 768):

* ``fused``: fp32 tokens + bf16 residual -> fp32 result and its bf16 copy, both with a gradient (``norm2`` of a block);
* ``bf16``: bf16 tokens + bf16 residual -> bf16 (torch's layer norm takes bf16 parameters here, the kernels fp32 ones);
* ``plain``: fp32 -> fp32, no residual (the final norm);

the AFNO norm ``LayerNorm((90, 180))`` on NCHW fields of 768 and 1 536 rows of 16 200 elements, fp32 and bf16; and one ViT
``Block`` (384 wide, 8 heads, mlp_ratio 4) at 18 540 tokens under bf16 autocast with ``MK_TOKEN_NORM=hip`` against ``torch``.

The two paths are alternated in one process.  Each sample is a window of back-to-back calls between one pair of device events,
sized from a warm-up estimate to last at least ``--window`` seconds; per row the median over ``--rounds`` windows.  Before a row
is timed the two paths are compared on its inputs.

The kernels alone are printed against their algorithmic bytes: every input read once and every output written once (the
backward's workspace traffic and its finishing launch are in the time, not in the bytes).  These are the same event windows
around back-to-back calls of the C ABI on preallocated buffers, not a kernel trace: they hold the launch gaps, and at these
sizes the operands stay in the Infinity Cache between calls.  It fails when no GPU is found.

The table of DESIGN section 25 is the output of ``python3 tools/toknorm_bench.py --window 0.5 --rounds 5``.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from event_timing import rel, timed  # noqa: E402

TOKEN_SHAPES = [(18540, 384), (8100, 768)]
AFNO_SHAPES = [(768, 90, 180), (1536, 90, 180)]
F32, BF16 = torch.float32, torch.bfloat16
EPS = 1e-6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("toknorm_bench: no GPU found")
    from makani_amd import ops
    from makani_amd.vit import Block
    dev = torch.device("cuda:0")
    rows, kernels = [], []
    torch.manual_seed(1)

    def row(name, shape, hip, ref, leaves, grads, ref_leaves=None):
        """``hip`` / ``ref``: callables that return the tuple of results; ``grads``: one cotangent per result; ``ref_leaves``: what
        the torch path differentiates with respect to where that is not ``leaves`` (bf16 copies of the parameters)."""
        def fwd(call):
            def run():
                with torch.no_grad():
                    return call()
            return run

        def fwd_bwd(call):
            wrt = ref_leaves if (call is ref and ref_leaves is not None) else leaves
            return lambda: torch.autograd.grad(call(), wrt, grads)

        err = max(rel(a, b) for a, b in zip(fwd(hip)(), fwd(ref)()))      # a sanity bound before any timing; tests/ has parity
        gerr = max(rel(a, b) for a, b in zip(fwd_bwd(hip)(), fwd_bwd(ref)()))
        assert err < 2e-2 and gerr < 2e-2, (name, shape, err, gerr)
        for label, fns in (("fwd", (fwd(hip), fwd(ref))), ("fwd+bwd", (fwd_bwd(hip), fwd_bwd(ref)))):
            t_hip, t_torch = timed(fns, args.window, args.rounds)
            r = dict(case=name, shape=list(shape), what=label, hip_ms=round(t_hip * 1e3, 4), torch_ms=round(t_torch * 1e3, 4),
                     ratio=round(t_torch / t_hip, 3), out_err=err, grad_err=gerr)
            rows.append(r)
            print(f"{name:>10} {str(tuple(shape)):>18} {label:>7} {r['hip_ms']:>9.4f} {r['torch_ms']:>9.4f} {r['ratio']:>9.2f}", flush=True)

    print(f"{'case':>10} {'shape':>18} {'pass':>7} {'hip ms':>9} {'torch ms':>9} {'torch/hip':>9}")
    for n, L in TOKEN_SHAPES:
        w = (1.0 + 0.1 * torch.randn(L, device=dev)).requires_grad_(True)
        b = (0.1 * torch.randn(L, device=dev)).requires_grad_(True)
        x = torch.randn(n, L, device=dev).requires_grad_(True)
        xb = torch.randn(n, L, device=dev).bfloat16().requires_grad_(True)
        r = torch.randn(n, L, device=dev).bfloat16().requires_grad_(True)
        g, gb = torch.randn(n, L, device=dev), torch.randn(n, L, device=dev).bfloat16()

        def ref_fused():
            y = F.layer_norm(x + r, (L,), w, b, EPS)
            return y, y.to(BF16)

        row("fused", (n, L), lambda: ops.token_layer_norm(x, w, b, EPS, r, F32, True), ref_fused, [x, r, w, b], [g, gb])
        # torch's layer norm wants the parameters in the input's dtype: a bf16 module, which this package's kernels do not ask for
        wl, bl = (p.detach().bfloat16().requires_grad_(True) for p in (w, b))
        row("bf16", (n, L), lambda: (ops.token_layer_norm(xb, w, b, EPS, r),), lambda: (F.layer_norm(xb + r, (L,), wl, bl, EPS),),
            [xb, r, w, b], [gb], [xb, r, wl, bl])
        row("plain", (n, L), lambda: (ops.token_layer_norm(x, w, b, EPS),), lambda: (F.layer_norm(x, (L,), w, b, EPS),), [x, w, b], [g])
        del x, xb, r, g, gb
        torch.cuda.empty_cache()
    for n, h, wd in AFNO_SHAPES:
        w = (1.0 + 0.1 * torch.randn(h, wd, device=dev)).requires_grad_(True)
        b = (0.1 * torch.randn(h, wd, device=dev)).requires_grad_(True)
        for dt, tag in ((F32, "afno fp32"), (BF16, "afno bf16")):
            x = torch.randn(1, n, h, wd, device=dev).to(dt).requires_grad_(True)
            g = torch.randn(1, n, h, wd, device=dev).to(dt)
            wl, bl = (p.detach().to(dt).requires_grad_(True) for p in (w, b))
            row(tag, (n, h * wd), lambda: (ops.token_layer_norm(x, w, b, EPS),), lambda: (F.layer_norm(x, (h, wd), wl, bl, EPS),), [x, w, b], [g],
                [x, wl, bl])
            del x, g
            torch.cuda.empty_cache()
    # one ViT block under bf16 autocast
    n, L = TOKEN_SHAPES[0]
    blk = Block(L, 8, mlp_ratio=4.0, qkv_bias=True).to(dev)
    with torch.no_grad():
        blk.attn.qkv.weight.mul_(4.0)             # scores of order 1
    x = torch.randn(1, n, L, device=dev).requires_grad_(True)
    g = torch.randn(1, n, L, device=dev)

    def block(value):
        def call():
            os.environ["MK_TOKEN_NORM"] = value        # read at call time
            with torch.autocast("cuda", dtype=BF16):
                return (blk(x).float(),)
        return call

    row("Block", (n, L), block("hip"), block("torch"), [x] + list(blk.parameters()), [g])
    os.environ.pop("MK_TOKEN_NORM", None)
    del blk, x, g
    torch.cuda.empty_cache()
    # the kernels alone, against their algorithmic bytes: the same windows around back-to-back calls of the C ABI
    lib, t3 = ops._lib.load(), ops._tok3
    size = {F32: 4, BF16: 2}
    for (n, L), x_dt, r_dt, y_dt, lowp, tag in [(s, *c) for s in TOKEN_SHAPES for c in ((F32, BF16, F32, True, "fused"), (BF16, BF16, BF16, False, "bf16"),
                                                                                    (F32, None, F32, False, "plain"))] + \
                                              [((s[0], s[1] * s[2]), dt, None, dt, False, "afno") for s in AFNO_SHAPES for dt in (F32, BF16)]:
        x = torch.randn(n, L, device=dev).to(x_dt)
        r = None if r_dt is None else torch.randn(n, L, device=dev).to(r_dt)
        w, b = torch.randn(L, device=dev), torch.randn(L, device=dev)
        y, y2 = torch.empty(n, L, device=dev, dtype=y_dt), (torch.empty(n, L, device=dev, dtype=BF16) if lowp else None)
        gy, gy2 = torch.randn(n, L, device=dev).to(y_dt), (torch.randn(n, L, device=dev).bfloat16() if lowp else None)
        stats = torch.empty(n, 2, device=dev)
        gx, gr = torch.empty_like(x), (None if r is None else torch.empty_like(r))
        gwb = torch.empty(2, L, device=dev)
        ws = torch.empty(lib.mk_token_layernorm_workspace(n, L), device=dev)      # once, not per call as the op does
        bytes_f = n * L * (size[x_dt] + (size[r_dt] if r_dt else 0) + size[y_dt] + (2 if lowp else 0))
        bytes_b = n * L * (2 * size[x_dt] + (2 * size[r_dt] if r_dt else 0) + size[y_dt] + (2 if lowp else 0))
        cases = [("mk_token_layernorm_fwd", lambda: ops.token_layernorm_fwd_raw(x, L, r, L, w, b, y, y2, None, stats, n, L, EPS), bytes_f),
                 ("mk_token_layernorm_bwd", lambda: lib.mk_token_layernorm_bwd(*t3(x, L), *t3(r, L), *t3(gy, L), ops._ptr(gy2), L, None, 0, 0,
                                                                               stats.data_ptr(), w.data_ptr(), gx.data_ptr(), ops._ptr(gr),
                                                                               ws.data_ptr(), gwb.data_ptr(), n, L, ops._stream()), bytes_b)]
        times = timed([c[1] for c in cases], args.window, args.rounds)
        for (what, _, nbytes), t in zip(cases, times):
            kr = dict(kernel=what, case=tag, shape=[n, L], x=str(x_dt), ms=round(t * 1e3, 4), bytes=nbytes, TBps=round(nbytes / t / 1e12, 2))
            kernels.append(kr)
            print(f"{tag:>6} {str((n, L)):>14} {str(x_dt):>15} {what}: {kr['ms']:.4f} ms  {kr['TBps']:.2f} TB/s (algorithmic bytes)", flush=True)
        del x, r, y, y2, gy, gy2, gx, gr
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(dict(tool="toknorm_bench", window_s=args.window, rounds=args.rounds, rows=rows, kernels=kernels), fh, indent=1)
    losing = [r for r in rows if r["ratio"] < 1.0]
    print(f"toknorm_bench: done, {len(losing)} of {len(rows)} rows slower than the torch path")
    for r in losing:
        print(f"  slower: {r['case']} {tuple(r['shape'])} {r['what']}: torch/hip {r['ratio']:.2f}")


if __name__ == "__main__":
    main()
