#!/usr/bin/env python3
"""Times patch embedding and the un-patchify of the patch networks on one MI355X: ``MK_PATCH=hip`` (``mk_patchify`` /
``mk_unpatchify`` around the ``mk_token_linear_*`` GEMM) against ``MK_PATCH=torch`` (``nn.Conv2d`` and torch's permuted copies)
under bf16 autocast.

    python3 tools/patch_bench.py [--window 0.1] [--rounds 3] [--part embed,embed-dx,unpatchify,kernels] [--only NAME] [--out FILE.json]
    rocprofv3 --kernel-trace --stats ... -- python3 tools/patch_bench.py --trace-steps 3

Rows, each forward and forward + backward (fp32 images and parameters):

* ``PatchEmbed.forward_tokens(x, pos_embed)`` at 73 x 721 x 1440 with 7 x 8 patches -> 384 (``vit_73ch``) and -> 1024
  (``vit_73ch_big``), and at 26 and 73 x 720 x 1440 with 8 x 8 patches -> 768 (AFNOv1) for B = 1 and 2; gradients of the
  parameters and the position embedding;
* the same rows with the image requiring a gradient (what multi-step training asks for);
* the head's un-patchify alone at the same grids: bf16 rows -> bf16 image, and with backward the fp32 gradient -> bf16 rows.

The two paths are alternated in one process.  Each sample is a window of back-to-back calls between one pair of device events,
sized from a warm-up estimate to last at least ``--window`` seconds; per row the median over ``--rounds`` windows.  Before a row
is timed the two paths are compared on its inputs.

The two kernels alone are printed against their algorithmic bytes (each element read once and written once).  It fails when no
GPU is found.  ``--part`` selects groups of rows (MIOpen searches its solvers at the first call of every convolution shape, which
takes most of the wall time of the embedding rows), ``--only`` the shapes whose name contains it.

The tables of DESIGN section 29 are the output of ``python3 tools/patch_bench.py --window 0.1 --rounds 3``.
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

# (name, B, C, H, W, patch, E)
EMBED = [("vit_73ch", 1, 73, 721, 1440, (7, 8), 384), ("vit_73ch_big", 1, 73, 721, 1440, (7, 8), 1024),
         ("afnov1_26ch", 1, 26, 720, 1440, (8, 8), 768), ("afnov1_26ch", 2, 26, 720, 1440, (8, 8), 768),
         ("afnov1_73ch", 1, 73, 720, 1440, (8, 8), 768), ("afnov1_73ch", 2, 73, 720, 1440, (8, 8), 768)]


def trace_steps(n):
    """``n`` training steps (forward + backward, bf16 autocast) of a two-block ViT with ``MK_PATCH=hip`` and ``MK_TOKEN_LINEAR=hip``:
    what a kernel trace of the path should list -- ``patch_kernel``, ``toklinear_*`` and ``attn_*`` and no vendor convolution."""
    from makani_amd.vit import VisionTransformer
    os.environ["MK_PATCH"] = "hip"
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
    print(f"patch_bench: {n} traced steps, loss {loss.item():.6f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--part", default="embed,embed-dx,unpatchify,kernels", help="comma-separated groups of rows to run")
    ap.add_argument("--only", default="", help="run only the shapes whose name contains this (vit_73ch, afnov1_26ch, ...)")
    ap.add_argument("--trace-steps", type=int, default=0,
                    help="run only that many steps of a small ViT (for rocprofv3 --kernel-trace --stats) and exit")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("patch_bench: no GPU found")
    if args.trace_steps:
        trace_steps(args.trace_steps)
        return
    parts = set(args.part.split(","))
    assert parts <= {"embed", "embed-dx", "unpatchify", "kernels"}, args.part
    from makani_amd import layers, ops
    global EMBED
    EMBED = [e for e in EMBED if args.only in e[0]]
    dev = torch.device("cuda:0")
    rows, kernels = [], []
    torch.manual_seed(1)

    def row(name, shape, call, wrt, g):
        def fwd():
            with torch.no_grad():
                return call()

        def fwd_bwd():
            return torch.autograd.grad(call(), wrt, g)

        hip_f, torch_f = with_knob("MK_PATCH", "hip", fwd), with_knob("MK_PATCH", "torch", fwd)
        hip_fb, torch_fb = with_knob("MK_PATCH", "hip", fwd_bwd), with_knob("MK_PATCH", "torch", fwd_bwd)
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
            print(f"{name:>26} {str(tuple(shape)):>30} {label:>7} {r['hip_ms']:>9.3f} {r['torch_ms']:>9.3f} {r['ratio']:>9.2f}", flush=True)

    print(f"{'row':>26} {'(B, C, H, W, p0, p1, E)':>30} {'pass':>7} {'hip ms':>9} {'torch ms':>9} {'torch/hip':>9}")
    for image_grad in (False, True):
        for name, B, C, H, W, patch, E in EMBED if ("embed-dx" if image_grad else "embed") in parts else []:
            pe = layers.PatchEmbed(img_size=(H, W), patch_size=patch, in_chans=C, embed_dim=E).to(dev)
            pos = (0.02 * torch.randn(1, pe.num_patches, E, device=dev)).requires_grad_(True)
            x = torch.randn(B, C, H, W, device=dev).requires_grad_(image_grad)
            g = torch.randn(B, pe.num_patches, E, device=dev)

            def call():
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    return pe.forward_tokens(x, pos)

            row(f"{name} embed" + (" dx" if image_grad else ""), (B, C, H, W) + patch + (E,), call,
                ([x] if image_grad else []) + list(pe.parameters()) + [pos], g)
            del pe, pos, x, g
            torch.cuda.empty_cache()

    seen = set()
    for name, B, C, H, W, patch, _ in EMBED if "unpatchify" in parts else []:
        if (B, C, H, W, patch) in seen:
            continue
        seen.add((B, C, H, W, patch))
        hp, wp = H // patch[0], W // patch[1]
        t = torch.randn(B, hp, wp, C * patch[0] * patch[1], device=dev).bfloat16().requires_grad_(True)
        g = torch.randn(B, C, H, W, device=dev)

        def call():
            return ops.unpatchify(t, patch, C, (H, W), order=1)

        row(f"{name.split('_')[0]} un-patchify", (B, C, H, W) + patch, call, [t], g)
        del t, g
        torch.cuda.empty_cache()

    # the kernels alone, against their algorithmic bytes
    seen = set()
    for name, B, C, H, W, patch, _ in EMBED if "kernels" in parts else []:
        if (B, C, H, W, patch) in seen:
            continue
        seen.add((B, C, H, W, patch))
        R, F = B * (H // patch[0]) * (W // patch[1]), C * patch[0] * patch[1]
        n = B * C * H * W
        x32, x16 = torch.randn(B, C, H, W, device=dev), torch.randn(B, C, H, W, device=dev).bfloat16()
        t16 = torch.randn(R, F, device=dev).bfloat16()
        o16, i16, i32 = torch.empty_like(t16), torch.empty_like(x16), torch.empty_like(x32)
        runs = [("patchify order 0 fp32 -> bf16", lambda: ops.patchify_raw(x32, o16, patch, 0), 6 * n),
                ("patchify order 0 bf16 -> bf16", lambda: ops.patchify_raw(x16, o16, patch, 0), 4 * n),
                ("unpatchify order 0 bf16 -> fp32", lambda: ops.unpatchify_raw(t16, i32, patch, 0), 6 * n),
                ("unpatchify order 1 bf16 -> bf16", lambda: ops.unpatchify_raw(t16, i16, patch, 1), 4 * n),
                ("patchify order 1 fp32 -> bf16", lambda: ops.patchify_raw(x32, o16, patch, 1), 6 * n)]
        times = timed([c[1] for c in runs], args.window, args.rounds)
        for (what, _, by), t in zip(runs, times):
            kr = dict(kernel=what, shape=[B, C, H, W, *patch], ms=round(t * 1e3, 4), TBs=round(by / t / 1e12, 2))
            kernels.append(kr)
            print(f"(B, C, H, W, p0, p1) = {(B, C, H, W) + patch} {what}: {kr['ms']:.4f} ms  {kr['TBs']:.2f} TB/s (algorithmic)", flush=True)
        del x32, x16, t16, o16, i16, i32
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(dict(tool="patch_bench", window_s=args.window, rounds=args.rounds, rows=rows, kernels=kernels), fh, indent=1)
    losing = [r for r in rows if r["ratio"] < 1.0]
    print(f"patch_bench: done, {len(losing)} of {len(rows)} rows slower than the torch path")
    for r in losing:
        print(f"  slower: {r['module']} {r['shape']} {r['what']} ({r['ratio']:.2f})")


if __name__ == "__main__":
    main()
