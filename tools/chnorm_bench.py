#!/usr/bin/env python3
"""Times the channel layer norm (csrc/chnorm.hip) on one MI355X against the torch formulation it replaces.

    python3 tools/chnorm_bench.py [--window 0.5] [--rounds 3] [--shapes full,low] [--out FILE.json]

Fields ``[1, 384, 721, 1440]`` (full resolution) and ``[1, 384, 240, 480]`` (the model grid), bf16 and fp32, plain and
GELU-fused, forward alone and forward + backward:

* ``hip``: ``DistributedLayerNorm.forward`` on the HIP path (``ops.channel_layer_norm``);
* ``torch``: ``DistributedLayerNorm._forward_torch`` (transpose -> ``nn.LayerNorm`` -> transpose, contiguous) followed by
  ``F.gelu`` when fused -- the formulation of the parent commit -- in the same process on the same inputs.

The two are alternated.  Each sample is a window of back-to-back calls between one pair of device events, sized from a
warm-up estimate to last at least ``--window`` seconds; per row the median over ``--rounds`` windows.  ``GB/s`` is the
algorithmic traffic over the time: one read and one write of the field forward, and one read each of the field and of
``gy`` plus one write backward (statistics and parameters are below 1 %).  Before a row is timed the two paths are compared
on its inputs.  It fails when no GPU is found.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"full": (1, 384, 721, 1440), "low": (1, 384, 240, 480)}


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
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        est = window(f, 3)
        calls.append(max(3, int(np.ceil(1.1 * seconds / est))))
    out = [[] for _ in fns]
    for _ in range(rounds):
        for f, n, ts in zip(fns, calls, out):
            ts.append(window(f, n))
    return [float(np.median(ts)) for ts in out], calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="full,low")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("chnorm_bench: no GPU found")
    from makani_amd import ops
    from makani_amd.layer_norm import DistributedLayerNorm
    dev = torch.device("cuda:0")
    rows = []
    print(f"{'shape':>18} {'dtype':>5} {'gelu':>4} {'pass':>7} {'hip ms':>9} {'hip GB/s':>9} {'torch ms':>9} {'torch GB/s':>10} {'ratio':>6}")
    for name in args.shapes.split(","):
        shape = SHAPES[name]
        C = shape[1]
        for dtype in (torch.bfloat16, torch.float32):
            torch.manual_seed(1)
            m = DistributedLayerNorm(C, eps=1e-6).to(dev)
            with torch.no_grad():
                m.norm.weight.normal_()
                m.norm.bias.normal_()
            if dtype == torch.bfloat16:      # the torch formulation needs parameters of the field's dtype outside autocast
                mt = DistributedLayerNorm(C, eps=1e-6).to(dev).to(dtype)
                mt.load_state_dict(m.state_dict())
            else:
                mt = m
            x = (torch.randn(shape, device=dev) * 3 + 5).to(dtype).requires_grad_(True)
            gy = torch.randn(shape, device=dev).to(dtype)
            assert ops.channel_layer_norm_supported(x)
            field = x.numel() * x.element_size()
            for fuse in (False, True):
                def hip_f():
                    with torch.no_grad():
                        return m(x, fuse_gelu=fuse)

                def torch_f():
                    with torch.no_grad():
                        y = mt._forward_torch(x)
                        return F.gelu(y) if fuse else y

                def hip_fb():
                    y = m(x, fuse_gelu=fuse)
                    return torch.autograd.grad(y, (x, m.norm.weight, m.norm.bias), gy)

                def torch_fb():
                    y = mt._forward_torch(x)
                    if fuse:
                        y = F.gelu(y)
                    return torch.autograd.grad(y, (x, mt.norm.weight, mt.norm.bias), gy)

                # same function on these inputs, before any timing
                ya, yb = hip_f().float(), torch_f().float()
                err = (torch.linalg.norm(ya - yb) / torch.linalg.norm(yb)).item()
                ga, gb = hip_fb()[0].float(), torch_fb()[0].float()
                gerr = (torch.linalg.norm(ga - gb) / torch.linalg.norm(gb)).item()
                tol = 1e-4 if dtype == torch.float32 else 3e-2
                assert err < tol and gerr < tol, (err, gerr)
                del ya, yb, ga, gb
                for label, fns, nbytes in (("fwd", (hip_f, torch_f), 2 * field), ("fwd+bwd", (hip_fb, torch_fb), 5 * field)):
                    (t_hip, t_torch), calls = timed(fns, args.window, args.rounds)
                    r = dict(shape=list(shape), dtype=str(dtype).split(".")[-1], gelu=fuse, what=label, bytes=nbytes,
                             hip_ms=round(t_hip * 1e3, 4), torch_ms=round(t_torch * 1e3, 4),
                             hip_GBs=round(nbytes / t_hip / 1e9, 1), torch_GBs=round(nbytes / t_torch / 1e9, 1),
                             ratio=round(t_torch / t_hip, 2), calls_per_window=calls, y_err=err, gx_err=gerr)
                    rows.append(r)
                    print(f"{'x'.join(map(str, shape)):>18} {r['dtype'][:5]:>5} {int(fuse):>4} {label:>7} {r['hip_ms']:>9.3f} "
                          f"{r['hip_GBs']:>9.1f} {r['torch_ms']:>9.3f} {r['torch_GBs']:>10.1f} {r['ratio']:>6.2f}", flush=True)
            del x, gy
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(tool="chnorm_bench", window_s=args.window, rounds=args.rounds, rows=rows), f, indent=1)
    print("chnorm_bench: done")


if __name__ == "__main__":
    main()
