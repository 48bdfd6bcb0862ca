#!/usr/bin/env python3
"""Times the grid conversion (csrc/grid.hip through ``makani_amd.grids.GridConverter``) on one MI355X.

    python3 tools/grid_bench.py [--window 0.1] [--rounds 3] [--part module,kernel] [--out FILE.json]

At 73 x 721 x 1440, B = 1 and 2, an fp32 batch on an equiangular grid onto the Legendre-Gauss latitudes:

* ``GridConverter.forward`` to fp32 and to bf16, with and without the loader's ``(x - bias) / scale``, forward alone and forward +
  backward: ``MK_GRID=hip`` against ``MK_GRID=torch`` (the same call on the same tensors, alternated in one process);
* the two kernels alone (preallocated output, no autograd) against their algorithmic bytes in TB/s: the source once and the
  destination once.

Each sample is a window of back-to-back calls between one pair of device events, sized from a warm-up estimate to last at
least ``--window`` seconds; per row the median over ``--rounds`` windows (``event_timing.py``).  Before a row is timed the two
paths must agree on its inputs within twice the per-element bounds of DESIGN section 40 (forward ``3 u (|a'| + |b'|)``,
backward ``(t + 3) u sum |c_t gy_t| / |scale|``, plus a bf16 ulp where the result is bf16, plus ``u |w gy| / |scale|`` per a-term for
torch's ``fl(1 - fl(w))`` in its lerp backward).  It fails when no GPU is found.  The
default of ``MK_GRID`` follows DESIGN section 19: ``hip`` only if no row here is slower than the torch path; the table of DESIGN
section 40 is this tool's output.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from event_timing import timed, window, with_knob  # noqa: E402

C, H, W = 73, 721, 1440
U = 2.0 ** -24


def bf16_ulp(v):
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(1e-30))) - 7)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--part", default="module,kernel", help="comma-separated groups of rows to run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("grid_bench: no GPU found")
    parts = set(args.part.split(","))
    assert parts <= {"module", "kernel"}, args.part
    from makani_amd import _lib, ops
    from makani_amd.grids import GridConverter
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    lat = torch.deg2rad(torch.linspace(90.0, -90.0, H)).to(dev)
    lon = torch.deg2rad(torch.linspace(0.0, 360.0, W + 1)[:-1]).to(dev)
    conv = GridConverter("equiangular", "legendre-gauss", lat, lon)
    tables = conv.tables(dev)
    idx = conv.indices
    terms = torch.bincount(torch.cat([idx, idx + 1]), minlength=H).view(1, 1, H, 1).double()
    scale = 1.0 + 9.0 * torch.rand(C, device=dev, generator=g)
    bias = 100.0 * torch.randn(C, device=dev, generator=g)
    rows, kernels = [], []
    print(f"{'row':>44} {'B':>2} {'hip ms':>10} {'torch ms':>10} {'torch/hip':>9}")
    for B in (1, 2):
        x = (torch.randn(B, C, H, W, device=dev, generator=g) * scale.view(1, C, 1, 1) + bias.view(1, C, 1, 1)).requires_grad_(True)
        for out_dtype in (torch.float32, torch.bfloat16):
            gy = torch.randn(B, C, H, W, device=dev, generator=g).to(out_dtype)
            for norm in (False, True):
                kw = dict(bias=bias, scale=scale) if norm else {}
                tag = f"fp32 -> {'fp32' if out_dtype == torch.float32 else 'bf16'}{', normalised' if norm else ''}"

                def fwd():
                    with torch.no_grad():
                        return conv(x, out_dtype=out_dtype, **kw)

                def both():
                    x.grad = None
                    conv(x, out_dtype=out_dtype, **kw).backward(gy)
                    return x.grad

                # ---- the two paths on these inputs, within twice the bounds
                with torch.no_grad():
                    xn = (x - bias.view(1, C, 1, 1)) / scale.view(1, C, 1, 1) if norm else x
                    fbound = 3.0 * U * (xn[..., idx, :].abs() + xn[..., idx + 1, :].abs())
                    del xn
                    y = {m: with_knob("MK_GRID", m, fwd)().float() for m in ("hip", "torch")}
                    slack = 2.0 * fbound + (bf16_ulp(y["torch"]) if out_dtype == torch.bfloat16 else 0.0)
                    assert bool(((y["hip"] - y["torch"]).abs() <= slack).all()), f"forward paths disagree: {tag} B={B}"
                    del y, fbound, slack
                gx = {m: with_knob("MK_GRID", m, both)().clone() for m in ("hip", "torch")}
                x.grad = None
                with with_env("MK_GRID", "torch"):
                    conv(x, **kw).backward(gy.abs().float())            # the weights lie in [0, 1]: sum |c_t gy_t| / |scale|
                mag, x.grad = x.grad.double(), None
                # torch's lerp backward multiplies by fl(1 - fl(w)): the rounding of w enters the a-term as u |w gy|, which is
                # not relative to 1 - w (the kernel's coefficient is 1 - w rounded once from float64): allowed on top
                extra = torch.zeros_like(mag).index_add_(-2, idx, (gy.abs().double() * conv.interp_weights.abs()))
                if norm:
                    extra /= scale.view(1, C, 1, 1).abs().double()
                tol = 2.0 * ((terms + 3.0) * U * mag + U * extra)
                assert bool(((gx["hip"] - gx["torch"]).abs().double() <= tol).all()), f"backward paths disagree: {tag} B={B}"
                del gx, mag, extra, tol
                torch.cuda.empty_cache()
                if "module" in parts:
                    for name, fn in ((f"forward, {tag}", fwd), (f"forward + backward, {tag}", both)):
                        t_hip, t_torch = timed([with_knob("MK_GRID", "hip", fn), with_knob("MK_GRID", "torch", fn)], args.window, args.rounds)
                        r = dict(row=name, B=B, hip_ms=round(t_hip * 1e3, 4), torch_ms=round(t_torch * 1e3, 4), ratio=round(t_torch / t_hip, 3))
                        rows.append(r)
                        print(f"{name:>44} {B:>2} {r['hip_ms']:>10.3f} {r['torch_ms']:>10.3f} {r['ratio']:>9.2f}", flush=True)
                    x.grad = None
                if "kernel" in parts:
                    xd = x.detach()
                    y = torch.empty(B, C, H, W, dtype=out_dtype, device=dev)
                    gxb = torch.empty(B, C, H, W, device=dev)
                    b32, s32 = (bias, scale) if norm else (None, None)
                    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
                    code = 0 if out_dtype == torch.float32 else 1

                    def kf():
                        ops._lat_lerp_fwd_raw(xd, tables, b32, s32, y)

                    def kb():
                        _lib.check(lib.mk_lat_lerp_bwd(gy.data_ptr(), code, H * W, W, gxb.data_ptr(), 0, H * W, W, tables.rowptr.data_ptr(),
                                                       tables.term_row.data_ptr(), tables.term_coef.data_ptr(),
                                                       s32.data_ptr() if norm else None, C, B * C, H, H, W, st), "mk_lat_lerp_bwd")

                    n = B * C * H * W
                    for name, fn, by in (("mk_lat_lerp_fwd", kf, n * (4 + y.element_size())), ("mk_lat_lerp_bwd", kb, n * (gy.element_size() + 4))):
                        for _ in range(2):
                            fn()
                        sec = window(fn, 20)
                        k = dict(kernel=f"{name}, {tag}", B=B, ms=round(sec * 1e3, 4), bytes=by, TBs=round(by / sec / 1e12, 2))
                        kernels.append(k)
                        print(f"{'kernel: ' + k['kernel']:>44} {B:>2} {k['ms']:>10.3f} ms {k['TBs']:>6.2f} TB/s (algorithmic)", flush=True)
                    del y, gxb
                torch.cuda.empty_cache()
        del x, gy
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(dict(tool="grid_bench", window_s=args.window, rounds=args.rounds, rows=rows, kernels=kernels), fh, indent=1)
    losing = [r for r in rows if r["ratio"] < 1.0]
    print(f"grid_bench: done, {len(losing)} of {len(rows)} rows slower than the torch path")
    for r in losing:
        print(f"  slower: {r['row']} B={r['B']} ({r['ratio']:.2f})")


class with_env:
    """``os.environ[name] = value`` for a block."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = os.environ.get(self.name)
        os.environ[self.name] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.old


if __name__ == "__main__":
    main()
