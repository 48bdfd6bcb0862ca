"""LossHandler forward + backward on the production field [B, 73, 721, 1440] (B = 1, 2; fp32 and bf16 predictions), one
process: the HIP path (ops.geo_lp_sums + the [B, C] epilogue) alternated with the eager-torch formulation this package
ran before it had the kernels (the reference's, makani/utils/losses.py:213-249), for "geometric l2", "weighted squared
geometric l2" with unequal channel weights and "absolute geometric l1".  Medians of device-event times with the
10th / 90th percentiles of both sides.

Then, per (B, dtype, p): the two C entry points alone (mk_geo_lp_sums incl. its finalize, mk_geo_lp_bwd) against the
bytes they must move -- forward B (bytes(p) + 4) C H W, backward B (2 bytes(p) + 4) C H W -- and the absolute squared
L2 loss with uniform weights through the sums against the same loss through mk_wmse_*.

    python tools/loss_bench.py [--quick] [--iters N] [--parent PATH]

--parent PATH: a copy of an older makani_amd/losses.py.  It is imported next to the current one, the eager formulation
kept here is first checked against it to the last bit (loss and gradient) on one input, and the timed baseline is then
that file's own LossHandler.
--quick: 3 steps of the HIP path alone at B = 1 fp32, so that a kernel trace (rocprofv3 --kernel-trace --stats) shows
what one step launches."""
import argparse
import importlib.util
import json
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from makani_amd import _lib, ops  # noqa: E402
from makani_amd.losses import LossHandler  # noqa: E402

C, H, W = 73, 721, 1440
SPELLINGS = ["geometric l2", "weighted squared geometric l2", "absolute geometric l1"]


class EagerHandler:
    """The Lp losses as eager torch ops on the full fields, with the handler's weights."""

    def __init__(self, handler):
        self.h, self.o = handler, handler.loss_obj
        self.q = self.o.quadrature.quad_weight                       # [1, 1, H, W]

    def quad(self, x):
        return torch.sum(x * self.q, dim=(-2, -1))

    def __call__(self, prd, tar, inp=None):
        h, o = self.h, self.o
        chw = h.channel_weights
        chw = (chw * h.multistep_weight).reshape(1, -1) if h.training else chw.reshape(1, -1)
        n = prd.size()[0]
        norms = self.quad(torch.abs(prd - tar) ** o.p).reshape(n, -1)
        if not o.absolute:
            norms = norms / self.quad(torch.abs(tar) ** o.p).reshape(n, -1)
        if not o.squared:
            norms = norms ** (1.0 / o.p)
        return torch.sum(chw * norms)


def make_params(spec):
    g = torch.Generator().manual_seed(3)
    return SimpleNamespace(loss=spec, n_future=0, img_shape_x=H, img_shape_y=W, img_crop_shape_x=H, img_crop_shape_y=W,
                           img_crop_offset_x=0, img_crop_offset_y=0, N_out_channels=C,
                           channel_names=[f"c{i}" for i in range(C)],
                           channel_weights=(torch.rand(C, generator=g) + 0.5).tolist(), model_grid_type="equiangular")


def load_parent(path):
    spec = importlib.util.spec_from_file_location("makani_amd._parent_losses", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(ts):
    ts = sorted(ts)
    return dict(med=round(statistics.median(ts), 4), p10=round(ts[len(ts) // 10], 4), p90=round(ts[(9 * len(ts)) // 10], 4))


def step(loss_fn, x, tar):
    x.grad = None
    loss_fn(x, tar, None).backward()


def check_restatement(parent, dev):
    """The eager formulation above equals the older file's handler bit for bit (loss and gradient) on one input."""
    g = torch.Generator(device=dev).manual_seed(1)
    tar = torch.randn(1, C, 91, 180, device=dev, generator=g)
    prd = torch.randn(1, C, 91, 180, device=dev, generator=g)
    for spec in SPELLINGS:
        params = make_params(spec)
        params.img_shape_x = params.img_crop_shape_x = 91
        params.img_shape_y = params.img_crop_shape_y = 180
        old = parent.LossHandler(params).to(dev)
        old.train()
        out = []
        for fn in (old, EagerHandler(old)):
            x = prd.clone().requires_grad_(True)
            loss = fn(x, tar, None)
            loss.backward()
            out.append((loss.detach(), x.grad))
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]), spec
    print(json.dumps(dict(check="eager formulation == --parent LossHandler, bitwise", spellings=SPELLINGS)), flush=True)


def bench_handlers(args, parent, dev, gen):
    cases = [(1, torch.float32)] if args.quick else [(1, torch.float32), (1, torch.bfloat16), (2, torch.float32),
                                                     (2, torch.bfloat16)]
    for B, dtype in cases:
        tar = torch.randn(B, C, H, W, device=dev, generator=gen)
        x = (tar + 0.3 * torch.randn(B, C, H, W, device=dev, generator=gen)).to(dtype).requires_grad_(True)
        for spec in SPELLINGS[:1] if args.quick else SPELLINGS:
            new = LossHandler(make_params(spec)).to(dev)
            new.train()
            if parent is not None:
                old = parent.LossHandler(make_params(spec)).to(dev)
                old.train()
            else:
                old = EagerHandler(new)
            t_new, t_old = [], []
            if args.quick:
                t_new = [timed(lambda: step(new, x, tar)) for _ in range(3)]
                t_old = [float("nan")]
            else:
                for _ in range(2):                                        # warm-up
                    step(new, x, tar)
                    step(old, x, tar)
                # same inputs, same loss to rounding
                l_new, l_old = float(new(x, tar, None).detach()), float(old(x, tar, None).detach())
                assert abs(l_new - l_old) < 5e-6 * abs(l_old), (spec, l_new, l_old)
                for _ in range(args.iters):
                    t_new.append(timed(lambda: step(new, x, tar)))
                    t_old.append(timed(lambda: step(old, x, tar)))
            sn, so = summary(t_new), summary(t_old)
            print(json.dumps(dict(loss=spec, B=B, dtype=str(dtype).replace("torch.", ""), hip_ms=sn, eager_ms=so,
                                  baseline="parent" if parent is not None else "restatement",
                                  speedup=round(so["med"] / sn["med"], 1))), flush=True)
        del tar, x
        torch.cuda.empty_cache()


def bench_kernels(args, dev, gen):
    """The C entry points alone on preallocated buffers."""
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    wrow = torch.rand(H, device=dev, generator=gen) + 0.1
    for B, dtype, p in [(b, d, p) for b in (1, 2) for d in (torch.float32, torch.bfloat16) for p in (2, 1)]:
        tar = torch.randn(B, C, H, W, device=dev, generator=gen)
        prd = (tar + 0.3 * torch.randn(B, C, H, W, device=dev, generator=gen)).to(dtype)
        gp = torch.empty_like(prd)
        g = torch.rand(B, C, device=dev, generator=gen)
        ws = torch.empty(lib.mk_geo_lp_workspace(B, C, H), dtype=torch.float64, device=dev)
        out = torch.empty(B, C, 2, dtype=torch.float64, device=dev)
        dt = ops._pw_dtype(prd)

        def fwd():
            _lib.check(lib.mk_geo_lp_sums(prd.data_ptr(), dt, tar.data_ptr(), wrow.data_ptr(), ws.data_ptr(), out.data_ptr(),
                                          p, B, C, H, W, st))

        def bwd():
            _lib.check(lib.mk_geo_lp_bwd(prd.data_ptr(), dt, tar.data_ptr(), wrow.data_ptr(), g.data_ptr(), gp.data_ptr(), p,
                                         B, C, H, W, st))

        for _ in range(2):
            fwd()
            bwd()
        tf, tb = [], []
        for _ in range(args.iters):
            tf.append(timed(fwd))
            tb.append(timed(bwd))
        n = B * C * H * W
        bf, bb = n * (prd.element_size() + 4), n * (2 * prd.element_size() + 4)
        sf, sb = summary(tf), summary(tb)
        print(json.dumps(dict(kernel="mk_geo_lp_sums / mk_geo_lp_bwd", B=B, dtype=str(dtype).replace("torch.", ""), p=p,
                              fwd_MB=round(bf / 1e6, 1), fwd_ms=sf, fwd_TBps=round(bf / sf["med"] / 1e9, 2),
                              bwd_MB=round(bb / 1e6, 1), bwd_ms=sb, bwd_TBps=round(bb / sb["med"] / 1e9, 2))), flush=True)
        del tar, prd, gp
        torch.cuda.empty_cache()


def bench_uniform(args, dev, gen):
    """"absolute squared geometric l2" with uniform weights: through mk_wmse_* (as the handler routes it) and through
    the sums (the handler's host-side knowledge of the uniform weight withheld)."""
    for B, dtype in [(1, torch.float32), (1, torch.bfloat16)]:
        tar = torch.randn(B, C, H, W, device=dev, generator=gen)
        x = (tar + 0.3 * torch.randn(B, C, H, W, device=dev, generator=gen)).to(dtype).requires_grad_(True)
        wmse = LossHandler(make_params("absolute squared geometric l2")).to(dev)
        sums = LossHandler(make_params("absolute squared geometric l2")).to(dev)
        sums._uniform = {True: None, False: None}
        for h in (wmse, sums):
            h.train()
        assert type(wmse(x, tar, None).grad_fn).__name__ == "_WeightedMSEBackward"
        assert type(sums(x, tar, None).grad_fn).__name__ != "_WeightedMSEBackward"
        for _ in range(2):
            step(wmse, x, tar)
            step(sums, x, tar)
        tw, ts = [], []
        for _ in range(args.iters):
            tw.append(timed(lambda: step(wmse, x, tar)))
            ts.append(timed(lambda: step(sums, x, tar)))
        print(json.dumps(dict(loss="absolute squared geometric l2 (uniform)", B=B, dtype=str(dtype).replace("torch.", ""),
                              wmse_ms=summary(tw), sums_ms=summary(ts))), flush=True)
        del tar, x
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--parent", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(7)
    parent = load_parent(args.parent) if args.parent else None
    if parent is not None:
        check_restatement(parent, dev)
    bench_handlers(args, parent, dev, gen)
    if not args.quick:
        bench_kernels(args, dev, gen)
        bench_uniform(args, dev, gen)


if __name__ == "__main__":
    main()
