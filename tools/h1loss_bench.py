"""LossHandler("geometric h1") forward + backward on the production field [B, 73, 721, 1440] (B = 1, 2; relative and
absolute), one process: the path on the packed spectrum (RealSHT.forward_packed -> ops.degree_power -> [B, C, L] float64
sums) alternated with the LossHandler of an older makani_amd/losses.py (spec_unpack, the view_as_real chain of torch ops
and its autograd, spec_pack).  Medians of device-event times with the 10th / 90th percentiles of both sides; the two
handlers share one transform object (one Legendre table of 721 x 721 x 736 fp32 and its engine images).

Then the two C entry points alone (mk_degree_power incl. its finalize, mk_degree_power_bwd) on a packed spectrum
[721, 721, B 73] against the bytes they must move: forward the stored triangle (l >= m) once, backward the stored triangle
read and the whole spectrum written.  Last, what a spatially sharded rank no longer moves, as a byte count.

    python tools/h1loss_bench.py [--iters N] [--parent PATH] [--quick]

--parent PATH: a copy of an older makani_amd/losses.py; imported next to the current one, its LossHandler is the timed
baseline, and its loss and gradient are first compared with the new path on the timed input.  Without it only the new
path is timed.
--quick: 3 steps of the new path alone at B = 1, so that a kernel trace shows what one step launches.

The loss has not been run at lmax = 721 before.  Sizes are tried from the production grid down; a size the transform
refuses (an error from a table or a kernel's argument check) is reported and the next smaller one is used and named."""
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

from makani_amd import _lib  # noqa: E402
from makani_amd.losses import LossHandler  # noqa: E402

C = 73
SIZES = [(721, 1440), (361, 720), (181, 360), (91, 180)]
SPELLINGS = ["geometric h1", "absolute geometric h1"]


def make_params(spec, H, W):
    return SimpleNamespace(loss=spec, n_future=0, img_shape_x=H, img_shape_y=W, img_crop_shape_x=H, img_crop_shape_y=W,
                           img_crop_offset_x=0, img_crop_offset_y=0, N_out_channels=C,
                           channel_names=[f"c{i}" for i in range(C)], channel_weights="auto", model_grid_type="equiangular")


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


def pick_size(dev, gen):
    """The largest grid of SIZES on which one forward + backward of the new path runs; every refused size is reported."""
    for H, W in SIZES:
        try:
            h = LossHandler(make_params(SPELLINGS[0], H, W)).to(dev)
            h.train()
            tar = torch.randn(1, C, H, W, device=dev, generator=gen)
            x = (tar + 0.3 * torch.randn(1, C, H, W, device=dev, generator=gen)).requires_grad_(True)
            step(h, x, tar)
            torch.cuda.synchronize()
            ok = bool(torch.isfinite(x.grad).all())
            if not ok:
                raise RuntimeError("non-finite gradient")
            sht = h.loss_obj.sht
            print(json.dumps(dict(size=[H, W], lmax=sht.lmax, mmax=sht.mmax, runs=True,
                                  production=(H, W) == SIZES[0])), flush=True)
            return H, W, sht
        except RuntimeError as e:
            print(json.dumps(dict(size=[H, W], runs=False, error=str(e)[:300])), flush=True)
            torch.cuda.empty_cache()
    raise SystemExit("no size of the list runs")


def bench_handlers(args, parent, dev, gen, H, W, sht):
    spellings = SPELLINGS[:1] if args.quick else SPELLINGS
    handlers = {}
    for spec in spellings:
        pair = [LossHandler(make_params(spec, H, W)), parent.LossHandler(make_params(spec, H, W)) if parent is not None else None]
        for i, h in enumerate(pair):
            if h is not None:
                h.loss_obj.sht = sht                    # one table for every handler of the run
                pair[i] = h.to(dev)
                pair[i].train()
        handlers[spec] = pair
    for B in ((1,) if args.quick else (1, 2)):
        tar = torch.randn(B, C, H, W, device=dev, generator=gen)
        x = (tar + 0.3 * torch.randn(B, C, H, W, device=dev, generator=gen)).requires_grad_(True)
        for spec in spellings:
            new, old = handlers[spec]
            t_new, t_old = [], []
            if args.quick:
                t_new = [timed(lambda: step(new, x, tar)) for _ in range(3)]
            else:
                for _ in range(2):                                        # warm-up
                    step(new, x, tar)
                    if old is not None:
                        step(old, x, tar)
                agree = None
                if old is not None:                                       # same inputs, same loss and gradient to fp32 rounding
                    step(new, x, tar)
                    g_new, l_new = x.grad.clone(), float(new(x, tar, None).detach())
                    step(old, x, tar)
                    l_old = float(old(x, tar, None).detach())
                    agree = dict(loss_rel=abs(l_new - l_old) / abs(l_old),
                                 grad_rel=float(torch.linalg.norm((g_new - x.grad).double()) / torch.linalg.norm(x.grad.double())))
                    del g_new
                for _ in range(args.iters):
                    t_new.append(timed(lambda: step(new, x, tar)))
                    if old is not None:
                        t_old.append(timed(lambda: step(old, x, tar)))
            line = dict(loss=spec, B=B, size=[H, W], new_ms=summary(t_new))
            if t_old:
                so = summary(t_old)
                line.update(parent_ms=so, speedup=round(so["med"] / line["new_ms"]["med"], 2), new_vs_parent=agree)
            print(json.dumps(line), flush=True)
        del tar, x
        torch.cuda.empty_cache()


def bench_kernels(args, dev, gen, L, M):
    """The C entry points alone on preallocated buffers; the empty triangle of the spectrum holds NaN."""
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    stored = sum(min(l + 1, M) for l in range(L))
    for B in (1, 2):
        bc = B * C
        c = torch.view_as_complex(torch.randn(L, M, bc, 2, device=dev, generator=gen))
        l = torch.arange(L, device=dev).reshape(L, 1)
        m = torch.arange(M, device=dev).reshape(1, M)
        c[(l < m)] = complex(float("nan"), float("nan"))
        gc = torch.empty_like(c)
        ws = torch.empty(lib.mk_degree_power_workspace(L, M, bc), dtype=torch.float64, device=dev)
        P = torch.empty(L, bc, dtype=torch.float64, device=dev)
        gP = torch.rand(L, bc, dtype=torch.float64, device=dev, generator=gen)

        def fwd():
            _lib.check(lib.mk_degree_power(c.data_ptr(), ws.data_ptr(), P.data_ptr(), L, M, bc, 0, 0, st))

        def bwd():
            _lib.check(lib.mk_degree_power_bwd(c.data_ptr(), gP.data_ptr(), gc.data_ptr(), L, M, bc, 0, 0, st))

        for _ in range(2):
            fwd()
            bwd()
        assert bool(torch.isfinite(P).all()) and bool(torch.isfinite(torch.view_as_real(gc)).all())
        tf, tb = [], []
        for _ in range(args.iters):
            tf.append(timed(fwd))
            tb.append(timed(bwd))
        bf, bb = stored * bc * 8, (stored + L * M) * bc * 8
        sf, sb = summary(tf), summary(tb)
        print(json.dumps(dict(kernel="mk_degree_power / mk_degree_power_bwd", B=B, L=L, M=M, BC=bc,
                              fwd_MB=round(bf / 1e6, 1), fwd_ms=sf, fwd_TBps=round(bf / sf["med"] / 1e9, 2),
                              bwd_MB=round(bb / 1e6, 1), bwd_ms=sb, bwd_TBps=round(bb / sb["med"] / 1e9, 2))), flush=True)
        del c, gc, ws
        torch.cuda.empty_cache()


def sharded_bytes(H, W):
    """Per rank and per step under spatial parallelism, B = 1: before, both fields were gathered in full on every rank (and
    transformed in full there); now two [B, 2] float64 all-reduces (one for an absolute loss)."""
    field = C * H * W * 4
    print(json.dumps(dict(sharded="per rank, B = 1", gathered_before_MB=round(2 * field / 1e6, 1),
                          all_reduced_now_bytes=2 * 2 * 8, transforms_before="2 full fields on every rank",
                          transforms_now="2 shards per rank")), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--parent", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(7)
    parent = load_parent(args.parent) if args.parent else None
    H, W, sht = pick_size(dev, gen)
    bench_handlers(args, parent, dev, gen, H, W, sht)
    if not args.quick:
        bench_kernels(args, dev, gen, sht.lmax, sht.mmax)
        sharded_bytes(H, W)


if __name__ == "__main__":
    main()
