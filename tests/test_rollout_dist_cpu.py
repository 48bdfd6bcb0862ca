"""world-size 2 gloo tests (CPU) of Rollout under spatial parallelism: every rank rolls out its own h / w shard of uneven
13 x 24 fields (a toy model of elementwise operations, mode "none", so a shard's prediction is the slice of the full
field's bit for bit).  The ``[B, C, 6]`` sums take one all-reduce per step and must equal the single-process sums to 1e-12 relative (float64
partial sums added in another order); the map and the emitted fields stay sharded and equal the slices bit for bit,
``finalize(gather=True)`` returns the full map; the curves equal the single-process run to 1e-6.  The spawn pattern of
test_metrics_dist_cpu.py."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_rollout_cpu import build, make_params, make_problem

H, W, B, T, STEPS = 13, 24, 2, 2, 3
OUT = [2, 0]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _params(tmp, hs=None, ws=None, i=0, j=0):
    kw = dict(n_history=T - 1, masked_channels=[1], held_channels=[2])
    if hs is not None:
        kw.update(img_local_offset_x=sum(hs[:i]), img_local_shape_x=hs[i], img_local_offset_y=sum(ws[:j]), img_local_shape_y=ws[j])
    return make_params(H, W, tmp, steps=STEPS, **kw)


class _Pointwise(torch.nn.Module):
    """The channel mix of the toy model as elementwise products and sums in a fixed order: a point's value does not depend
    on the extent of the field around it (a library convolution may pick another kernel for another extent)."""

    def __init__(self, w, b):
        super().__init__()
        self.w, self.b = torch.nn.Parameter(w[:, :, 0, 0].clone()), torch.nn.Parameter(b.clone())

    def forward(self, x):
        out = []
        for c in range(self.w.shape[0]):
            acc = x[:, 0] * self.w[c, 0]
            for k in range(1, self.w.shape[1]):
                acc = acc + x[:, k] * self.w[c, k]
            out.append(acc + self.b[c])
        return torch.stack(out, dim=1)


def _rollout(params, prob, shard=None):
    from makani_amd.inference import Rollout
    shard = shard or (lambda x: x)
    wrap, h, loss = build(params, prob, shard=shard, model=lambda: _Pointwise(prob.w, prob.b))
    ro = Rollout(params, wrap, metrics=h, loss=loss)
    emitted = ro.run(shard(prob.inp), shard(prob.tar), output_channels=OUT)
    curve, space = ro.finalize()
    _, full = ro.finalize(gather=True)
    return dict(emit=emitted.numpy(), sums=ro.last_sums.numpy(), space=space.numpy(), full=full.numpy(), curve=curve.numpy(),
                acc=h.acc_curve.numpy().copy(), rmse=h.rmse_curve.numpy().copy(), calls=None)


def _worker(rank, world, port, hsize, wsize, tmp, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank))
        torch.set_num_threads(1)
        from makani_amd import comm, inference
        from makani_amd.distributed import compute_split_shapes, split_tensor_along_dim
        comm.init(model_parallel_sizes=[hsize, wsize, 1, 1], backend="gloo")
        i, j = comm.get_rank("h"), comm.get_rank("w")
        hs, ws = compute_split_shapes(H, hsize), compute_split_shapes(W, wsize)
        calls = []
        all_reduce = inference.dist.all_reduce

        def shard(x):
            x = split_tensor_along_dim(x, -2, hsize)[i]
            return split_tensor_along_dim(x, -1, wsize)[j].contiguous()

        class CountedDist:
            def __getattr__(self, name):
                if name == "all_reduce":
                    return lambda t, **kw: calls.append(tuple(t.shape)) or all_reduce(t, **kw)
                return getattr(dist, name)

        inference.dist = CountedDist()
        out = _rollout(_params(tmp, hs, ws, i, j), make_problem(B, T, H, W, STEPS, seed=31), shard)
        out["calls"] = list(calls)
        dist.barrier()
        q.put((rank, ((i, j), out)))          # numpy arrays travel through the queue by value
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, "".join(traceback.format_exception(type(e), e, e.__traceback__))))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def _run(world, hsize, wsize, tmp):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, hsize, wsize, tmp, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    bad = {r: m for r, m in results.items() if isinstance(m, str)}
    assert not bad, "\n".join(f"rank {r}: {m}" for r, m in bad.items())
    return results


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float(((a - b).abs() / b.abs()).max())


@pytest.mark.parametrize("hsize,wsize", [(2, 1), (1, 2)])
def test_sharded_rollout_equals_single_process(tmp_path, hsize, wsize):
    from makani_amd.distributed import compute_split_shapes
    results = _run(2, hsize, wsize, tmp_path)
    want = _rollout(_params(tmp_path), make_problem(B, T, H, W, STEPS, seed=31))
    hs, ws = compute_split_shapes(H, hsize), compute_split_shapes(W, wsize)
    assert sorted(w for w, _ in results.values()) == [(i, j) for i in range(hsize) for j in range(wsize)]
    for r, ((i, j), got) in results.items():
        rows, cols = slice(sum(hs[:i]), sum(hs[:i + 1])), slice(sum(ws[:j]), sum(ws[:j + 1]))
        assert got["calls"] == [(B, 3, 6)] * STEPS, (r, got["calls"])           # one all-reduce of the sums per step
        assert _rel(got["sums"], want["sums"]) < 1e-12, r
        assert (got["emit"] == want["emit"][..., rows, cols]).all(), r
        assert (got["space"] == want["space"][..., rows, cols]).all(), r
        assert (got["full"] == want["space"]).all(), r
        assert _rel(got["curve"], want["curve"]) < 1e-6, r
        assert _rel(got["rmse"], want["rmse"]) < 1e-6, r
        assert float(abs(torch.as_tensor(got["acc"]) - torch.as_tensor(want["acc"])).max()) < 1e-6 * B, r
