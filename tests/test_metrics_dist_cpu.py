"""world-size 2 / 4 gloo tests (CPU) of MetricsHandler under spatial and data parallelism: every rank feeds its own
h / w shard of uneven 33 x 60 fields (and its own batches under data parallelism); the spatial partial sums are
all-reduced, the curves reduced over the data ranks, and every rank's finalize() must equal the single-process result
on the full field.  The spawn pattern of test_distributed_cpu.py, with a launcher of its own."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_metrics_cpu import make_params, make_rollout, rel, run_handler

TOL = 1e-6
H, W, B, STEPS = 33, 60, 2, 2


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _problem(n_data):
    params = make_params(H, W, steps=STEPS)
    clim, mult, batches = make_rollout(B, len(params.channel_names), H, W, STEPS, seed=41, n_batches=n_data)
    return params, clim, mult, batches


def _summary(logs, acc, rmse):
    out = {k: float(v) for k, v in logs["base"].items()}
    out.update({k: float(v) for k, v in logs["metrics"].items() if k != "rollouts"})
    out["acc"], out["rmse"] = acc.numpy().copy(), rmse.numpy().copy()
    return out


def _worker(rank, world, port, hsize, wsize, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank))
        torch.set_num_threads(1)
        from makani_amd import comm
        from makani_amd.distributed import split_tensor_along_dim
        comm.init(model_parallel_sizes=[hsize, wsize, 1, 1], backend="gloo")
        params, clim, mult, batches = _problem(comm.get_size("data"))

        def shard(x):
            x = split_tensor_along_dim(x, -2, comm.get_size("h"))[comm.get_rank("h")]
            return split_tensor_along_dim(x, -1, comm.get_size("w"))[comm.get_rank("w")].contiguous()

        h, logs, acc, rmse = run_handler(params, mult, clim, [batches[comm.get_rank("data")]], shard=shard)
        # the trainer's visualisation gather still returns the full field
        assert torch.equal(h._gather_input(shard(batches[0][0][0])), batches[0][0][0])
        dist.barrier()
        q.put((rank, _summary(logs, acc, rmse)))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, "".join(traceback.format_exception(type(e), e, e.__traceback__))))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def _run(world, hsize, wsize):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, hsize, wsize, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    bad = {r: m for r, m in results.items() if isinstance(m, str)}
    assert not bad, "\n".join(f"rank {r}: {m}" for r, m in bad.items())
    return results


@pytest.mark.parametrize("hsize,wsize,data", [(2, 1, 1), (2, 2, 1), (2, 1, 2)])
def test_sharded_handler_equals_single_process(hsize, wsize, data):
    world = hsize * wsize * data
    results = _run(world, hsize, wsize)
    params, clim, mult, batches = _problem(data)
    _, logs, acc, rmse = run_handler(params, mult, clim, batches)       # one process, full field, every batch
    want = _summary(logs, acc, rmse)
    for r, got in results.items():
        assert got["validation steps"] == 1.0                            # the local count, as the reference logs it
        for key, val in want.items():
            if key == "validation steps":
                continue
            assert rel(got[key], val) < TOL, (r, key)
    for r, got in results.items():
        for key in want:
            assert rel(got[key], results[0][key]) < 1e-7, (r, key)
    assert want["validation steps"] == data
    assert np.all(want["acc"] > 0.5)
