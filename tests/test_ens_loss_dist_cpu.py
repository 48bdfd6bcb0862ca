"""gloo test (CPU) of ``LossHandler("ensemble crps")`` under spatial parallelism: two ranks split 33 x 60 fields along ``h``
(17 and 16 rows), each forms the two integrals of its own rows, the ``[B, C, 2]`` float64 sums are all-reduced over the
spatial group and no field is gathered (the gather is replaced by a function that raises).  Every rank's loss must equal the
unsharded one to 1e-12 relative and its input gradient must be bit-equal to its slice of the unsharded gradient: the
gradient of a point depends on its own members, its row's weight and the channel weights only.  The spawn pattern of
test_lploss_dist_cpu.py."""
import os

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import ens_loss_checks as lc
from test_lploss_cpu import make_params
from test_lploss_dist_cpu import _free_port, _no_gather, count_reduces

H, W, B, C, E = 33, 60, 2, 6, 3
SPEC = "weighted ensemble crps"


def _params():
    params = make_params(SPEC, H, W)
    params.ensemble_size = E
    return params


def _problem():
    ens, tar, _, _ = lc.problem((B, E, C, H, W), "float32", "ties")
    return torch.from_numpy(np.array(ens)).reshape(B * E, C, H, W), torch.from_numpy(np.array(tar))


def _worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank))
        torch.set_num_threads(1)
        from makani_amd import comm, losses
        from makani_amd.distributed import split_tensor_along_dim
        comm.init(model_parallel_sizes=[world, 1, 1, 1], backend="gloo")
        losses.gather_from_parallel_region = _no_gather
        reduces = count_reduces(losses)
        prd, tar = _problem()
        hr = comm.get_rank("h")
        shard = lambda x: split_tensor_along_dim(x, -2, comm.get_size("h"))[hr].contiguous()
        handler = losses.LossHandler(_params()).train()
        assert handler.do_gather_input
        x = shard(prd).clone().requires_grad_(True)
        loss = handler(x, shard(tar), None)
        assert reduces == ["spatial"], reduces      # ONE all-reduce of the [B, C, 2] sums per forward (and no gather: it raises)
        loss.backward()
        dist.barrier()
        q.put((rank, (hr, float(loss.detach()), x.grad.clone(), handler.loss_obj.last_sums.clone())))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, "".join(traceback.format_exception(type(e), e, e.__traceback__))))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_sharded_crps_loss_equals_the_unsharded_one_without_a_gather():
    from makani_amd.distributed import compute_split_shapes
    from makani_amd.losses import LossHandler
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    bad = {r: m for r, m in results.items() if isinstance(m, str)}
    assert not bad, "\n".join(f"rank {r}: {m}" for r, m in bad.items())
    prd, tar = _problem()
    handler = LossHandler(_params()).train()
    x = prd.clone().requires_grad_(True)
    want = handler(x, tar, None)
    want.backward()
    want = float(want.detach())
    hs = compute_split_shapes(H, world)
    assert hs == [17, 16] and sorted(r[0] for r in results.values()) == [0, 1]
    whole = torch.zeros_like(handler.loss_obj.last_sums)
    for r, (hr, loss, grad, last) in results.items():
        assert abs(loss - want) <= 1e-12 * abs(want), (r, loss, want)
        rows = slice(sum(hs[:hr]), sum(hs[:hr + 1]))
        assert grad.shape == x.grad[:, :, rows].shape and torch.equal(grad, x.grad[:, :, rows]), r
        whole += last                       # last_sums is of the rank's own rows
    assert torch.allclose(whole[..., :2], handler.loss_obj.last_sums[..., :2], rtol=1e-12, atol=0)
