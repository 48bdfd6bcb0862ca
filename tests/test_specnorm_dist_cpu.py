"""world-size 2 / 4 gloo tests (CPU) of the sharded combination of the H1 loss: every rank holds its (l, m) slice of one
synthetic packed spectrum (uneven: 33 degrees, 17 orders), forms its ``[B, 2]`` partial sums with
``GeometricH1Loss.norms_from_spectrum`` at the offsets of the loss's own ``DistributedRealSHT`` and all-reduces them over
the ``"spatial"`` group.  Every rank must hold the sums of the whole spectrum, and the all-reduce must hand the upstream
gradient to the rank's partial sums unchanged.  No transform runs here (it has no CPU path).  The spawn pattern of
test_lploss_dist_cpu.py, with a launcher of its own."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_specnorm_cpu import L, M, norms_numpy, packed_spectrum

B, C = 2, 3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, hsize, wsize, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank))
        torch.set_num_threads(1)
        from makani_amd import comm
        from makani_amd.losses import GeometricH1Loss
        from makani_amd.mappings import reduce_from_parallel_region
        comm.init(model_parallel_sizes=[hsize, wsize, 1, 1], backend="gloo")
        loss = GeometricH1Loss((L, 2 * (M - 1)))
        sht = loss.sht
        assert loss.sharded and (sht.lmax, sht.mmax) == (L, M)
        c = packed_spectrum(L, M, B * C, seed=21)
        shard = c[sht.l_off:sht.l_off + sht.lmax_local, sht.m_off:sht.m_off + sht.mmax_local].contiguous()
        shard.requires_grad_(True)
        part = loss.norms_from_spectrum(shard, B, sht.l_off, sht.m_off)
        total = reduce_from_parallel_region(part, "spatial")
        g = torch.randn(B, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(22))
        (total * g).sum().backward()
        # the same upstream gradient applied to the rank's own partial sums, without the collective
        alone = shard.detach().clone().requires_grad_(True)
        (loss.norms_from_spectrum(alone, B, sht.l_off, sht.m_off) * g).sum().backward()
        dist.barrier()
        q.put((rank, ((comm.get_rank("h"), comm.get_rank("w")), tuple(shard.shape), total.detach(), part.detach(),
                      bool(torch.equal(shard.grad, alone.grad)), float(shard.grad.abs().sum()))))
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


@pytest.mark.parametrize("hsize,wsize", [(2, 1), (1, 2), (2, 2)])
def test_sharded_h1_sums_equal_the_whole_spectrum(hsize, wsize):
    from makani_amd.distributed import compute_split_shapes
    results = _run(hsize * wsize, hsize, wsize)
    ls, ms = compute_split_shapes(L, hsize), compute_split_shapes(M, wsize)
    want = norms_numpy(packed_spectrum(L, M, B * C, seed=21), B)
    assert sorted(w for w, *_ in results.values()) == [(i, j) for i in range(hsize) for j in range(wsize)]
    for r, ((i, j), shape, total, part, same_grad, grad_mass) in results.items():
        assert shape == (ls[i], ms[j], B * C), r
        assert total.dtype == torch.float64 and tuple(total.shape) == (B, 2), r
        assert abs(total.numpy() / want - 1).max() <= 1e-12, r
        assert (part.numpy() < want).all(), r          # a proper part of the whole on every rank
        assert same_grad and grad_mass > 0, r
