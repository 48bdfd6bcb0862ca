"""Two ranks (h = 2) sharing cuda:0 over gloo: ``DistributedRealFFT2`` / ``DistributedInverseRealFFT2`` with their local
transforms on the HIP kernels (``MK_PLANAR_FFT=hip``) against the local modules, gathered output and input gradient, in the
measure and at the bound of the reference's ``tests/distributed/tests_fft.py`` (mean per-field relative L2 error <= 1e-6).
Built like ``tests/test_distributed_gpu.py``: the ranks take turns on the one card around every collective."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_distributed_gpu import _free_port, _gather, _shard, _take_turns_on_the_card

pytestmark = pytest.mark.gpu

BOUND = 1e-6
GRIDS = [(64, 96, 21, 17), (91, 180, 70, 61)]       # the second with uneven latitude and mode shards


def _err(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    cplx = a.is_complex() or b.is_complex()
    a = a.to(torch.complex128) if cplx else a.double()
    b = b.to(torch.complex128) if cplx else b.double()
    return torch.mean(torch.linalg.vector_norm(a - b, dim=(-2, -1)) / torch.linalg.vector_norm(b, dim=(-2, -1))).item()


def _body(dev, grid):
    from makani_amd.distributed import DistributedInverseRealFFT2, DistributedRealFFT2
    from makani_amd.layers import InverseRealFFT2, RealFFT2
    nlat, nlon, lmax, mmax = grid
    B, C = 2, 4
    torch.manual_seed(333)
    xg = torch.randn(B, C, nlat, nlon)
    gg = torch.complex(torch.randn(B, C, lmax, mmax), torch.randn(B, C, lmax, mmax))
    cg = torch.complex(torch.randn(B, C, lmax, mmax), torch.randn(B, C, lmax, mmax))
    hg = torch.randn(B, C, nlat, nlon)
    f_l, f_d = RealFFT2(nlat, nlon, lmax=lmax, mmax=mmax).to(dev), DistributedRealFFT2(nlat, nlon, lmax=lmax, mmax=mmax).to(dev)
    i_l, i_d = InverseRealFFT2(nlat, nlon, lmax=lmax, mmax=mmax).to(dev), DistributedInverseRealFFT2(nlat, nlon, lmax=lmax, mmax=mmax).to(dev)
    assert list(f_d.state_dict()) == [] and f_d._hip(xg.to(dev)) and f_l.hip_ready(xg.to(dev))
    # forward: local module on the whole field, distributed module on this rank's latitudes
    xo = xg.to(dev).requires_grad_(True)
    yo = f_l(xo)
    yo.backward(gg.to(dev))
    xl = _shard(xg, 2, "h").to(dev).requires_grad_(True)
    yl = f_d(xl)
    assert tuple(yl.shape) == (B, C, f_d.l_shapes[dist.get_rank()], mmax)
    yl.backward(_shard(gg, 2, "h").to(dev))
    e = (_err(_gather(yl.detach(), 2, "h"), yo), _err(_gather(xl.grad, 2, "h"), xo.grad))
    print(f"[fft2] distributed forward {grid}: out={e[0]:.3e} grad={e[1]:.3e}")
    assert max(e) <= BOUND
    # inverse
    co = cg.to(dev).requires_grad_(True)
    zo = i_l(co)
    zo.backward(hg.to(dev))
    cl = _shard(cg, 2, "h").to(dev).requires_grad_(True)
    zl = i_d(cl)
    assert tuple(zl.shape) == (B, C, i_d.lat_shapes[dist.get_rank()], nlon)
    zl.backward(_shard(hg, 2, "h").to(dev))
    e = (_err(_gather(zl.detach(), 2, "h"), zo), _err(_gather(cl.grad, 2, "h"), co.grad))
    print(f"[fft2] distributed inverse {grid}: out={e[0]:.3e} grad={e[1]:.3e}")
    assert max(e) <= BOUND


def _worker(rank, world, port, q, lock):
    held = False
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                          MK_PLANAR_FFT="hip")
        from makani_amd import comm
        comm.init(model_parallel_sizes=[world, 1, 1, 1], backend="gloo")
        dev = torch.device("cuda:0")
        _take_turns_on_the_card(lock)
        lock.acquire()
        held = True
        for grid in GRIDS:
            _body(dev, grid)
        torch.cuda.synchronize()
        dist.barrier()
        q.put((rank, "ok"))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, "".join(traceback.format_exception(type(e), e, e.__traceback__))))
    finally:
        if held:
            try:
                lock.release()
            except ValueError:
                pass
        if dist.is_initialized():
            dist.destroy_process_group()


def test_h2_planar_pair_on_one_gpu():
    assert torch.cuda.device_count() >= 1
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    lock = ctx.Lock()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, lock)) for r in range(2)]
    for p in procs:
        p.start()
    results = [q.get(timeout=600) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    bad = [r for r in results if r[1] != "ok"]
    assert not bad, "\n".join(f"rank {r}: {m}" for r, m in bad)
