"""world-size 2 / 4 gloo tests (CPU) of ``LossHandler("... spectral ensemble crps")`` under spatial parallelism.  The
transform has no CPU path, so every rank's ``DistributedRealSHT.forward_packed`` is replaced by a function that hands out the
rank's (l, m) slice of one synthetic packed spectrum (uneven: 13 degrees, 9 orders; the unstored triangle holds NaN) at the
offsets of the loss's own transform; everything behind it is the handler's: the per-degree sums of the rank's degrees and
orders, ONE all-reduce of ``[B, C, 2]`` over the ``"spatial"`` group, the loss.  No field or spectrum is gathered (the gather
is replaced by a function that raises).  Every rank's loss and all-reduced sums must equal the unsharded ones within the
float64 bound of tests/spec_crps_checks.py, and the gradient of its slice must equal the slice of the unsharded gradient
within 1e-5 relative L2 per row.  The spawn pattern of test_specnorm_dist_cpu.py."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import spec_crps_checks as sc
from kernel_checks import row_rel
from test_lploss_cpu import make_params
from test_lploss_dist_cpu import _free_port, _no_gather, count_reduces

L, M, B, E, C = 13, 9, 2, 3, 6
DIMS = (L, M, B, E, C)
H, W = L, 2 * (M - 1)
SPEC = "weighted fair spectral ensemble crps"
COMBINED = "weighted fair combined ensemble crps"


def _params(spec=SPEC):
    params = make_params(spec, H, W)
    params.ensemble_size = E
    params.crps_spectral_weight = 0.25
    return params


def _spectra():
    cp, ct, _ = sc.problem(DIMS, "ties")
    return torch.from_numpy(np.array(cp)), torch.from_numpy(np.array(ct))


def _run_handler(handler, cp, ct, h_loc, w_loc):
    """The handler on fields of the right (local) shape whose transform hands out ``cp`` (a leaf) and ``ct``: (loss, cp.grad,
    the sums the loss was formed from)."""
    calls, seen = [cp, ct], {}
    handler.spectral_obj.sht.forward_packed = lambda x: calls.pop(0)
    from_sums = handler.spectral_obj.from_sums
    handler.spectral_obj.from_sums = lambda s, chw: seen.setdefault("loss", from_sums(seen.setdefault("sums", s), chw))
    loss = handler(torch.zeros(B * E, C, h_loc, w_loc), torch.zeros(B, C, h_loc, w_loc), None)
    assert not calls
    loss.backward()
    return loss.detach(), cp.grad, seen["sums"].detach()


def _worker(rank, world, port, hsize, wsize, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank))
        torch.set_num_threads(1)
        from makani_amd import comm, losses
        comm.init(model_parallel_sizes=[hsize, wsize, 1, 1], backend="gloo")
        losses.gather_from_parallel_region = _no_gather
        reduces = count_reduces(losses)
        handler = losses.LossHandler(_params()).train()
        sht = handler.spectral_obj.sht
        assert handler.do_gather_input and handler.spectral_obj.sharded and (sht.lmax, sht.mmax) == (L, M)
        cp, ct = _spectra()
        ls, ms = slice(sht.l_off, sht.l_off + sht.lmax_local), slice(sht.m_off, sht.m_off + sht.mmax_local)
        shard = cp[ls, ms].contiguous().requires_grad_(True)
        loss, grad, sums = _run_handler(handler, shard, ct[ls, ms].contiguous(), sht.nlat_local, sht.nlon_local)
        assert reduces == ["spatial"], reduces              # the spectral term alone: ONE all-reduce per forward
        # "combined": the grid term's all-reduce and the spectral term's, nothing else (and no gather: it raises)
        del reduces[:]
        both = losses.LossHandler(_params(COMBINED)).train()
        _run_handler(both, shard.detach().clone().requires_grad_(True), ct[ls, ms].contiguous(), sht.nlat_local, sht.nlon_local)
        assert reduces == ["spatial", "spatial"], reduces
        dist.barrier()
        q.put((rank, ((comm.get_rank("h"), comm.get_rank("w")), (sht.l_off, sht.m_off), tuple(shard.shape), float(loss), grad.clone(),
                      sums.clone(), handler.spectral_obj.last_degree_sums.clone())))
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


@pytest.mark.parametrize("hsize,wsize", [(2, 1), (4, 1), (1, 2), (2, 2)])
def test_sharded_spectral_crps_equals_the_unsharded_one_without_a_gather(hsize, wsize):
    from makani_amd.distributed import compute_split_shapes
    from makani_amd.losses import LossHandler
    results = _run(hsize * wsize, hsize, wsize)
    handler = LossHandler(_params()).train()
    assert not handler.do_gather_input and not handler.spectral_obj.sharded
    cp, ct = _spectra()
    whole = cp.clone().requires_grad_(True)
    want_loss, want_grad, want_sums = _run_handler(handler, whole, ct, H, W)
    want_loss, want_grad = float(want_loss), want_grad.numpy()
    # the float64 bound of the [B, C, 2] sums: the per-degree bounds added over the degrees (degree weights one), times the
    # scale, once for the whole and once for the shards, plus one rounding per addition over the degrees and per all-reduce addition
    ref = sc.sums(cp.numpy(), ct.numpy(), DIMS)
    scale = handler.spectral_obj.scale
    lim = 2 * scale * sc.bound(ref, DIMS).sum(axis=1).reshape(B, C, 2) + (L + hsize * wsize) * sc.U * np.abs(want_sums.numpy())
    chw = (handler.channel_weights * handler.multistep_weight).reshape(C).double().numpy()
    loss_lim = float((np.abs(chw).reshape(1, C) * (lim[..., 0] + 0.5 * handler.spectral_obj.kappa * lim[..., 1])).sum())
    loss_lim += float(np.spacing(np.float32(abs(want_loss))))          # the loss is rounded to fp32 once
    ls, ms = compute_split_shapes(L, hsize), compute_split_shapes(M, wsize)
    assert sorted(w for w, *_ in results.values()) == [(i, j) for i in range(hsize) for j in range(wsize)]
    degree_sums = torch.zeros(B, C, L, 2, dtype=torch.float64)
    for r, ((i, j), (l_off, m_off), shape, loss, grad, sums, last) in results.items():
        assert (l_off, m_off) == (sum(ls[:i]), sum(ms[:j])) and shape == (ls[i], ms[j], B * E * C), r
        assert sums.dtype == torch.float64 and tuple(sums.shape) == (B, C, 2), r
        assert (np.abs(sums.numpy() - want_sums.numpy()) <= lim).all(), r
        assert abs(loss - want_loss) <= loss_lim, (r, loss, want_loss)
        piece = want_grad[l_off:l_off + ls[i], m_off:m_off + ms[j]]
        stored = sc.stored_mask(ls[i], ms[j], l_off, m_off)
        assert (grad.numpy()[~stored] == 0).all(), r                   # exact zeros in the unstored triangle (it holds NaN)
        rows = stored.any(axis=1)
        if rows.any():
            assert row_rel(grad.numpy()[rows].reshape(int(rows.sum()), -1), piece[rows].reshape(int(rows.sum()), -1)).max() <= 1e-5, r
        degree_sums[:, :, l_off:l_off + ls[i]] += last                 # partial sums of the rank's degrees and orders
    assert torch.allclose(degree_sums, handler.spectral_obj.last_degree_sums, rtol=1e-13, atol=0)
