"""gloo tests (CPU) of ``EnsembleScores`` under spatial and data parallelism: every rank feeds its own h shard of uneven
33 x 60 fields (and its own batch under data parallelism).  The ``[B, C, 4]`` sums are all-reduced over the spatial group
per update and must reproduce the unsharded numpy sums within the bound; the rank counts are reduced in ``finalize`` and
must be equal.  The spawn pattern of test_lploss_dist_cpu.py."""
import os
import socket
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import ens_checks as ec

H, W, B, C, E, STEPS = 33, 60, 2, 3, 5, 2


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _params():
    return SimpleNamespace(valid_autoreg_steps=STEPS - 1, N_out_channels=C, img_shape_x=H, img_shape_y=W, img_crop_shape_x=H,
                           img_crop_shape_y=W, img_crop_offset_x=0, img_crop_offset_y=0, model_grid_type="equiangular",
                           split_data_channels=False)


def _problem(data_rank):
    return ec.problem((B, E, C, H, W), seed=40 + data_rank)


def _worker(rank, world, port, hsize, wsize, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank))
        torch.set_num_threads(1)
        from makani_amd import comm
        from makani_amd.distributed import split_tensor_along_dim
        from makani_amd.ensemble import EnsembleScores
        comm.init(model_parallel_sizes=[hsize, wsize, 1, 1], backend="gloo")
        where = (comm.get_rank("data"), comm.get_rank("h"), comm.get_rank("w"))
        ens, tar, _ = _problem(where[0])

        def shard(x):
            x = split_tensor_along_dim(torch.from_numpy(np.array(x)), -2, comm.get_size("h"))[comm.get_rank("h")]
            return split_tensor_along_dim(x, -1, comm.get_size("w"))[comm.get_rank("w")].contiguous()

        sc = EnsembleScores(_params(), E, "cpu")
        sc.update(shard(ens), shard(tar), 1)
        local_ranks = sc.rank_histogram.clone()
        out = sc.finalize()
        dist.barrier()
        q.put((rank, (where, sc.last_sums.numpy(), local_ranks.numpy(), {k: v.numpy() for k, v in out.items()})))
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


@pytest.mark.parametrize("hsize,wsize,data", [(2, 1, 1), (2, 1, 2)])
def test_sharded_scores_equal_the_unsharded_ones(hsize, wsize, data):
    from makani_amd.ensemble import EnsembleScores
    results = _run(hsize * wsize * data, hsize, wsize)
    assert sorted(w for w, _, _, _ in results.values()) == [(d, i, j) for d in range(data) for i in range(hsize) for j in range(wsize)]
    wrow = EnsembleScores(_params(), E, "cpu").wrow.numpy()          # unsharded: the whole [H]
    assert wrow.shape == (H,)
    whole_ranks = sum(ec.ranks_skipped(*_problem(d)[:2])[0] for d in range(data))
    tot = np.zeros((C, 4))
    for d in range(data):
        s = ec.sums(*_problem(d)[:2], wrow)
        tot += np.concatenate([s[..., :2], np.sqrt(s[..., 2:])], axis=-1).sum(axis=0)
    mean = tot / (B * data)
    for r, ((d, i, j), last, local_ranks, out) in results.items():
        ens, tar, _ = _problem(d)
        ec.assert_sums(last, ens, tar, wrow, f"rank {r}")
        assert local_ranks[0].sum() == 0 and 0 < local_ranks[1].sum() < B * C * H * W       # its own shard only
        assert np.array_equal(out["rank_histogram"][1], whole_ranks) and not out["rank_histogram"][0].any()
        assert not out["skipped"].any()
        assert np.allclose(out["crps"][1], mean[:, 0] - mean[:, 1] / 2, rtol=1e-11, atol=0)
        assert np.allclose(out["spread"][1], mean[:, 3], rtol=1e-11, atol=0)
        assert np.allclose(out["ens_mean_rmse"][1], mean[:, 2], rtol=1e-11, atol=0)
        assert np.isnan(out["crps"][0]).all()
