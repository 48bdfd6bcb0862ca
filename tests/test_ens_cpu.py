"""CPU tests of the ensemble scores: the checker itself (pairwise against sorted against the integral), ``ops.ensemble_sums``
on CPU tensors (the torch float64 formulation, which the bound is shown to hold for before any kernel is held to it),
``EnsembleScores`` against numpy, and ``EnsembleRollout`` against the same loop written by hand."""
import math

import numpy as np
import pytest
import torch

import capi_checks as capi
import ens_checks as ec

from test_rollout_cpu import C, build, make_params, make_problem


def run_op(ens, tar, wrow, ranks_start=None, with_counts=True, flat=False):
    from makani_amd import ops
    B, E, Cn, H, W = ens.shape
    e = torch.from_numpy(np.array(ens))
    ranks = torch.zeros(Cn, E + 1, dtype=torch.int64) if ranks_start is None else torch.from_numpy(ranks_start.copy())
    skipped = torch.zeros(Cn, dtype=torch.int64)
    out = ops.ensemble_sums(e.reshape(B * E, Cn, H, W) if flat else e, torch.from_numpy(np.array(tar)), torch.from_numpy(np.array(wrow)),
                            ranks if with_counts else None, skipped if with_counts else None)
    assert out.shape == (B, Cn, 4) and out.dtype == torch.float64 and len(ops.ENSEMBLE_SUMS) == 4
    return out.numpy(), ranks.numpy(), skipped.numpy()


# ---------------------------------------------------------------------------------------------------------------------
# the checker is checked
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [2, 3, 5, 8, 17])
def test_pairwise_sorted_and_integral_forms_agree(E):
    ens, tar, _ = ec.problem((1, E, 3, 4, 6))
    a, g, q, v = ec.point_values(ens, tar)
    gs = ec.sorted_g(ens)
    scale = np.abs(ens).max(axis=1) + np.abs(tar)
    assert (np.abs(g - gs) <= 1e-15 * E * scale).all()
    x, y = ens.astype(np.float64), tar.astype(np.float64)
    for idx in np.ndindex(tar.shape):
        b, c, h, w = idx
        want = ec.crps_integral(x[b, :, c, h, w], y[idx])
        assert abs((a[idx] - 0.5 * g[idx]) - want) <= 1e-14 * E * scale[idx], (E, idx)
    assert np.allclose(v, x.var(axis=1, ddof=1), rtol=1e-12, atol=0) and np.allclose(q, (x.mean(axis=1) - y) ** 2, rtol=1e-9, atol=1e-30)


def test_checker_counts_ties_as_not_less_and_skips_nan():
    ens = np.array([1.0, 2.0, 2.0, 3.0], dtype=np.float32).reshape(1, 4, 1, 1, 1).repeat(3, axis=-1)
    tar = np.array([2.0, 0.0, np.nan], dtype=np.float32).reshape(1, 1, 1, 3)
    ranks, skipped = ec.ranks_skipped(ens, tar)
    assert ranks.tolist() == [[1, 1, 0, 0, 0]] and skipped.tolist() == [1]
    assert np.isnan(ec.sums(ens, tar, np.ones(1, dtype=np.float32))).all()


# ---------------------------------------------------------------------------------------------------------------------
# ops.ensemble_sums on CPU tensors
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("E", [1, 2, 5, 70])
def test_cpu_formulation_is_within_the_bound_of_the_pairwise_reference(E, dtype):
    shape = (2, E, 3, 5, 8)
    ens, tar, wrow = ec.problem(shape, dtype)
    got, ranks, skipped = run_op(ens, tar, wrow)
    names = (0, 1, 2) if E == 1 else (0, 1, 2, 3)
    ec.assert_sums(got, ens, tar, wrow, f"E={E} {dtype}", names)
    if E == 1:
        assert np.isnan(got[..., 3]).all() and (got[..., 1] == 0).all()
    want_ranks, want_skipped = ec.ranks_skipped(ens, tar)
    assert np.array_equal(ranks, want_ranks) and np.array_equal(skipped, want_skipped) and not skipped.any()
    assert (ranks.sum(axis=1) == 2 * 5 * 8).all()
    # the flattened [B * E, C, H, W] model output is viewed, counts are added to, None switches them off
    start = np.arange(3 * (E + 1), dtype=np.int64).reshape(3, E + 1) + 2 ** 33
    flat, ranks2, _ = run_op(ens, tar, wrow, ranks_start=start, flat=True)
    assert np.array_equal(flat, got, equal_nan=True) and np.array_equal(ranks2, start + want_ranks)
    assert np.array_equal(run_op(ens, tar, wrow, with_counts=False)[0], got, equal_nan=True)


@pytest.mark.parametrize("E", [2, 5, 70])
def test_nan_rules_on_cpu(E):
    ens, tar, wrow = (np.array(a) for a in ec.problem((2, E, 3, 5, 8)))
    ens[0, E - 1, 1, 2, 3] = np.nan          # a member
    tar[1, 2, 4, 7] = np.nan                 # the target
    ens[1, 0, 0, 0, 0] = tar[1, 0, 0, 0] = np.nan      # both
    got, ranks, skipped = run_op(ens, tar, wrow)
    ec.assert_sums(got, ens, tar, wrow, f"NaN E={E}")
    nan = np.isnan(got).all(axis=-1)
    assert nan.tolist() == [[False, True, False], [True, False, True]] and not np.isnan(got[~nan]).any()
    want_ranks, want_skipped = ec.ranks_skipped(ens, tar)
    assert skipped.tolist() == [1, 1, 1] and np.array_equal(skipped, want_skipped) and np.array_equal(ranks, want_ranks)
    assert (ranks.sum(axis=1) == 2 * 5 * 8 - 1).all()


def test_ties_with_the_target_count_as_not_less():
    rng = np.random.default_rng(4)
    ens = rng.integers(-2, 3, size=(2, 5, 2, 5, 8)).astype(np.float32)
    tar = rng.integers(-2, 3, size=(2, 2, 5, 8)).astype(np.float32)
    wrow = np.linspace(0.5, 1.0, 5, dtype=np.float32)
    assert (ens == tar[:, None]).any(axis=1).mean() >= 0.25
    got, ranks, skipped = run_op(ens, tar, wrow)
    ec.assert_sums(got, ens, tar, wrow, "ties")
    assert np.array_equal(ranks, ec.ranks_skipped(ens, tar)[0]) and not skipped.any()


@pytest.mark.parametrize("E", [2, 3, 7])
def test_identical_members_reduce_to_the_deterministic_sums(E):
    from makani_amd import ops
    ens1, tar, wrow = ec.problem((2, 1, 3, 5, 8))
    ens = np.repeat(ens1, E, axis=1)
    got, ranks, _ = run_op(ens, tar, wrow)
    det = ops.geo_metric_sums(torch.from_numpy(np.array(ens1[:, 0])), torch.from_numpy(np.array(tar)), None,
                              torch.from_numpy(np.array(wrow))).numpy()
    lim = ec.bound(ens, tar, wrow)
    assert (np.abs(got[..., 0] - det[..., 0]) <= lim[..., 0]).all() and (np.abs(got[..., 2] - det[..., 1]) <= lim[..., 2]).all()
    assert (got[..., 1] == 0).all() and (got[..., 3] == 0).all()
    assert (ranks[:, 1:E] == 0).all() and (ranks[:, 0] + ranks[:, E] == 2 * 5 * 8).all()


def test_ensemble_sums_rejects_bad_arguments_and_reads_its_knob(monkeypatch):
    from makani_amd import ops
    ens, tar, wrow = (torch.from_numpy(np.array(a)) for a in ec.problem((2, 3, 2, 5, 8)))
    for args, needle in (((ens[:, :, :1], tar, wrow), "must be"), ((ens, tar[0], wrow), "target must be"),
                         ((ens, tar, wrow[:-1]), "4 weights for 5"), ((ens.reshape(6, 2, 5, 8)[:5], tar, wrow), "must be"),
                         ((ens, tar, wrow, torch.zeros(2, 3, dtype=torch.int64)), "ranks"),
                         ((ens, tar, wrow, torch.zeros(2, 4, dtype=torch.int32)), "ranks"),
                         ((ens, tar, wrow, None, torch.zeros(3, dtype=torch.int64)), "skipped")):
        with pytest.raises(ValueError, match=needle):
            ops.ensemble_sums(*args)
    a = ops.ensemble_sums(ens, tar, wrow)
    for mode in ("hip", "torch"):                               # CPU tensors take the torch formulation under either
        monkeypatch.setenv("MK_ENSEMBLE", mode)
        assert torch.equal(ops.ensemble_sums(ens, tar, wrow), a)
    monkeypatch.setenv("MK_ENSEMBLE", "fast")
    with pytest.raises(ValueError, match="MK_ENSEMBLE"):
        ops.ensemble_sums(ens, tar, wrow)
    monkeypatch.delenv("MK_ENSEMBLE")
    assert ops.ensemble_sums(ens.requires_grad_(True), tar, wrow).requires_grad is False


# ---------------------------------------------------------------------------------------------------------------------
# the handler
# ---------------------------------------------------------------------------------------------------------------------
def test_scores_finalize_equals_numpy(tmp_path):
    from makani_amd.ensemble import EnsembleScores
    from makani_amd.metric import MetricsHandler
    H, W, E, steps = 12, 24, 5, 3
    params = make_params(H, W, tmp_path, steps=steps)
    sc = EnsembleScores(params, E, "cpu")
    mh = MetricsHandler(params, torch.ones(C), torch.zeros(C, H, W), torch.device("cpu"))
    assert torch.equal(sc.wrow, mh.wrow) and abs(float(sc.wrow.double().sum()) * W - 1.0) < 1e-6
    wrow = sc.wrow.numpy()
    batches = [ec.problem((2, E, C, H, W), seed=s) for s in (1, 2)]
    tot = np.zeros((steps, C, 4))
    ranks = np.zeros((steps, C, E + 1), dtype=np.int64)
    for idt in (0, 2):                       # lead time 1 gets no update
        for k, (ens, tar, _) in enumerate(batches):
            if idt == 2 and k == 1:
                continue
            sc.update(torch.from_numpy(np.array(ens)), torch.from_numpy(np.array(tar)), idt)
            s = ec.sums(ens, tar, wrow)
            tot[idt, :, :2] += s[..., :2].sum(axis=0)
            tot[idt, :, 2:] += np.sqrt(s[..., 2:]).sum(axis=0)
            ranks[idt] += ec.ranks_skipped(ens, tar)[0]
    stds = np.array([2.0, 0.5, 3.0])
    for given in (None, stds):
        out = sc.finalize(stds=given)
        scale = 1.0 if given is None else stds[None, :]
        n = np.array([4.0, np.nan, 2.0]).reshape(-1, 1)
        A, G, R, S = (tot[..., k] / n for k in range(4))
        want = {"crps": (A - G / 2) * scale, "fair_crps": (A - G * E / (2 * (E - 1))) * scale, "ens_mean_rmse": R * scale,
                "spread": S * scale, "spread_skill": math.sqrt((E + 1) / E) * S / R}
        for k, w in want.items():
            assert out[k].shape == (steps, C) and out[k].dtype == torch.float64
            assert np.allclose(out[k].numpy(), w, rtol=1e-12, atol=0, equal_nan=True), k
            assert np.isnan(out[k][1].numpy()).all() and not np.isnan(out[k][[0, 2]].numpy()).any()
        assert np.array_equal(out["rank_histogram"].numpy(), ranks) and out["rank_histogram"].dtype == torch.int64
        assert not out["skipped"].any() and tuple(out["skipped"].shape) == (steps, C)
    assert (out["crps"][0] > 0).all() and (out["fair_crps"][0] < out["crps"][0]).all()
    sc.zero_buffers()
    assert not sc.sums.any() and not sc.rank_histogram.any() and not sc.counter.any()
    with pytest.raises(ValueError, match="members"):
        sc.update(torch.zeros(2, E + 1, C, H, W), torch.zeros(2, C, H, W), 0)


# ---------------------------------------------------------------------------------------------------------------------
# the rollout
# ---------------------------------------------------------------------------------------------------------------------
def handwritten(params, prob, E, noise_std, seed, steps):
    """The ensemble loop written out with the step wrapper itself: repeat, perturb members 1 ... E - 1, step, score."""
    from makani_amd.ensemble import EnsembleScores
    wrap, _, _ = build(params, prob)
    pp = wrap.preprocessor
    B = prob.inp.shape[0]
    pp.unpredicted_inp_eval, pp.unpredicted_tar_eval = prob.xz.repeat_interleave(E, dim=0), prob.yz.repeat_interleave(E, dim=0)
    sc = EnsembleScores(params, E, "cpu")
    x = pp.flatten_history(prob.inp).repeat_interleave(E, dim=0)
    g = torch.Generator().manual_seed(seed)
    noise = torch.randn((B, E - 1) + tuple(x.shape[1:]), generator=g)
    xv = x.view((B, E) + tuple(x.shape[1:]))
    control = xv[:, 0].clone()
    xv[:, 1:] += noise_std * noise
    assert torch.equal(xv[:, 0], control) and not torch.equal(xv[:, 1], control)
    preds = []
    with torch.no_grad():
        for idt in range(steps):
            pred = wrap(x).float()
            sc.update(pred.view((B, E) + tuple(pred.shape[1:])), prob.tar[:, idt], idt)
            preds.append(pred.view((B, E) + tuple(pred.shape[1:])))
            x = pp.append_history(x, pred, idt)
    return torch.stack(preds), sc


@pytest.mark.parametrize("nh", [0, 1])
def test_ensemble_rollout_equals_the_handwritten_loop(tmp_path, nh):
    from makani_amd.ensemble import EnsembleScores
    from makani_amd.inference import EnsembleRollout, Rollout
    H, W, B, steps, E, noise = 12, 24, 2, 3, 4, 0.25
    params = make_params(H, W, tmp_path, steps=steps, n_history=nh, history_normalization_mode="none", masked_channels=[1])
    params.noise_std = noise
    prob = make_problem(B, nh + 1, H, W, steps, seed=3 + nh)
    want, sc0 = handwritten(params, prob, E, noise, seed=11, steps=steps)
    wrap, _, _ = build(params, prob)
    sc1 = EnsembleScores(params, E, "cpu")
    ro = EnsembleRollout(params, wrap, sc1, E)
    assert isinstance(ro, Rollout) and ro.noise_std == noise
    got = ro.run(prob.inp, prob.tar, generator=torch.Generator().manual_seed(11), output_channels=list(range(C)))
    assert got.shape == (steps, B, E, C, H, W) and got.dtype == torch.float32
    assert torch.equal(got, want)
    assert not torch.equal(got[:, :, 0], got[:, :, 1])
    for name in ("sums", "counter", "rank_histogram", "skipped"):
        assert torch.equal(getattr(sc1, name), getattr(sc0, name)), name
    assert sc1.counter.tolist() == [B] * steps and int(sc1.rank_histogram.sum()) == steps * B * C * H * W
    # member 0 is the control: it is the deterministic rollout of the unperturbed initial condition
    wrap, _, _ = build(params, prob)
    det = Rollout(params, wrap).run(prob.inp, steps=steps, output_channels=list(range(C)))
    assert torch.equal(got[:, :, 0], det)
    # noise_std = 0 given explicitly: all members equal the control, and the spread is exactly zero
    wrap, _, _ = build(params, prob)
    sc2 = EnsembleScores(params, E, "cpu")
    same = EnsembleRollout(params, wrap, sc2, E, noise_std=0.0).run(prob.inp, prob.tar, output_channels=[0])
    assert torch.equal(same[:, :, 1], same[:, :, 0]) and float(sc2.finalize()["spread"].abs().max()) == 0.0
    # a free-running ensemble needs no scores
    wrap, _, _ = build(params, prob)
    free = EnsembleRollout(params, wrap, None, E).run(prob.inp, steps=2, generator=torch.Generator().manual_seed(11), output_channels=[2])
    assert torch.equal(free, got[:2, :, :, 2:3])
    with pytest.raises(ValueError, match="members"):
        EnsembleRollout(params, wrap, sc1, E + 1)


def test_matmul_parallel_raises(monkeypatch, tmp_path):
    from makani_amd import comm
    from makani_amd.inference import EnsembleRollout
    params = make_params(12, 24, tmp_path)
    wrap, _, _ = build(params, make_problem(1, 1, 12, 24, 3, seed=0))
    monkeypatch.setattr(comm, "get_size", lambda name: 2 if name == "matmul" else 1)
    with pytest.raises(NotImplementedError):
        EnsembleRollout(params, wrap, None, 2)


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI refuses bad arguments before any launch (tests/capi_checks.py)
# ---------------------------------------------------------------------------------------------------------------------
_A = capi.A
_OK = dict(ens=_A, dtype=0, bstride=3 * 80, estride=80, tar=_A, wrow=_A, ws=_A, sums=_A, ranks=_A, skipped=_A, B=2, E=3, C=2, H=5, W=8)


def _args(**kw):
    return tuple(dict(_OK, **kw).values())


REFUSED = [
    ("mk_ens_sums", _args(ens=_A + 2), "ensemble not aligned to its element"),
    ("mk_ens_sums", _args(tar=_A + 2), "fp32 stream not 4-byte aligned"),
    ("mk_ens_sums", _args(ranks=_A + 4), "64-bit buffer not 8-byte aligned"),
    ("mk_ens_sums", _args(sums=None), "null pointer"),
    ("mk_ens_sums", _args(dtype=2), "dtype must be 0 (fp32) or 1 (bf16)"),
    ("mk_ens_sums", _args(E=1), "E outside 2 ... 64 (the members of a point are sorted in registers)"),
    ("mk_ens_sums", _args(E=65, bstride=65 * 80), "E outside 2 ... 64 (the members of a point are sorted in registers)"),
    ("mk_ens_sums", _args(estride=79), "a member's [C][H][W] block must be contiguous: strides below C * H * W"),
    ("mk_ens_sums", _args(bstride=239), "members of different samples overlap: need bstride >= E * estride or estride >= B * bstride"),
    ("mk_ens_sums", _args(W=0), "bad sizes"),
]


@pytest.mark.parametrize("case", REFUSED, ids=capi.case_ids(REFUSED))
def test_bad_argument_is_refused_before_any_launch(case):
    capi.assert_refused(*case)


def test_workspace_size():
    from makani_amd import _lib
    lib = _lib.load()
    assert lib.mk_ens_workspace(2, 3, 17) == 3 * 2 * 3 * 4 and lib.mk_ens_workspace(1, 1, 8) == 4 and lib.mk_ens_workspace(0, 1, 1) == 0
