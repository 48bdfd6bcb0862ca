"""GPU tests of csrc/ens.hip through the C ABI (guarded outputs, poisoned inputs, inputs one element past their alignment), of
``ops.ensemble_sums`` on the device and of ``EnsembleRollout`` on a small SFNO.  The sums are held to the derived bound of
tests/ens_checks.py against the numpy pairwise restatement (which the CPU tests hold the torch formulation to first); the
counts are integers and compared with ``np.array_equal``.  The inputs lie between NaN bands, so a read past either end shows
up as a skipped point and a NaN sum."""
import functools

import numpy as np
import pytest
import torch

import ens_checks as ec
from kernel_checks import guarded, poisoned

pytestmark = pytest.mark.gpu

# (B, E, C, H, W): one point; odd sizes; P = 8, 16, 32, 64 with and without pads; two slabs and several tiles (17 x 20, 33 x 64);
# a row longer than a tile at P = 64 (1441); samples whose alignments disagree (C H W = 27)
SHAPES = [(1, 2, 1, 1, 1), (2, 3, 2, 3, 5), (1, 5, 3, 5, 8), (2, 8, 2, 17, 20), (1, 16, 3, 33, 64), (1, 17, 2, 5, 33), (1, 33, 1, 3, 9),
          (1, 63, 1, 3, 9), (1, 64, 1, 2, 1441), (4, 4, 1, 3, 9)]
DTYPES = ["float32", "bfloat16"]
FILL = -77          # what the guard bands of the integer outputs hold
ids = lambda s: "x".join(map(str, s))


@functools.lru_cache(maxsize=None)
def reference(shape, dtype):
    """numpy ``(ranks, skipped)`` of the shared problem, computed once."""
    ens, tar, _ = ec.problem(shape, dtype)
    return ec.ranks_skipped(ens, tar)


def _device_members(ens, dtype, dev, offset, gap):
    """The members on the device as ``dtype``: between NaN bands; ``offset``: one element past a 16-byte boundary;
    ``gap``: that many NaN elements behind every member's block.  Returns (tensor to keep, pointer, bstride, estride)."""
    B, E = ens.shape[:2]
    chw = int(np.prod(ens.shape[2:]))
    t = torch.from_numpy(np.array(ens)).to(getattr(torch, dtype)).reshape(B, E, chw)
    if gap:
        t = torch.cat([t, torch.full((B, E, gap), float("nan"), dtype=t.dtype)], dim=2)
    flat = t.reshape(-1)
    if offset:
        flat = torch.cat([torch.full((1,), float("nan"), dtype=t.dtype), flat])
    d = poisoned(flat, dev)
    d = d[1:] if offset else d
    assert d.data_ptr() % 16 == (d.element_size() if offset else 0)
    return d, d.data_ptr(), E * (chw + gap), chw + gap


def launch(dev, ens, tar, wrow, dtype="float32", ranks_start=None, skipped_start=None, offset=False, gap=0, with_counts=True):
    """One call of mk_ens_sums on numpy inputs; returns numpy (sums, ranks, skipped) after checking every guard band."""
    from makani_amd import _lib
    lib = _lib.load()
    B, E, C, H, W = ens.shape
    keep, eptr, bstride, estride = _device_members(ens, dtype, dev, offset, gap)
    td = poisoned(torch.from_numpy(np.array(tar)), dev)
    wd = poisoned(torch.from_numpy(np.array(wrow)), dev)
    sums, s_check = guarded((B, C, 4), torch.float64, dev)
    ws, w_check = guarded((lib.mk_ens_workspace(B, C, H),), torch.float64, dev)
    ranks, r_check = guarded((C, E + 1), torch.int64, dev, fill=FILL)
    skipped, k_check = guarded((C,), torch.int64, dev, fill=FILL)
    ranks.copy_(torch.from_numpy(ranks_start)) if ranks_start is not None else ranks.zero_()
    skipped.copy_(torch.from_numpy(skipped_start)) if skipped_start is not None else skipped.zero_()
    rc = lib.mk_ens_sums(eptr, 0 if dtype == "float32" else 1, bstride, estride, td.data_ptr(), wd.data_ptr(), ws.data_ptr(),
                         sums.data_ptr(), ranks.data_ptr() if with_counts else None, skipped.data_ptr() if with_counts else None,
                         B, E, C, H, W, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "mk_ens_sums")
    torch.cuda.synchronize()
    for check, what in ((s_check, "sums"), (w_check, "workspace"), (r_check, "ranks"), (k_check, "skipped")):
        check(what)
    return sums.cpu().numpy(), ranks.cpu().numpy(), skipped.cpu().numpy()


@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "shifted"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_sums_within_the_bound_and_counts_equal_numpy(dev, shape, dtype, offset):
    ens, tar, wrow = ec.problem(shape, dtype)
    got, ranks, skipped = launch(dev, ens, tar, wrow, dtype, offset=offset)
    want_ranks, want_skipped = reference(shape, dtype)
    assert np.array_equal(skipped, want_skipped) and not skipped.any(), "a read outside the members' points?"
    assert np.array_equal(ranks, want_ranks)
    ec.assert_sums(got, ens, tar, wrow, f"{ids(shape)} {dtype}")
    B, E, C, H, W = shape
    assert (ranks.sum(axis=1) == B * H * W).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_counts_are_added_to_and_runs_repeat(dev, dtype):
    shape = (2, 8, 2, 17, 20)
    ens, tar, wrow = ec.problem(shape, dtype)
    want_ranks, _ = reference(shape, dtype)
    rng = np.random.default_rng(3)
    start = rng.integers(2 ** 32, 2 ** 40, size=want_ranks.shape, dtype=np.int64)
    kstart = rng.integers(2 ** 32, 2 ** 40, size=(2,), dtype=np.int64)
    one, ranks, skipped = launch(dev, ens, tar, wrow, dtype, start, kstart)
    assert np.array_equal(ranks, start + want_ranks) and np.array_equal(skipped, kstart)
    two, ranks2, skipped2 = launch(dev, ens, tar, wrow, dtype, start, kstart)               # a second identical run: the same bits
    assert np.array_equal(one.view(np.int64), two.view(np.int64)) and np.array_equal(ranks2, ranks) and np.array_equal(skipped2, skipped)
    none, untouched, untouched_k = launch(dev, ens, tar, wrow, dtype, with_counts=False)    # NULL: nothing is written there
    assert np.array_equal(none.view(np.int64), one.view(np.int64)) and not untouched.any() and not untouched_k.any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 3, 2, 3, 5), (1, 16, 3, 33, 64), (1, 64, 1, 2, 1441)], ids=ids)
def test_member_stride_with_nan_in_the_gaps(dev, shape, dtype):
    """Every member's block is followed by five NaN elements (so the members' alignments disagree too): nothing reads them."""
    ens, tar, wrow = ec.problem(shape, dtype)
    got, ranks, skipped = launch(dev, ens, tar, wrow, dtype, gap=5)
    assert not skipped.any() and np.array_equal(ranks, reference(shape, dtype)[0])
    ec.assert_sums(got, ens, tar, wrow, f"gaps {ids(shape)} {dtype}")


@pytest.mark.parametrize("E", [4, 5, 33])
def test_ties_with_the_target_count_as_not_less(dev, E):
    rng = np.random.default_rng(E)
    ens = rng.integers(-2, 3, size=(2, E, 2, 5, 33)).astype(np.float32)
    tar = rng.integers(-2, 3, size=(2, 2, 5, 33)).astype(np.float32)
    wrow = np.linspace(0.5, 1.0, 5, dtype=np.float32)
    assert (ens == tar[:, None]).any(axis=1).mean() >= 0.25          # the premise: at least a quarter of the points tie
    for dtype in DTYPES:                                            # small integers are bf16 values
        got, ranks, skipped = launch(dev, ens, tar, wrow, dtype)
        assert np.array_equal(ranks, ec.ranks_skipped(ens, tar)[0]) and not skipped.any()
        ec.assert_sums(got, ens, tar, wrow, f"ties E={E} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 5, 3, 5, 8), (2, 16, 3, 33, 64), (2, 64, 3, 3, 9)], ids=ids)
def test_nan_in_a_member_in_the_target_and_in_both(dev, shape, dtype):
    ens, tar, wrow = (np.array(a) for a in ec.problem(shape, dtype))
    B, E, C, H, W = shape
    ens[0, E - 1, 1, H - 1, W - 1] = np.nan          # a member: the largest index of its block
    ens[0, 0, 1, 0, 0] = np.nan                      # and another point of the same field
    tar[1, 2, H // 2, 3] = np.nan                    # the target
    ens[1, E // 2, 0, 0, 1] = tar[1, 0, 0, 1] = np.nan      # both
    got, ranks, skipped = launch(dev, ens, tar, wrow, dtype)
    want_ranks, want_skipped = ec.ranks_skipped(ens, tar)
    assert skipped.tolist() == [1, 2, 1] and np.array_equal(skipped, want_skipped)
    assert np.array_equal(ranks, want_ranks)
    ec.assert_sums(got, ens, tar, wrow, f"NaN {ids(shape)} {dtype}")        # NaN exactly where numpy's are, the others in bound
    assert np.isnan(got).all(axis=-1).tolist() == [[False, True, False], [True, False, True]]


@pytest.mark.parametrize("shape", [(1, 16, 3, 33, 64), (2, 8, 2, 17, 20)], ids=ids)
def test_row_shards_add_up_to_the_whole(dev, shape):
    ens, tar, wrow = ec.problem(shape)
    full, ranks, _ = launch(dev, ens, tar, wrow)
    H = shape[3]
    parts = [launch(dev, np.ascontiguousarray(ens[..., a:b, :]), np.ascontiguousarray(tar[..., a:b, :]), wrow[a:b])
             for a, b in ((0, H // 2 + 1), (H // 2 + 1, H))]
    assert np.array_equal(parts[0][1] + parts[1][1], ranks) and np.array_equal(ranks, reference(shape, "float32")[0])
    lim = ec.bound(ens, tar, wrow)
    assert (np.abs(parts[0][0] + parts[1][0] - full) <= 2 * lim).all()      # each side is within the bound of the reference


def test_member_offsets_beyond_2_31(dev):
    """Two bf16 members 2^31 + 24 elements apart in one 4.3 GB allocation that is never filled: only the two blocks, the NaN
    elements around them and the target are written, and the second member's offset needs 64 bits."""
    from makani_amd import _lib
    lib = _lib.load()
    shape = (1, 2, 2, 17, 20)
    ens, tar, wrow = ec.problem(shape, "bfloat16")
    B, E, C, H, W = shape
    chw, estride = C * H * W, 2 ** 31 + 24
    buf = torch.empty(estride + chw + 16, dtype=torch.bfloat16, device=dev)
    for e in range(E):
        lo = e * estride
        buf[max(lo - 16, 0):lo + chw + 16] = float("nan")
        buf[lo:lo + chw] = torch.from_numpy(np.array(ens[0, e])).to(torch.bfloat16).reshape(-1).to(dev)
    td, wd = poisoned(torch.from_numpy(np.array(tar)), dev), poisoned(torch.from_numpy(np.array(wrow)), dev)
    sums, s_check = guarded((B, C, 4), torch.float64, dev)
    ws = torch.empty(lib.mk_ens_workspace(B, C, H), dtype=torch.float64, device=dev)
    ranks = torch.zeros(C, E + 1, dtype=torch.int64, device=dev)
    skipped = torch.zeros(C, dtype=torch.int64, device=dev)
    _lib.check(lib.mk_ens_sums(buf.data_ptr(), 1, E * estride, estride, td.data_ptr(), wd.data_ptr(), ws.data_ptr(), sums.data_ptr(),
                               ranks.data_ptr(), skipped.data_ptr(), B, E, C, H, W, torch.cuda.current_stream().cuda_stream),
               "mk_ens_sums")
    torch.cuda.synchronize()
    s_check("sums")
    assert not skipped.any().item() and np.array_equal(ranks.cpu().numpy(), reference(shape, "bfloat16")[0])
    ec.assert_sums(sums.cpu().numpy(), ens, tar, wrow, "2^31")


# ---------------------------------------------------------------------------- the op, the handler and the rollout on the device
def _on(dev, shape, dtype="float32"):
    ens, tar, wrow = ec.problem(shape, dtype)
    return (torch.from_numpy(np.array(ens)).to(dev, getattr(torch, dtype)), torch.from_numpy(np.array(tar)).to(dev),
            torch.from_numpy(np.array(wrow)).to(dev))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 5, 3, 5, 8), (1, 16, 3, 33, 64), (2, 70, 1, 3, 9)], ids=ids)
def test_torch_formulation_on_the_device_agrees_with_hip(dev, monkeypatch, shape, dtype):
    """``MK_ENSEMBLE=torch`` on device tensors against ``hip``: both within the bound of numpy, the counts equal.  E = 70 takes
    the torch formulation under either."""
    from makani_amd import ops
    B, E, C, H, W = shape
    ens, tar, wrow = _on(dev, shape, dtype)
    out = {}
    for mode in ("hip", "torch"):
        monkeypatch.setenv("MK_ENSEMBLE", mode)
        ranks = torch.zeros(C, E + 1, dtype=torch.int64, device=dev)
        skipped = torch.zeros(C, dtype=torch.int64, device=dev)
        flat = ens.reshape(B * E, C, H, W) if mode == "hip" else ens          # the model's [B * E, C, H, W] output is read in place
        s = ops.ensemble_sums(flat, tar, wrow, ranks, skipped)
        out[mode] = (s.cpu().numpy(), ranks.cpu().numpy(), skipped.cpu().numpy())
        ec.assert_sums(out[mode][0], *ec.problem(shape, dtype), f"{mode} {ids(shape)} {dtype}")
    assert np.array_equal(out["hip"][1], out["torch"][1]) and np.array_equal(out["hip"][1], reference(shape, dtype)[0])
    assert not out["hip"][2].any() and not out["torch"][2].any()
    if E > 64:
        assert np.array_equal(out["hip"][0], out["torch"][0])


def test_a_captured_update_replays_to_the_eager_result(dev, tmp_path, monkeypatch):
    from makani_amd.ensemble import EnsembleScores
    from test_ens_dist_cpu import _params
    monkeypatch.setenv("MK_ENSEMBLE", "hip")
    B, E, C, H, W = 2, 5, 3, 33, 60
    first, second = _on(dev, (B, E, C, H, W)), _on(dev, (B, E, C, H, W), "bfloat16")
    eager = EnsembleScores(_params(), E, dev)
    eager.update(first[0], first[1], 0)
    eager.update(second[0].float(), second[1], 0)
    sc = EnsembleScores(_params(), E, dev)
    sc.update(first[0], first[1], 0)                 # also the warm-up
    ens, tar = second[0].float().clone(), second[1].clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sc.update(ens, tar, 0)
    graph.replay()
    torch.cuda.synchronize()
    for name in ("sums", "counter", "rank_histogram", "skipped"):
        assert torch.equal(getattr(sc, name), getattr(eager, name)), name
    assert float(sc.counter[0]) == 2 * B and int(sc.rank_histogram[0].sum()) == 2 * B * C * H * W
    ec.assert_sums(sc.last_sums.cpu().numpy(), second[0].float().cpu().numpy(), second[1].cpu().numpy(), sc.wrow.cpu().numpy(), "replay")


def test_ensemble_rollout_of_the_package_sfno_captured_equals_eager(dev, tmp_path, monkeypatch):
    """Two steps of E = 4 members of a small package SFNO under bf16 autocast, with ``capture`` off and on: the curves, the
    counts and the emitted fields are equal, and the scoring pass is the HIP one."""
    from makani_amd import _lib
    from makani_amd.ensemble import EnsembleScores
    from makani_amd.inference import EnsembleRollout
    from test_rollout_cpu import C as CR, build, make_params, make_problem
    from test_stepper_gpu import _sfno
    monkeypatch.setenv("MK_ROLLOUT", "hip")
    monkeypatch.setenv("MK_ENSEMBLE", "hip")
    H, W, B, steps, T, E = 64, 128, 2, 2, 2, 4
    params = make_params(H, W, tmp_path, steps=steps, n_history=T - 1, masked_channels=[1])
    params.noise_std = 0.1
    prob = make_problem(B, T, H, W, steps, seed=4)
    lib, calls = _lib.load(), []

    class Counted:
        def __getattr__(self, name):
            if name == "mk_ens_sums":
                return lambda *a: calls.append(torch.cuda.is_current_stream_capturing()) or lib.mk_ens_sums(*a)
            return getattr(lib, name)

    monkeypatch.setattr(_lib, "load", lambda: Counted())
    res = {}
    for capture in (False, True):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            wrap, _, _ = build(params, prob, dev, model=_sfno(dev, T * (CR + 1) + 3, CR, H, W))
            sc = EnsembleScores(params, E, dev)
            ro = EnsembleRollout(params, wrap, sc, E, capture=capture)
            out = ro.run(prob.inp.to(dev), prob.tar.to(dev), generator=torch.Generator(device=dev).manual_seed(7), output_channels=[0, 2])
        assert out.shape == (steps, B, E, 2, H, W)
        res[capture] = (out, sc.finalize(), sc)
    assert calls == [False] * (2 * steps)            # every scoring launch is eager, behind the step (or its replay)
    assert torch.equal(res[True][0], res[False][0]) and not torch.equal(res[True][0][:, :, 0], res[True][0][:, :, 1])
    for k, v in res[False][1].items():
        assert torch.equal(res[True][1][k], v), k
    fin = res[False][1]
    assert int(fin["rank_histogram"].sum()) == steps * B * CR * H * W and not fin["skipped"].any()
    assert bool((fin["crps"] > 0).all()) and bool((fin["spread"] > 0).all()) and bool(torch.isfinite(fin["spread_skill"]).all())
