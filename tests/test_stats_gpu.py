"""GPU tests of csrc/stats.hip through the C ABI (guarded outputs, poisoned inputs) and of ``DatasetStats`` on it.

Every sum is held to the derived bound of tests/stats_checks.py against the exact sum over the fp32 inputs; the time sum,
min and max are compared bit for bit with the sequential float64 formulation.  The worst ratio of error to bound that was
seen on an MI355X is a record in DESIGN section 35, not a limit."""
import functools

import numpy as np
import pytest
import torch

import stats_checks as sc
from kernel_checks import SENTINEL, guarded, poisoned

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1), (1, 2, 3, 5), (2, 3, 5, 8), (3, 2, 17, 20), (5, 3, 33, 64), (2, 2, 16, 1441)]
FLAGS = [(p, v, w) for p in (False, True) for v in (False, True) for w in (0, 1)]       # prev, pivot, n_wind


@functools.lru_cache(maxsize=None)
def problem(shape):
    """fp32 inputs of one shape, shared by its cases: samples with a per-channel offset, the sample before them, a pivot
    near the data, positive row weights and a non-zero start of the time sum."""
    T, C, H, W = shape
    rng = np.random.default_rng(sum(shape))
    off = (300.0 * np.arange(C)).reshape(1, C, 1, 1)
    x = (rng.standard_normal(shape) + off).astype(np.float32)
    prev = (rng.standard_normal(shape[1:]) + off[0]).astype(np.float32)
    pivot = x[0].mean((-2, -1)).astype(np.float32)
    wrow = ((0.1 + rng.random(H)) / (H * W)).astype(np.float32)
    start = rng.standard_normal(shape[1:]) * 3.0
    return x, prev, pivot, wrow, start


@functools.lru_cache(maxsize=None)
def truth(shape, has_prev, has_pivot):
    x, prev, pivot, wrow, _ = problem(shape)
    return sc.exact_sums(x, prev if has_prev else None, pivot if has_pivot else None, wrow)


@functools.lru_cache(maxsize=None)
def wind_truth(shape):
    x = problem(shape)[0]
    return sc.exact_wind_sums(x, 0, shape[1] - 1)


def shifted(t, dev, fill):
    """``t`` on the device one element past a 16-byte boundary, between NaN bands (inputs) -- the element in front is NaN too."""
    flat = torch.cat([torch.full((1,), fill, dtype=t.dtype), t.reshape(-1)])
    return poisoned(flat, dev)[1:].view(t.shape)


def launch(dev, x, prev, pivot, wrow, start, wind=None, offset=False):
    """One call of mk_field_stats on numpy inputs; returns numpy (sums, minmax, wsums, tsum) after checking every guard band."""
    from makani_amd import _lib
    lib = _lib.load()
    T, C, H, W = x.shape
    put = (lambda a: shifted(torch.from_numpy(a), dev, float("nan"))) if offset else (lambda a: poisoned(torch.from_numpy(a), dev))
    xd = put(x)
    pd = put(prev) if prev is not None else None
    vd = poisoned(torch.from_numpy(pivot), dev) if pivot is not None else None
    wd = poisoned(torch.from_numpy(wrow), dev)
    n_wind = 0 if wind is None else len(wind[0])
    ws, ws_check = guarded((lib.mk_field_stats_workspace(C, H, n_wind),), torch.float64, dev)
    sums, sums_check = guarded((C, 4), torch.float64, dev)
    minmax, mm_check = guarded((C, 2), torch.float32, dev)
    if offset:
        tbuf, ts_check = guarded((C * H * W + 1,), torch.float64, dev)
        tsum = tbuf[1:].view(C, H, W)
    else:
        tsum, ts_check = guarded((C, H, W), torch.float64, dev)
    tsum.copy_(torch.from_numpy(start))
    wu = wv = wsums = None
    w_check = lambda what="": None
    if n_wind:
        wu = torch.tensor(wind[0], dtype=torch.int32, device=dev)
        wv = torch.tensor(wind[1], dtype=torch.int32, device=dev)
        wsums, w_check = guarded((n_wind, 2), torch.float64, dev)
    ptr = lambda t: t.data_ptr() if t is not None else None
    assert xd.data_ptr() % 16 == (4 if offset else 0) and tsum.data_ptr() % 16 == (8 if offset else 0)
    rc = lib.mk_field_stats(xd.data_ptr(), ptr(pd), ptr(vd), wd.data_ptr(), ws.data_ptr(), sums.data_ptr(), minmax.data_ptr(),
                            tsum.data_ptr(), ptr(wu), ptr(wv), n_wind, ptr(wsums), T, C, H, W, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "mk_field_stats")
    torch.cuda.synchronize()
    for chk, what in ((ws_check, "workspace"), (sums_check, "sums"), (mm_check, "minmax"), (ts_check, "tsum"), (w_check, "wsums")):
        chk(what)
    if offset:
        assert float(tbuf[0]) == SENTINEL, "the element in front of the offset tsum was written"
    return (sums.cpu().numpy(), minmax.cpu().numpy(), wsums.cpu().numpy() if n_wind else None, tsum.cpu().numpy())


def check_case(dev, shape, has_prev, has_pivot, n_wind, offset=False):
    x, prev, pivot, wrow, start = problem(shape)
    T, C, H, W = shape
    wind = ([0], [C - 1]) if n_wind else None
    sums, minmax, wsums, tsum = launch(dev, x, prev if has_prev else None, pivot if has_pivot else None, wrow, start, wind, offset)
    worst = 0.0
    for c, rows in enumerate(truth(shape, has_prev, has_pivot)):
        for k, (val, mag, n) in enumerate(rows):
            worst = max(worst, sc.check_sum(sums[c, k], val, mag, n, f"{shape} channel {c} sum {k}"))
    if not has_prev and T == 1:
        assert (sums[:, 2:] == 0).all() and not np.signbit(sums[:, 2:]).any()
    assert np.array_equal(minmax[:, 0], x.min((0, 2, 3))) and np.array_equal(minmax[:, 1], x.max((0, 2, 3)))
    assert np.array_equal(tsum, sc.sequential_time_sum(start, x)), "tsum is not the sequential float64 sum"
    if n_wind:
        for k, (val, mag, n) in enumerate(wind_truth(shape)):
            worst = max(worst, sc.check_sum(wsums[0, k], val, mag, n, f"{shape} wind sum {k}"))
    print(f"stats {shape} prev={has_prev} pivot={has_pivot} wind={n_wind} offset={offset}: worst error / bound {worst:.4f}")
    return worst


@pytest.mark.parametrize("has_prev,has_pivot,n_wind", FLAGS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_field_stats_against_exact_sums(dev, shape, has_prev, has_pivot, n_wind):
    check_case(dev, shape, has_prev, has_pivot, n_wind)


@pytest.mark.parametrize("has_prev,has_pivot,n_wind", FLAGS)
def test_field_stats_one_element_past_alignment(dev, has_prev, has_pivot, n_wind):
    """x, prev and tsum each one element past a 16-byte boundary: W = 64 rows then start with a scalar head of three."""
    check_case(dev, (5, 3, 33, 64), has_prev, has_pivot, n_wind, offset=True)


@pytest.mark.parametrize("has_prev,has_pivot,n_wind", FLAGS)
def test_rows_whose_streams_disagree_run_scalar(dev, has_prev, has_pivot, n_wind):
    """C H W = 27 is no multiple of four, so the samples t >= 1 lie 12, 8 and 4 bytes past the alignment of sample 0: rows of
    nine points, wide enough for a vector step, take the scalar walk as a whole."""
    check_case(dev, (4, 1, 3, 9), has_prev, has_pivot, n_wind)


def test_prev_aligned_differently_from_x_runs_scalar(dev):
    """Only prev one element past a 16-byte boundary: x, tsum and the pair's row agree, prev does not."""
    shape = (5, 3, 33, 64)
    x, prev, pivot, wrow, start = problem(shape)
    want = launch(dev, x, prev, pivot, wrow, start, ([0], [2]))
    from makani_amd import _lib
    lib = _lib.load()
    T, C, H, W = shape
    xd, wd, vd = (poisoned(torch.from_numpy(a), dev) for a in (x, wrow, pivot))
    pd = shifted(torch.from_numpy(prev), dev, float("nan"))
    ws, ws_check = guarded((lib.mk_field_stats_workspace(C, H, 1),), torch.float64, dev)
    sums, sums_check = guarded((C, 4), torch.float64, dev)
    minmax, mm_check = guarded((C, 2), torch.float32, dev)
    wsums, w_check = guarded((1, 2), torch.float64, dev)
    tsum, ts_check = guarded((C, H, W), torch.float64, dev)
    tsum.copy_(torch.from_numpy(start))
    wu, wv = (torch.tensor([c], dtype=torch.int32, device=dev) for c in (0, 2))
    assert xd.data_ptr() % 16 == 0 and pd.data_ptr() % 16 == 4
    _lib.check(lib.mk_field_stats(xd.data_ptr(), pd.data_ptr(), vd.data_ptr(), wd.data_ptr(), ws.data_ptr(), sums.data_ptr(),
                                  minmax.data_ptr(), tsum.data_ptr(), wu.data_ptr(), wv.data_ptr(), 1, wsums.data_ptr(), T, C, H, W,
                                  torch.cuda.current_stream().cuda_stream), "mk_field_stats")
    torch.cuda.synchronize()
    for chk, what in ((ws_check, "workspace"), (sums_check, "sums"), (mm_check, "minmax"), (ts_check, "tsum"), (w_check, "wsums")):
        chk(what)
    # the time sum, min and max do not depend on the walk; the sums are the same terms in another order
    assert np.array_equal(tsum.cpu().numpy(), want[3]) and np.array_equal(minmax.cpu().numpy(), want[1])
    got = sums.cpu().numpy()
    for c, rows in enumerate(truth(shape, True, True)):
        for k, (val, mag, n) in enumerate(rows):
            sc.check_sum(got[c, k], val, mag, n, f"prev shifted, channel {c} sum {k}")
    for k, (val, mag, n) in enumerate(wind_truth(shape)):
        sc.check_sum(wsums.cpu().numpy()[0, k], val, mag, n, f"prev shifted, wind sum {k}")


def test_nan_stays_in_its_channel(dev):
    shape = (3, 3, 17, 20)
    rng = np.random.default_rng(1)
    x = rng.standard_normal(shape).astype(np.float32)
    prev, wrow = rng.standard_normal(shape[1:]).astype(np.float32), (0.1 + rng.random(17)).astype(np.float32)
    start = np.zeros(shape[1:])
    clean = launch(dev, x, prev, None, wrow, start, ([0], [2]))
    bad = x.copy()
    bad[1, 1, 9, 13] = np.nan
    sums, minmax, wsums, tsum = launch(dev, bad, prev, None, wrow, start, ([0], [2]))
    assert np.isnan(sums[1]).all() and np.isnan(minmax[1]).all()
    for c in (0, 2):
        assert np.array_equal(sums[c], clean[0][c]) and np.array_equal(minmax[c], clean[1][c])
    assert np.array_equal(wsums, clean[2])
    assert np.isnan(tsum[1, 9, 13]) and np.isnan(tsum).sum() == 1
    # without prev and with one sample the difference sums have no term: NaN all the same, as the channel holds one
    sums1, minmax1, _, _ = launch(dev, bad[1:2], None, None, wrow, start)
    assert np.isnan(sums1[1]).all() and np.isnan(minmax1[1]).all() and not np.isnan(sums1[[0, 2]]).any()
    # a NaN in the v channel of a pair reaches the pair's sums through the magnitude
    bad2 = x.copy()
    bad2[0, 2, 0, 0] = np.nan
    assert np.isnan(launch(dev, bad2, prev, None, wrow, start, ([0], [2]))[2]).all()


def test_second_run_equals_the_first_bit_for_bit(dev):
    shape = (5, 3, 33, 64)
    x, prev, pivot, wrow, start = problem(shape)
    a = launch(dev, x, prev, pivot, wrow, start, ([0], [2]))
    b = launch(dev, x, prev, pivot, wrow, start, ([0], [2]))
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


def test_row_slices_give_the_slices(dev):
    shape = (5, 3, 33, 64)
    x, prev, pivot, wrow, start = problem(shape)
    full = launch(dev, x, prev, pivot, wrow, start, ([0], [2]))
    parts = []
    for lo, hi in ((0, 16), (16, 33)):
        cut = lambda a: np.ascontiguousarray(a[..., lo:hi, :])
        parts.append(launch(dev, cut(x), cut(prev), pivot, wrow[lo:hi].copy(), cut(start), ([0], [2])))
        assert np.array_equal(parts[-1][3], full[3][:, lo:hi]), "the time sum of a row slice differs from the slice"
    assert np.array_equal(np.minimum(parts[0][1][:, 0], parts[1][1][:, 0]), full[1][:, 0])
    assert np.array_equal(np.maximum(parts[0][1][:, 1], parts[1][1][:, 1]), full[1][:, 1])
    for c, rows in enumerate(truth(shape, True, True)):
        for k, (_, mag, n) in enumerate(rows):
            assert abs(parts[0][0][c, k] + parts[1][0][c, k] - full[0][c, k]) <= sc.bound(mag, n), (c, k)
    for k, (_, mag, n) in enumerate(wind_truth(shape)):
        assert abs(parts[0][2][0, k] + parts[1][2][0, k] - full[2][0, k]) <= sc.bound(mag, n), k


def test_unserved_wind_pairs_are_nan(dev):
    """A pair with an index outside [0, C), or whose u channel an earlier pair names, reads nothing and gets NaN sums."""
    shape = (2, 3, 5, 8)
    x, prev, pivot, wrow, start = problem(shape)
    want = launch(dev, x, None, None, wrow, start, ([0], [2]))[2]
    got = launch(dev, x, None, None, wrow, start, ([0, 1, 0, 7], [2, 3, 1, 0]))[2]
    assert np.array_equal(got[0], want[0]) and np.isnan(got[1:]).all()


def _module_bound(x, prev, pivot, wrow):
    """(N + 3) 2^-53 sum |term| of the four sums per channel, the magnitudes in float64 torch."""
    T, C, H, W = x.shape
    xd, w = x.double(), wrow.double().reshape(1, 1, H, 1)
    d = xd - pivot.double().reshape(1, C, 1, 1)
    e = xd - torch.cat([prev.double()[None], xd[:-1]]) if prev is not None else xd[1:] - xd[:-1]
    mags = torch.stack([(w * d.abs()).sum((0, 2, 3)), (w * d * d).sum((0, 2, 3)), (w * e.abs()).sum((0, 2, 3)), (w * e * e).sum((0, 2, 3))], -1)
    n = torch.tensor([d[:, 0].numel()] * 2 + [e[:, 0].numel()] * 2, dtype=torch.float64, device=x.device)
    return (n + 3) * sc.U * mags


def test_dataset_stats_hip_equals_torch_and_replays(dev, monkeypatch):
    """``DatasetStats.update`` on the kernel against the torch path within the bound; then one update captured in a graph:
    the replay leaves the bits of the eager call."""
    from makani_amd.stats import DatasetStats
    C, H, W = 4, 33, 60
    g = torch.Generator(device=dev).manual_seed(5)
    batches = [torch.randn(t, C, H, W, device=dev, generator=g) + 50.0 * torch.arange(C, device=dev).view(1, C, 1, 1) for t in (3, 4)]

    def feed(mode, carry):
        monkeypatch.setenv("MK_STATS", mode)
        st = DatasetStats(C, (H, W), wind_pairs=([0], [2]), carry=carry)
        for b in batches:
            st.update(b)
        return st

    for carry in (False, True):
        hip, ref = feed("hip", carry), feed("torch", carry)
        assert torch.equal(hip.pivot, ref.pivot) and hip.n_diff == ref.n_diff == (6 if carry else 5)
        tol = sum(_module_bound(b, batches[i - 1][-1] if (carry and i) else None, hip.pivot, hip.wrow) for i, b in enumerate(batches))
        err = (hip.sums - ref.sums).abs()
        print(f"DatasetStats carry={carry}: worst |hip - torch| / bound {float((err / tol).max()):.4f}")
        assert bool((err <= tol).all())
        assert torch.equal(hip.tsum, ref.tsum) and torch.equal(hip.mins, ref.mins) and torch.equal(hip.maxs, ref.maxs)
        assert bool(((hip.wsums - ref.wsums).abs() <= (7 * H * W + 3) * sc.U * ref.wsums.abs()).all())
        fin_h, fin_r = hip.finalize(), ref.finalize()
        for k, v in fin_h.items():
            assert np.allclose(v[:, [1, 3]], fin_r[k][:, [1, 3]], rtol=1e-11, atol=1e-12), k
        # the pair's channels: var = W1 / N - (W0 / N)^2 has no pivot, so it carries the error of the two raw sums, each
        # (N + 3) 2^-53 of its terms on either path: at most 3 (N + 3) 2^-53 W1 / N per path, as (W0 / N)^2 <= W1 / N
        n, w1 = hip.npts, float(ref.wsums[0, 1])
        for c in (0, 2):
            assert fin_h["global_means"][0, c] == 0.0 == fin_r["global_means"][0, c]
            assert abs(fin_h["global_stds"][0, c, 0, 0] ** 2 - fin_r["global_stds"][0, c, 0, 0] ** 2) <= 6 * (n + 3) * sc.U * w1 / n

    monkeypatch.setenv("MK_STATS", "hip")
    eager = feed("hip", True)
    st = DatasetStats(C, (H, W), wind_pairs=([0], [2]), carry=True)
    st.update(batches[0])
    static = batches[1].clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st.update(static)
    graph.replay()
    torch.cuda.synchronize()
    for name in ("sums", "mins", "maxs", "tsum", "wsums", "last"):
        assert torch.equal(getattr(st, name), getattr(eager, name)), name
    assert st.n_time == eager.n_time == 7
    # a second replay runs the launches again but not the host's counting: count(T) accounts for it
    eager.update(batches[1])
    graph.replay()
    st.count(4)
    torch.cuda.synchronize()
    assert torch.equal(st.sums, eager.sums) and torch.equal(st.tsum, eager.tsum)
    assert (st.n_time, st.n_diff, st.npts, st.wtot, st.wtot_diff) == (eager.n_time, eager.n_diff, eager.npts, eager.wtot, eager.wtot_diff)
    for k, v in st.finalize().items():
        assert np.array_equal(v, eager.finalize()[k]), k


def test_tool_feeds_the_device_from_pinned_memory(dev, tmp_path):
    """tools/get_stats.py with batches staged in pinned memory and the kernel: the files of the same run on the CPU."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    try:
        import get_stats
    finally:
        sys.path.pop(0)
    rng = np.random.default_rng(2)
    x = rng.standard_normal((7, 4, 17, 20)).astype(np.float32)
    x[:, 1] += 40.0
    (tmp_path / "in").mkdir()
    np.save(tmp_path / "in" / "a.npy", x[:4])
    np.save(tmp_path / "in" / "b.npy", x[4:])
    common = ["--input_dir", str(tmp_path / "in"), "--batch_size", "3", "--carry", "--wind_angle", "--channel_names",
              '["u10m", "t2m", "v10m", "z500"]']
    assert get_stats.main(common + ["--output_dir", str(tmp_path / "gpu"), "--device", "cuda:0"]) == 0
    assert get_stats.main(common + ["--output_dir", str(tmp_path / "cpu"), "--device", "cpu"]) == 0
    from makani_amd.stats import FILES
    for name in FILES:
        a, b = np.load(tmp_path / "gpu" / f"{name}.npy"), np.load(tmp_path / "cpu" / f"{name}.npy")
        if name in ("mins", "maxs", "time_means"):
            assert np.array_equal(a, b), name
        else:
            assert np.allclose(a, b, rtol=1e-11, atol=1e-12), name
