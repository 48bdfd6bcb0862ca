"""CPU tests of the dataset histograms: ``ops.hist_edges`` and ``ops.field_hist`` (torch path) against ``np.histogram``,
``DatasetHistograms``, tools/get_histograms.py and the argument checks of ``mk_field_hist``.  Counts are integers and every
comparison is ``np.array_equal``: there is no tolerance in this file."""
import os
import sys

import numpy as np
import pytest
import torch

import hist_checks as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EDGE_CASES = [(off, scale, nbins, dtype) for off in (0.0, 250.0, 1e5) for scale in (1e-3, 1.0, 300.0)
              for nbins in (1, 2, 7, 100, 4096) for dtype in ("float32", "float64")]


# ---------------------------------------------------------------------------------------------------------------------
# edges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_hist_edges_are_numpys_bit_for_bit(dtype):
    from makani_amd import ops
    rng = np.random.default_rng(0)
    seen = raised = 0
    for off, scale, nbins, dt in EDGE_CASES:
        if dt != dtype:
            continue
        for lo, hi in ((off - scale * rng.random(), off + scale * rng.random()), (off, off), (off + scale, off + scale)):
            # bounds as the reference passes them: fp32 mins / maxs turned into Python floats
            lo, hi = float(np.float32(lo)), float(np.float32(hi))
            data = np.zeros(1, dtype=dtype)
            try:
                want = np.histogram(data, bins=nbins, range=(lo, hi))[1]
            except ValueError as e:
                assert "Too many bins" in str(e)
                with pytest.raises(ValueError, match="Too many bins for data range"):
                    ops.hist_edges(lo, hi, nbins, dtype=dtype)
                raised += 1
                continue
            got = ops.hist_edges(lo, hi, nbins, dtype=dtype)
            assert got.shape == (1, nbins + 1) and got.dtype == want.dtype == np.dtype(dtype)
            assert np.array_equal(got[0].view(np.uint8), want.view(np.uint8)), (lo, hi, nbins, dtype)
            if lo == hi:
                assert got[0, 0] == lo - 0.5 and got[0, -1] == hi + 0.5
            seen += 1
    assert seen >= 100 and (raised > 0) == (dtype == "float32"), (seen, raised)   # fp32: 4096 bins across 2e-3 at 1e5 cannot be


def test_hist_edges_of_several_channels_and_its_refusals():
    from makani_amd import ops
    lo, hi = np.array([-3.0, 250.0, 7.0]), np.array([4.0, 251.5, 7.0])
    got = ops.hist_edges(lo, hi, 7)
    for c in range(3):
        assert np.array_equal(got[c], np.histogram(np.zeros(1, np.float32), bins=7, range=(float(lo[c]), float(hi[c])))[1])
    for a, b, n, msg in ((0.0, np.inf, 4, "not finite"), (np.nan, 1.0, 4, "not finite"), (2.0, 1.0, 4, "max must be larger"),
                         (0.0, 1.0, 0, "nbins"), (0.0, 1.0, -3, "nbins"), (0.0, 1.0, 2.5, "nbins"),
                         (1e5, 1e5 + 0.01, 100, "Too many bins for data range")):
        with pytest.raises(ValueError, match=msg):
            ops.hist_edges(a, b, n)
    assert ops.hist_edges(1e5, 1e5 + 0.01, 100, dtype=np.float64).shape == (1, 101)     # float64 has the room
    with pytest.raises(ValueError, match="float32 or float64"):
        ops.hist_edges(0.0, 1.0, 4, dtype=np.float16)
    with pytest.raises(ValueError, match="scalars or"):
        ops.hist_edges([0.0, 1.0], [2.0], 4)


# ---------------------------------------------------------------------------------------------------------------------
# the op on CPU tensors
# ---------------------------------------------------------------------------------------------------------------------
def run_op(x, edges, start=None, outside_start=None):
    from makani_amd import ops
    C, nbins = edges.shape[0], edges.shape[1] - 1
    counts = torch.zeros(C, nbins, dtype=torch.int64) if start is None else torch.from_numpy(start.copy())
    outside = torch.zeros(C, 3, dtype=torch.int64) if outside_start is None else torch.from_numpy(outside_start.copy())
    assert ops.field_hist(torch.from_numpy(np.array(x)), torch.from_numpy(edges.astype(np.float64)), counts, outside) is counts
    return counts.numpy(), outside.numpy()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("nbins", [1, 2, 7, 100, 4096, 5000])
def test_field_hist_on_cpu_equals_numpy(nbins, dtype):
    """Random fp32 with per-channel offsets, every edge and its fp32 neighbours, lo and hi, points outside, NaN and +-inf."""
    shape = (2, 3, 40, 64)
    x, edges, lo, hi = hc.problem(shape, nbins, dtype)
    counts, outside = run_op(x, edges)
    assert np.array_equal(counts, hc.numpy_counts(x, lo, hi, nbins, dtype))
    assert np.array_equal(counts, hc.table_counts(x, edges))
    want_out = hc.outside_counts(x, edges)
    assert np.array_equal(outside, want_out)
    assert (want_out[:, 2] == np.arange(1, 4)).all()                                        # the test's own data: c + 1 NaNs
    assert nbins > 100 or (want_out[:, :2] >= 3).all()                                      # ... and every value outside went in
    assert (counts.sum(1) + outside.sum(1) == 2 * 40 * 64).all()


def test_counts_accumulate_from_a_start_above_two_to_the_32():
    shape, nbins = (2, 3, 40, 64), 100
    x, edges, lo, hi = hc.problem(shape, nbins)
    rng = np.random.default_rng(3)
    start = rng.integers(0, 2 ** 40, size=(3, nbins), dtype=np.int64)
    start[0, 0] = 2 ** 32 - 1
    ostart = rng.integers(2 ** 32, 2 ** 40, size=(3, 3), dtype=np.int64)
    counts, outside = run_op(x, edges, start, ostart)
    assert np.array_equal(counts, start + hc.numpy_counts(x, lo, hi, nbins))
    assert np.array_equal(outside, ostart + hc.outside_counts(x, edges))
    from makani_amd import ops
    c2 = torch.zeros(3, nbins, dtype=torch.int64)
    ops.field_hist(torch.from_numpy(np.array(x)), torch.from_numpy(edges.astype(np.float64)), c2)       # outside=None
    assert np.array_equal(c2.numpy(), counts - start)


def test_knob_and_arguments_are_validated(monkeypatch):
    from makani_amd import build, ops
    assert "hist.hip" in build.SOURCES and ops.HIST_DEFAULT in ("hip", "torch") and ops.HIST_MAX_BINS == 4096
    x = torch.zeros(2, 3, 4, 5)
    edges = torch.from_numpy(ops.hist_edges(np.zeros(3), np.ones(3), 7).astype(np.float64))
    counts, outside = torch.zeros(3, 7, dtype=torch.int64), torch.zeros(3, 3, dtype=torch.int64)
    monkeypatch.setenv("MK_HIST", "cuda")
    with pytest.raises(ValueError, match="MK_HIST"):
        ops.field_hist(x, edges, counts)
    monkeypatch.setenv("MK_HIST", "torch")
    ops.field_hist(x, edges, counts, outside)
    assert int(counts[:, 0].sum()) == 3 * 40 and int(counts.sum()) == 120 and int(outside.sum()) == 0
    for args, msg in (((x.double(), edges, counts), "fp32"), ((x[0], edges, counts), "fp32"), ((x, edges.float(), counts), "float64"),
                      ((x, edges[:2], counts), "edges"), ((x, edges[:, :1], counts), "edges"), ((x, edges.t().contiguous().t(), counts), "edges"),
                      ((x, edges, counts.int()), "int64"), ((x, edges, counts[:, :6]), "counts"), ((x, edges, counts, outside.float()), "outside"),
                      ((x, edges, counts, outside[:, :2]), "outside"), ((x[:0], edges, counts), "empty")):
        with pytest.raises(ValueError, match=msg):
            ops.field_hist(*args)


# ---------------------------------------------------------------------------------------------------------------------
# DatasetHistograms
# ---------------------------------------------------------------------------------------------------------------------
def dataset(t=7, c=3, h=9, w=12, seed=1):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((t, c, h, w)) * (1.0 + np.arange(c)).reshape(1, c, 1, 1) + 100.0 * np.arange(c).reshape(1, c, 1, 1))
    return x.astype(np.float32)


def test_batches_of_three_and_four_equal_one_of_seven_and_numpy():
    from makani_amd.histograms import DatasetHistograms
    x = dataset()
    lo, hi = x.min((0, 2, 3)), x.max((0, 2, 3))
    one = DatasetHistograms(3, lo, hi, nbins=20).update(torch.from_numpy(x)).finalize()
    two = DatasetHistograms(3, lo.reshape(1, 3, 1, 1), hi.reshape(1, 3, 1, 1), nbins=20)
    two.update(torch.from_numpy(x[:3])).update(torch.from_numpy(x[3:]))
    two = two.finalize()
    assert one["count"] == two["count"] == 7
    for k in ("edges", "data", "outside"):
        assert np.array_equal(one[k], two[k]), k
    assert one["edges"].dtype == np.float32 and one["data"].dtype == np.int64 and one["data"].shape == (3, 20)
    assert np.array_equal(one["data"], hc.numpy_counts(x, lo, hi, 20)) and not one["outside"].any()
    assert (one["data"].sum(1) == 7 * 9 * 12).all()
    f64 = DatasetHistograms(3, lo, hi, nbins=20, edge_dtype="float64").update(torch.from_numpy(x)).finalize()
    assert f64["edges"].dtype == np.float64 and np.array_equal(f64["data"], hc.numpy_counts(x, lo, hi, 20, "float64"))


def test_merge_adds_and_refuses_other_edges(tmp_path):
    from makani_amd.histograms import KEYS, DatasetHistograms
    x = dataset()
    lo, hi = x.min((0, 2, 3)), x.max((0, 2, 3))
    a = DatasetHistograms(3, lo, hi, nbins=11).update(torch.from_numpy(x[:2]))
    b = DatasetHistograms(3, lo, hi, nbins=11).update(torch.from_numpy(x[2:]))
    empty = DatasetHistograms(3, lo, hi, nbins=11)
    want = a.finalize()["data"] + b.finalize()["data"]
    got = empty.merge(a).merge(b).merge(DatasetHistograms(3, lo, hi, nbins=11)).finalize()
    assert np.array_equal(got["data"], want) and got["count"] == 7
    assert np.array_equal(got["data"], hc.numpy_counts(x, lo, hi, 11))
    for other in (DatasetHistograms(3, lo, hi, nbins=12), DatasetHistograms(3, lo, hi + 1.0, nbins=11),
                  DatasetHistograms(3, lo, hi, nbins=11, edge_dtype="float64")):
        with pytest.raises(ValueError, match="edges"):
            a.merge(other)
    with pytest.raises(RuntimeError, match="no sample"):
        DatasetHistograms(3, lo, hi).finalize()
    with pytest.raises(ValueError, match="one value per channel"):
        DatasetHistograms(3, lo[:2], hi)
    with pytest.raises(ValueError, match="batch"):
        a.update(torch.zeros(2, 4, 9, 12))
    # save -> np.load
    out = empty.save(str(tmp_path / "h"))
    with np.load(tmp_path / "h" / "histograms.npz") as f:
        assert set(f.files) == set(KEYS)
        for k in ("edges", "data", "outside"):
            assert np.array_equal(f[k], out[k]) and f[k].dtype == out[k].dtype, k
        assert int(f["count"]) == 7
    # data outside the range is counted, not binned
    narrow = DatasetHistograms(3, lo + 1.0, hi - 1.0, nbins=5).update(torch.from_numpy(x)).finalize()
    assert np.array_equal(narrow["outside"], hc.outside_counts(x, narrow["edges"])) and narrow["outside"][:, :2].all()
    assert (narrow["data"].sum(1) + narrow["outside"].sum(1) == 7 * 9 * 12).all()


# ---------------------------------------------------------------------------------------------------------------------
# the tool
# ---------------------------------------------------------------------------------------------------------------------
def tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import get_histograms
    finally:
        sys.path.pop(0)
    return get_histograms


@pytest.mark.parametrize("batch_size", [2, 3])
@pytest.mark.parametrize("with_stats_dir", [False, True])
def test_tool_equals_the_restated_reference(tmp_path, capsys, with_stats_dir, batch_size):
    """The reference's algorithm in a few numpy lines: min and max per channel over all files, then np.histogram of the
    channel's points over that range."""
    x = dataset(t=7, c=3, h=9, w=12, seed=4)
    (tmp_path / "in").mkdir()
    np.save(tmp_path / "in" / "a.npy", x[:4])
    np.save(tmp_path / "in" / "b.npy", x[4:])
    mins, maxs = x.min((0, 2, 3)), x.max((0, 2, 3))
    want = np.stack([np.histogram(x[:, c].reshape(-1), bins=13, range=(mins[c].tolist(), maxs[c].tolist()))[0] for c in range(3)])
    want_edges = np.stack([np.histogram(x[:, c].reshape(-1), bins=13, range=(mins[c].tolist(), maxs[c].tolist()))[1] for c in range(3)])
    argv = ["--input_dir", str(tmp_path / "in"), "--output_dir", str(tmp_path / "out"), "--nbins", "13", "--batch_size",
            str(batch_size), "--device", "cpu"]
    if with_stats_dir:
        (tmp_path / "stats").mkdir()
        np.save(tmp_path / "stats" / "mins.npy", mins.astype(np.float64).reshape(1, 3, 1, 1))
        np.save(tmp_path / "stats" / "maxs.npy", maxs.astype(np.float64).reshape(1, 3, 1, 1))
        argv += ["--stats_dir", str(tmp_path / "stats")]
    else:
        argv += ["--write_stats"]
    assert tool().main(argv) == 0
    with np.load(tmp_path / "out" / "histograms.npz") as f:
        assert np.array_equal(f["data"], want) and np.array_equal(f["edges"], want_edges) and f["edges"].dtype == np.float32
        assert not f["outside"].any() and int(f["count"]) == 7
    text = capsys.readouterr().out
    assert f"Data range overview on {7 * 9 * 12} datapoints:" in text and f"0: min = {float(mins[0])}, max = {float(maxs[0])}" in text
    assert ("stats done" in text) == (not with_stats_dir)
    assert os.path.exists(tmp_path / "out" / "mins.npy") == (not with_stats_dir)


def test_tool_with_sqrt_bins_metadata_and_outside_points(tmp_path, capsys):
    import json
    x = dataset(t=5, c=2, h=9, w=12, seed=5)
    (tmp_path / "in").mkdir()
    np.save(tmp_path / "in" / "a.npy", x)
    (tmp_path / "stats").mkdir()
    np.save(tmp_path / "stats" / "mins.npy", np.array([-1.0, 99.0]))
    np.save(tmp_path / "stats" / "maxs.npy", np.array([1.0, 101.0]))
    with open(tmp_path / "meta.json", "w") as f:
        json.dump({"coords": {"channel": ["t2m", "z500"]}}, f)
    argv = ["--input_dir", str(tmp_path / "in"), "--output_dir", str(tmp_path / "out"), "--nbins", "0", "--device", "cpu",
            "--stats_dir", str(tmp_path / "stats"), "--metadata_file", str(tmp_path / "meta.json")]
    assert tool().main(argv) == 0
    nbins = int(round(np.sqrt(5 * 9 * 12)))
    with np.load(tmp_path / "out" / "histograms.npz") as f:
        assert f["data"].shape == (2, nbins)
        want = np.stack([np.histogram(x[:, c].reshape(-1), bins=nbins, range=r)[0] for c, r in enumerate(((-1.0, 1.0), (99.0, 101.0)))])
        assert np.array_equal(f["data"], want)
        assert np.array_equal(f["outside"], hc.outside_counts(x, f["edges"])) and f["outside"][:, :2].all()
    text = capsys.readouterr().out
    assert "t2m: min = -1.0, max = 1.0" in text and "z500: below = " in text


# ---------------------------------------------------------------------------------------------------------------------
# the entry point
# ---------------------------------------------------------------------------------------------------------------------
_P = 4096      # a non-null, 16-byte aligned address that is never dereferenced: validation returns before any launch
_OK = dict(x=_P, edges=_P, counts=_P, outside=None, nbins=100, T=2, C=3, H=9, W=16)
HIST_REJECTED = [(dict(nbins=0), b"nbins"), (dict(nbins=4097), b"nbins"), (dict(nbins=-1), b"nbins"), (dict(x=None), b"null pointer"),
                 (dict(edges=None), b"null pointer"), (dict(counts=None), b"null pointer"), (dict(edges=_P + 4), b"8-byte aligned"),
                 (dict(counts=_P + 4), b"8-byte aligned"), (dict(outside=_P + 4), b"8-byte aligned"), (dict(x=_P + 2), b"4-byte aligned"),
                 (dict(T=0), b"bad sizes"), (dict(W=-1), b"bad sizes"), (dict(C=70000, H=1, W=1), b"32-bit grid range"),
                 (dict(C=73, H=7210, W=14400), b"32-bit grid range"), (dict(T=2 ** 20, C=1, H=16, W=2 ** 10), b"32-bit bin")]       # 4 rows of a workgroup x W x T = 2^32


@pytest.mark.parametrize("bad,msg", HIST_REJECTED, ids=["-".join(f"{k}={v}" for k, v in b.items()) for b, _ in HIST_REJECTED])
def test_entry_point_refuses_before_any_launch(bad, msg):
    from makani_amd import _lib
    lib = _lib.load()
    a = dict(_OK, **bad)
    lib.mk_quadrature(7, 10, 0, 0)      # leaves a message of another function behind: the one below must replace it
    assert lib.mk_field_hist(*[a[k] for k in _OK], None) == 1
    got = lib.mk_last_error()
    assert got.startswith(b"mk_field_hist: ") and msg in got, got


def test_symbol_is_declared_and_built():
    from makani_amd import _lib
    lib = _lib.load()
    I, P = _lib.ctypes.c_int, _lib.ctypes.c_void_p
    assert _lib.SIGNATURES["mk_field_hist"] == (I, [P, P, P, P, I, I, I, I, I, P])
    assert hasattr(lib, "mk_field_hist")
