"""GPU tests of csrc/hist.hip through the C ABI (guarded outputs, poisoned inputs), of ``DatasetHistograms`` on it and of
tools/get_histograms.py.  Counts are integers: every comparison is ``np.array_equal`` against ``np.histogram``.  The inputs
lie between NaN bands and hold a known number of NaNs per channel, so a read past either end shows up as a NaN count."""
import os
import sys

import numpy as np
import pytest
import torch

import hist_checks as hc
from kernel_checks import guarded, poisoned

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1), (1, 2, 3, 5), (2, 3, 5, 8), (3, 2, 17, 20), (5, 3, 33, 64), (2, 2, 16, 1441)]
NBINS = [1, 2, 7, 100, 257, 4096]
FILL = -77          # what the guard bands of the integer outputs hold


def shifted(t, dev):
    """``t`` on the device one element past a 16-byte boundary, between NaN bands -- the element in front is NaN too."""
    flat = torch.cat([torch.full((1,), float("nan"), dtype=t.dtype), t.reshape(-1)])
    return poisoned(flat, dev)[1:].view(t.shape)


def launch(dev, x, edges, start=None, outside_start=None, offset=False, with_outside=True):
    """One call of mk_field_hist on numpy inputs; returns numpy (counts, outside) after checking every guard band."""
    from makani_amd import _lib
    lib = _lib.load()
    T, C, H, W = x.shape
    nbins = edges.shape[1] - 1
    xd = shifted(torch.from_numpy(np.array(x)), dev) if offset else poisoned(torch.from_numpy(np.array(x)), dev)
    ed = poisoned(torch.from_numpy(edges.astype(np.float64)), dev)
    counts, c_check = guarded((C, nbins), torch.int64, dev, fill=FILL)
    outside, o_check = guarded((C, 3), torch.int64, dev, fill=FILL)
    counts.copy_(torch.from_numpy(start)) if start is not None else counts.zero_()
    outside.copy_(torch.from_numpy(outside_start)) if outside_start is not None else outside.zero_()
    assert xd.data_ptr() % 16 == (4 if offset else 0)
    rc = lib.mk_field_hist(xd.data_ptr(), ed.data_ptr(), counts.data_ptr(), outside.data_ptr() if with_outside else None, nbins,
                           T, C, H, W, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "mk_field_hist")
    torch.cuda.synchronize()
    c_check("counts")
    o_check("outside")
    return counts.cpu().numpy(), outside.cpu().numpy()


def check_case(dev, shape, nbins, dtype, offset=False):
    x, edges, lo, hi = hc.problem(shape, nbins, dtype)
    counts, outside = launch(dev, x, edges, offset=offset)
    want_out = hc.outside_counts(x, edges)
    assert np.array_equal(outside[:, 2], want_out[:, 2]), "NaN counts: a read outside the channel's points?"
    assert np.array_equal(outside, want_out)
    assert np.array_equal(counts, hc.numpy_counts(x, lo, hi, nbins, dtype))
    T, C, H, W = shape
    assert (counts.sum(1) + outside.sum(1) == T * H * W).all()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("nbins", NBINS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_field_hist_equals_numpy(dev, shape, nbins, dtype):
    check_case(dev, shape, nbins, dtype)


@pytest.mark.parametrize("nbins", NBINS)
def test_one_element_past_alignment(dev, nbins):
    """x one element past a 16-byte boundary: rows of W = 64 then start with a scalar head of three."""
    check_case(dev, (5, 3, 33, 64), nbins, "float32", offset=True)


@pytest.mark.parametrize("nbins", [7, 257])
@pytest.mark.parametrize("offset", [False, True])
def test_samples_whose_alignments_disagree(dev, nbins, offset):
    """C H W = 27 is no multiple of four: the samples t >= 1 lie 12, 8 and 4 bytes past the alignment of sample 0, and
    every (sample, row) finds its own 16-byte boundary in rows of nine points."""
    check_case(dev, (4, 1, 3, 9), nbins, "float32", offset=offset)


@pytest.mark.parametrize("nbins", [7, 100, 4096])
def test_the_table_decides_not_the_guess(dev, nbins):
    """A strictly increasing table whose interior edges are moved by up to 0.4 bin widths from uniform: the uniform guess
    is off by one for many points, and the counts must still be those of the table."""
    shape = (3, 2, 17, 20)
    T, C, H, W = shape
    rng = np.random.default_rng(nbins)
    lo, hi = np.array([-2.0, 245.0]), np.array([3.0, 262.0])
    edges = np.stack([np.linspace(a, b, nbins + 1) for a, b in zip(lo, hi)])
    edges[:, 1:-1] += rng.uniform(-0.4, 0.4, size=(C, nbins - 1)) * ((hi - lo) / nbins)[:, None]
    assert (np.diff(edges, axis=1) > 0).all()
    x = (rng.uniform(size=shape) * (hi - lo).reshape(1, C, 1, 1) + lo.reshape(1, C, 1, 1)).astype(np.float32)
    hc.plant(x, edges, rng)
    counts, outside = launch(dev, x, edges)
    want = hc.table_counts(x, edges)
    assert np.array_equal(outside, hc.outside_counts(x, edges))
    assert np.array_equal(counts, want)
    # the test's own premise: binning by the uniform guess alone gets these data wrong
    v = x[:, 0].reshape(-1).astype(np.float64)
    v = v[(v >= edges[0, 0]) & (v <= edges[0, -1])]
    guess = np.minimum(((v - lo[0]) * nbins / (hi[0] - lo[0])).astype(np.int64), nbins - 1)
    assert not np.array_equal(np.bincount(guess, minlength=nbins), want[0])


@pytest.mark.parametrize("where", ["last edge", "first edge", "interior"])
@pytest.mark.parametrize("nbins", [1, 100, 4096])
def test_constant_channel_lands_in_one_bin(dev, nbins, where):
    """All T H W points of a channel in one bin: every lane of every wave adds to one address."""
    from makani_amd import ops
    shape = (2, 2, 33, 64)
    T, C, H, W = shape
    edges = ops.hist_edges(np.array([-1.0, 200.0]), np.array([1.0, 300.0]), nbins)
    b = {"last edge": nbins - 1, "first edge": 0, "interior": nbins // 2}[where]
    x = np.empty(shape, dtype=np.float32)
    for c in range(C):
        x[:, c] = {"last edge": edges[c, -1], "first edge": edges[c, 0], "interior": edges[c, b]}[where]
    counts, outside = launch(dev, x, edges)
    want = np.zeros((C, nbins), dtype=np.int64)
    want[:, b] = T * H * W
    assert np.array_equal(counts, want) and not outside.any()
    assert np.array_equal(counts, hc.table_counts(x, edges))


def test_counts_are_added_to_and_runs_repeat(dev):
    shape, nbins = (5, 3, 33, 64), 100
    x, edges, lo, hi = hc.problem(shape, nbins)
    want, want_out = hc.numpy_counts(x, lo, hi, nbins), hc.outside_counts(x, edges)
    rng = np.random.default_rng(3)
    start = rng.integers(2 ** 32, 2 ** 40, size=(3, nbins), dtype=np.int64)
    start[0, :2] = [2 ** 32 - 1, 0]
    ostart = rng.integers(2 ** 32, 2 ** 40, size=(3, 3), dtype=np.int64)
    one, one_out = launch(dev, x, edges, start, ostart)
    assert np.array_equal(one, start + want) and np.array_equal(one_out, ostart + want_out)
    two, two_out = launch(dev, x, edges, one, one_out)                           # a second call on the result of the first
    assert np.array_equal(two, start + 2 * want) and np.array_equal(two_out, ostart + 2 * want_out)
    again, again_out = launch(dev, x, edges, start, ostart)                      # a second identical run
    assert np.array_equal(again, one) and np.array_equal(again_out, one_out)
    none, untouched = launch(dev, x, edges, with_outside=False)                  # outside = NULL: nothing is written there
    assert np.array_equal(none, want) and not untouched.any()


@pytest.mark.parametrize("nbins", [100, 4096])
def test_row_slices_add_up_to_the_whole(dev, nbins):
    shape = (5, 3, 33, 64)
    x, edges, lo, hi = hc.problem(shape, nbins)
    full, full_out = launch(dev, x, edges)
    parts = [launch(dev, np.ascontiguousarray(x[..., a:b, :]), edges) for a, b in ((0, 16), (16, 33))]
    assert np.array_equal(parts[0][0] + parts[1][0], full) and np.array_equal(parts[0][1] + parts[1][1], full_out)
    assert np.array_equal(full, hc.numpy_counts(x, lo, hi, nbins))


def test_dataset_histograms_hip_equals_torch_and_replays(dev, monkeypatch):
    """``DatasetHistograms.update`` on the kernel equals the torch path exactly; then one update captured in a graph: the
    replay leaves what the eager call leaves."""
    from makani_amd.histograms import DatasetHistograms
    C, H, W = 4, 33, 60
    g = torch.Generator(device=dev).manual_seed(5)
    batches = [torch.randn(t, C, H, W, device=dev, generator=g) + 50.0 * torch.arange(C, device=dev).view(1, C, 1, 1) for t in (3, 4)]
    both = torch.cat(batches)
    lo = both.amin((0, 2, 3)).cpu().numpy() + 0.5        # a range inside the data: some points fall outside
    hi = both.amax((0, 2, 3)).cpu().numpy() - 0.5
    batches[1][2, 1, 5, 7] = float("nan")
    both = torch.cat(batches)

    def feed(mode, nbins):
        monkeypatch.setenv("MK_HIST", mode)
        acc = DatasetHistograms(C, lo, hi, nbins=nbins)
        for b in batches:
            acc.update(b)
        return acc

    for nbins in (50, 4096, 5000):                       # 5000: both run the torch formulation
        hip, ref = feed("hip", nbins), feed("torch", nbins)
        fh, fr = hip.finalize(), ref.finalize()
        for k in ("edges", "data", "outside"):
            assert np.array_equal(fh[k], fr[k]), (nbins, k)
        assert fh["count"] == fr["count"] == 7 and fh["outside"][1, 2] == 1 and fh["outside"][:, :2].all()
        x = both.cpu().numpy()
        assert np.array_equal(fh["data"], hc.numpy_counts(x, lo, hi, nbins))

    eager = feed("hip", 50)
    acc = DatasetHistograms(C, lo, hi, nbins=50)
    acc.update(batches[0])
    static = batches[1].clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        acc.update(static)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(acc.counts, eager.counts) and torch.equal(acc.outside, eager.outside) and acc.n_time == eager.n_time == 7
    # a second replay runs the launch again but not the host's counting: count(T) accounts for it
    eager.update(batches[1])
    graph.replay()
    acc.count(4)
    torch.cuda.synchronize()
    fa, fe = acc.finalize(), eager.finalize()
    assert fa["count"] == fe["count"] == 11
    for k in ("edges", "data", "outside"):
        assert np.array_equal(fa[k], fe[k]), k


def test_tool_on_the_device_writes_what_it_writes_on_the_cpu(dev, tmp_path):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    try:
        import get_histograms
    finally:
        sys.path.pop(0)
    rng = np.random.default_rng(2)
    x = rng.standard_normal((7, 4, 17, 20)).astype(np.float32)
    x[:, 1] += 40.0
    (tmp_path / "in").mkdir()
    np.save(tmp_path / "in" / "a.npy", x[:4])
    np.save(tmp_path / "in" / "b.npy", x[4:])
    common = ["--input_dir", str(tmp_path / "in"), "--batch_size", "3", "--nbins", "31"]
    assert get_histograms.main(common + ["--output_dir", str(tmp_path / "gpu"), "--device", "cuda:0"]) == 0
    assert get_histograms.main(common + ["--output_dir", str(tmp_path / "cpu"), "--device", "cpu"]) == 0
    with np.load(tmp_path / "gpu" / "histograms.npz") as a, np.load(tmp_path / "cpu" / "histograms.npz") as b:
        assert set(a.files) == set(b.files) == {"edges", "data", "outside", "count"}
        for k in a.files:
            assert np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype, k
        mins, maxs = x.min((0, 2, 3)), x.max((0, 2, 3))
        assert np.array_equal(a["data"], hc.numpy_counts(x, mins, maxs, 31)) and not a["outside"].any()
