"""What the histogram tests share (a plain module, imported by tests/test_hist_cpu.py and tests/test_hist_gpu.py): inputs that
sit on and next to every edge, and the counts ``np.histogram`` gives for them.  All comparisons are exact."""
import functools

import numpy as np

F32 = np.float32


def neighbours(values):
    """The fp32 roundings of ``values`` and their fp32 neighbours below and above."""
    e = np.asarray(values).astype(F32)
    return np.concatenate([e, np.nextafter(e, F32(-np.inf)), np.nextafter(e, F32(np.inf))])


def plant(x, edges, rng):
    """Overwrites up to half of each channel's points of ``x`` ``[T, C, H, W]`` (fp32, in place) with: every edge of the
    channel's table and its fp32 neighbours both ways (the first and last edge, i.e. lo and hi, among them), points outside
    on both sides, NaN, +inf and -inf.  With fewer points than values a random choice of them goes in, the NaN first."""
    T, C, H, W = x.shape
    for c in range(C):
        e = edges[c].astype(np.float64)
        width = e[-1] - e[0]
        special = np.concatenate([neighbours(e), np.array([e[0] - 0.3 * width, e[0] - 1.0, e[-1] + 0.3 * width, e[-1] + 1.0,
                                                           np.inf, -np.inf, np.inf], dtype=F32)])
        special = np.concatenate([np.full(1 + c, np.nan, dtype=F32), rng.permutation(special)])[:(T * H * W) // 2]
        where = rng.permutation(T * H * W)[:special.size]
        flat = np.ascontiguousarray(x[:, c]).reshape(-1)
        flat[where] = special
        x[:, c] = flat.reshape(T, H, W)
    return x


@functools.lru_cache(maxsize=None)
def problem(shape, nbins, edge_dtype="float32", seed=0):
    """``(x, edges, lo, hi)``: fp32 samples with a per-channel offset and scale, the table ``hist_edges`` builds over the range
    of the clean samples, and the special values of ``plant``.  Shared between tests: do not write to the arrays."""
    from makani_amd import ops
    T, C, H, W = shape
    rng = np.random.default_rng(seed + 7 * nbins + sum(shape))
    off = (250.0 * np.arange(C)).reshape(1, C, 1, 1)
    scale = (10.0 ** (np.arange(C) % 3 - 1)).reshape(1, C, 1, 1)
    x = (rng.standard_normal(shape) * scale + off).astype(F32)
    lo, hi = x.min((0, 2, 3)).astype(np.float64), x.max((0, 2, 3)).astype(np.float64)
    edges = ops.hist_edges(lo, hi, nbins, dtype=edge_dtype)
    plant(x, edges, rng)
    for a in (x, edges, lo, hi):
        a.setflags(write=False)
    return x, edges, lo, hi


def outside_counts(x, edges):
    """``[C, 3]`` int64: the points below the first edge, above the last, and the NaNs, per channel."""
    out = np.zeros((x.shape[1], 3), dtype=np.int64)
    for c in range(x.shape[1]):
        v = x[:, c].reshape(-1).astype(np.float64)
        out[c] = [(v < edges[c, 0]).sum(), (v > edges[c, -1]).sum(), np.isnan(v).sum()]
    return out


def numpy_counts(x, lo, hi, nbins, edge_dtype="float32"):
    """``[C, nbins]`` int64: ``np.histogram(x_c, bins=nbins, range=(lo_c, hi_c))`` per channel -- the reference's call, on fp32
    data for an fp32 table and on the data widened to float64 for a float64 table."""
    out = np.zeros((x.shape[1], nbins), dtype=np.int64)
    for c in range(x.shape[1]):
        v = x[:, c].reshape(-1).astype(edge_dtype)
        out[c], _ = np.histogram(v, bins=nbins, range=(float(lo[c]), float(hi[c])))
    return out


def table_counts(x, edges):
    """``[C, nbins]`` int64 by the definition, for any strictly increasing table: ``np.histogram`` with explicit edges
    (a sorted search against the table, the last bin closed) over the points that are not NaN."""
    out = np.zeros((x.shape[1], edges.shape[1] - 1), dtype=np.int64)
    for c in range(x.shape[1]):
        v = x[:, c].reshape(-1).astype(np.float64)
        out[c], _ = np.histogram(v[~np.isnan(v)], bins=edges[c].astype(np.float64))
    return out
