"""What the ensemble-score tests share (a plain module, imported by tests/test_ens_cpu.py, tests/test_ens_dist_cpu.py and
tests/test_ens_gpu.py): inputs with a temperature-like channel, a numpy float64 restatement of the sums that is independent
of the code under test (``g`` from ALL PAIRS, never from a sort), a brute-force integral of the CRPS, and the bound.

The reference reads the same rounded inputs as the code under test: members are rounded to fp32 or bf16 first and then
widened, which is exact.

The bound on a sum ``S`` against the reference ``R`` over ``n = H W`` points is derived, not tuned: every per-point value is a
float64 expression of about ``2E + 8`` operations on magnitudes up to ``M = max_e |x_e| + |y|`` (``M^2`` for ``q`` and ``v``), and
the weighted values are added in an unknown order, so

    |S - R| <= 4 (n + 2E + 8) 2^-53 sum_hw w M          for a and g
    |S - R| <= 8 (n + 2E + 8) 2^-53 sum_hw w M^2        for q and v

A per-point value formed in fp32 misses it by orders of magnitude on the temperature-like channel (offset 250, spread 1)."""
import functools

import numpy as np
import torch

U = 2.0 ** -53
OFFSETS = (250.0, 0.0, -3.0)      # per channel (cycled): the first is temperature-like
SPREADS = (1.0, 1.0, 10.0)


def rounded(a, dtype):
    """``a`` rounded to ``dtype`` ("float32" or "bfloat16"), as float32 numpy (bf16 values are fp32 values)."""
    t = torch.from_numpy(np.asarray(a, dtype=np.float64)).to(getattr(torch, dtype))
    return t.float().numpy()


@functools.lru_cache(maxsize=None)
def problem(shape, dtype="float32", seed=0):
    """``(ens [B, E, C, H, W], tar [B, C, H, W], wrow [H])`` as float32 numpy, the members rounded to ``dtype``: the truth
    and the members of a point are draws around one centre, so the ranks spread over 0 ... E.  Shared between tests: do not
    write to the arrays."""
    B, E, C, H, W = shape
    rng = np.random.default_rng(seed + 1000 * E + sum(shape))
    off = np.array([OFFSETS[c % 3] for c in range(C)]).reshape(1, C, 1, 1)
    spr = np.array([SPREADS[c % 3] for c in range(C)]).reshape(1, C, 1, 1)
    centre = off + spr * rng.standard_normal((B, C, H, W))
    ens = rounded(centre[:, None] + 0.5 * spr[:, None] * rng.standard_normal((B, E, C, H, W)), dtype)
    tar = rounded(centre + 0.5 * spr * rng.standard_normal((B, C, H, W)), "float32")
    wrow = rounded(rng.uniform(0.1, 1.0, size=H) / (H * W), "float32")
    for a in (ens, tar, wrow):
        a.setflags(write=False)
    return ens, tar, wrow


def bad_points(ens, tar):
    """``[B, C, H, W]`` bool: the target or a member is NaN."""
    return np.isnan(tar) | np.isnan(ens).any(axis=1)


def point_values(ens, tar):
    """``(a, g, q, v)`` per point, ``[B, C, H, W]`` float64 each, by the definition; ``g`` over all E^2 pairs, member by
    member (no sort, no E^2 temporary).  ``v`` is NaN for E = 1.  NaN inputs give NaN values."""
    x, y = ens.astype(np.float64), tar.astype(np.float64)
    E = x.shape[1]
    with np.errstate(invalid="ignore", divide="ignore"):
        a = np.abs(x - y[:, None]).sum(axis=1) / E
        g = np.zeros_like(y)
        for e in range(E):
            g += np.abs(x - x[:, e:e + 1]).sum(axis=1)
        g /= E * E
        m = x.sum(axis=1) / E
        q = (m - y) ** 2
        v = ((x - m[:, None]) ** 2).sum(axis=1) / (E - 1) if E > 1 else np.full_like(y, np.nan)
    bad = bad_points(ens, tar)
    return tuple(np.where(bad, np.nan, f) for f in (a, g, q, v))


def sorted_g(ens):
    """``g`` per point from the members sorted ascending: ``(2 / E^2) sum_k (2k - E - 1) x_(k)``."""
    x = np.sort(ens.astype(np.float64), axis=1)
    E = x.shape[1]
    coef = (2.0 * np.arange(1, E + 1) - E - 1.0).reshape(1, E, 1, 1, 1)
    return (coef * x).sum(axis=1) * (2.0 / (E * E))


def crps_integral(x, y):
    """The CRPS of one point by its integral definition, ``int (F_ens(t) - 1{y <= t})^2 dt``: both functions are constant
    between neighbouring values of ``{x_e} + {y}``, so the integral is a sum over those intervals."""
    x = np.asarray(x, dtype=np.float64)
    z = np.sort(np.concatenate([x, [float(y)]]))
    total = 0.0
    for lo, hi in zip(z[:-1], z[1:]):
        mid = 0.5 * (lo + hi)
        total += (np.mean(x <= mid) - float(y <= mid)) ** 2 * (hi - lo)
    return total


def sums(ens, tar, wrow):
    """``[B, C, 4]`` float64: ``sum_hw wrow[h] (a, g, q, v)``; NaN where a point of the (b, c) field is skipped."""
    w = wrow.astype(np.float64).reshape(1, 1, -1, 1)
    return np.stack([(w * f).sum(axis=(-2, -1)) for f in point_values(ens, tar)], axis=-1)


def ranks_skipped(ens, tar):
    """``(ranks [C, E + 1], skipped [C])`` int64: the histogram of ``#{e : x_e < y}`` over the points that are not skipped."""
    E, C = ens.shape[1], ens.shape[2]
    bad = bad_points(ens, tar)
    with np.errstate(invalid="ignore"):
        r = (ens < tar[:, None]).sum(axis=1)
    ranks = np.stack([np.bincount(r[:, c][~bad[:, c]], minlength=E + 1) for c in range(C)]).astype(np.int64)
    return ranks, bad.sum(axis=(0, 2, 3)).astype(np.int64)


def bound(ens, tar, wrow):
    """``[B, C, 4]`` float64, the bound of the module docstring (NaN inputs count as 0 in ``M``)."""
    E, (H, W) = ens.shape[1], tar.shape[-2:]
    M = np.nan_to_num(np.abs(ens.astype(np.float64))).max(axis=1) + np.nan_to_num(np.abs(tar.astype(np.float64)))
    w = wrow.astype(np.float64).reshape(1, 1, -1, 1)
    k = (H * W + 2 * E + 8) * U
    s1, s2 = (w * M).sum(axis=(-2, -1)), (w * M * M).sum(axis=(-2, -1))
    return np.stack([4 * k * s1, 4 * k * s1, 8 * k * s2, 8 * k * s2], axis=-1)


def assert_sums(got, ens, tar, wrow, what="", names=(0, 1, 2, 3)):
    """``got [B, C, 4]`` against ``sums``: NaN exactly where the reference is NaN, within ``bound`` elsewhere.  Prints the
    worst error over the bound per sum before it asserts."""
    got = np.asarray(got, dtype=np.float64)
    want, lim = sums(ens, tar, wrow), bound(ens, tar, wrow)
    for k in names:
        nan = np.isnan(want[..., k])
        assert np.array_equal(np.isnan(got[..., k]), nan), (what, k, "NaN pattern")
        err = np.abs(got[..., k] - want[..., k])[~nan]
        worst = float((err / lim[..., k][~nan]).max()) if err.size else 0.0
        print(f"{what} sum {k}: worst error / bound = {worst:.3e}")
        assert worst <= 1.0, (what, k, worst)
