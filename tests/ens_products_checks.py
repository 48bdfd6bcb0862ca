"""What the ensemble-product tests share (a plain module, imported by tests/test_ens_products_cpu.py and
tests/test_ens_products_gpu.py): a numpy float64 restatement of the products that is independent of the code under test
(``np.sort``, the formulas of include/makani_amd.h, members rounded to their dtype first and then widened, which is exact),
the bounds, and the assertion that holds a result to them.

The bounds are derived from the operands, never from a measured error.  ``u = 2^-53``, ``M = max_e |x_e|`` of the point, ``r`` the
reference value, the result taken in fp32 BEFORE scale and shift.  Both sides form the value in float64 and the result is
rounded once to fp32, ``2^-24 |r|``; the ``2^-40 |r|`` next to it covers a float64 error that moves the value across an fp32 tie.

* mean: E - 1 additions of magnitudes up to ``E M`` and a division on each side, in any order:
  ``(2^-24 + 2^-40) |r| + (E + 2) u M``.
* std: the deviations ``x_e - m`` are exact up to the error of ``m``, which a two-pass sum forgives to second order; E products,
  E additions, a division and a root are relative errors, the error of ``m`` an absolute one:
  ``(2^-24 + 2^-40) |r| + (E + 6) u |r| + 4 (E + 2) u M``.  E equal members give an exact ``+0`` (``m = x`` exactly).
* order statistic with ``t > 0``: a difference, a product and a sum (or one fma) of ``a = x_(k)``, ``b = x_(k+1)``:
  ``(2^-24 + 2^-40) |r| + 2^-52 (|a| + |b|)``, and ``a <= out <= b`` because rounding is monotone and a, b are fp32 values.
* order statistic with ``t == 0``, ``above``, ``below``: a member's value, or one IEEE fp32 division of two small integers:
  bit-equal.
* with scale and shift: bit-equal to ``np.float32(out_plain) * s + t`` evaluated in fp32 on the host; bf16: bit-equal to the
  bf16 rounding (to nearest even) of the fp32 result.
"""
import collections

import numpy as np
import torch

MEAN, STD, ORDER, ABOVE, BELOW = range(5)
Plane = collections.namedtuple("Plane", "kind exact want lo hi M E equal")


def quantile_position(q, E):
    """The test's own ``(k, t)`` of numpy's ``linear`` quantile."""
    if q == 1.0:
        return E - 1, 0.0
    h = float(q) * (E - 1)
    return int(np.floor(h)), h - np.floor(h)


def table7(E, q=0.3):
    """K = 7: mean, std, min, a quantile with ``t > 0``, max, above, below -- ``(kinds, orders, fracs)``."""
    k, t = quantile_position(q, E)
    if t == 0.0:                     # q (E - 1) an integer (E = 2 never: 0.3): take a fraction that is none
        k, t = min(k, E - 2), 0.375
    return [MEAN, STD, ORDER, ORDER, ORDER, ABOVE, BELOW], [0, 0, 0, k, E - 1, 0, 0], [0.0, 0.0, 0.0, t, 0.0, 0.0, 0.0]


def thresholds(ens, K, chans=None, seed=0):
    """``[K, Cs]`` fp32 thresholds inside the members' range: per selected channel a value near the channel's centre."""
    x = ens if chans is None else ens[:, :, list(chans)]
    rng = np.random.default_rng(seed)
    mid = np.nanmedian(x.astype(np.float64), axis=(0, 1, 3, 4))
    spr = np.nanstd(x.astype(np.float64), axis=(0, 1, 3, 4)) + 0.25
    return (mid[None] + spr[None] * rng.uniform(-0.5, 0.5, size=(K, x.shape[2]))).astype(np.float32)


def reference(ens, table, chans=None, thr=None):
    """One ``Plane`` per product for the fp32 numpy members ``ens`` ``[B, E, C, H, W]`` (already rounded to their dtype): ``want``
    ``[B, Cs, H, W]`` is float64 for the bounded kinds and float32 for the exact ones, NaN where a member or the threshold is."""
    kinds, orders, fracs = table
    x32 = np.asarray(ens, dtype=np.float32)
    if chans is not None:
        x32 = x32[:, :, list(chans)]
    x = x32.astype(np.float64)
    E = x.shape[1]
    bad = np.isnan(x32).any(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        M = np.nan_to_num(np.abs(x)).max(axis=1)
        m = np.zeros_like(x[:, 0])
        for e in range(E):
            m = m + x[:, e]
        m = m / E
        sv = np.zeros_like(m)
        for e in range(E):
            sv = sv + (x[:, e] - m) ** 2
        sd = np.sqrt(sv / (E - 1)) if E > 1 else np.full_like(m, np.nan)
        xs = np.sort(x32, axis=1)
        equal = (x32 == x32[:, :1]).all(axis=1)
        planes = []
        for i, kind in enumerate(kinds):
            lo = hi = None
            if kind == MEAN:
                want, exact = m, False
            elif kind == STD:
                want, exact = sd, False
            elif kind == ORDER:
                k, t = int(orders[i]), float(fracs[i])
                if t == 0.0:
                    want, exact = xs[:, k], True
                else:
                    lo, hi = xs[:, k], xs[:, k + 1]
                    a, b = lo.astype(np.float64), hi.astype(np.float64)
                    want, exact = a + t * (b - a), False
            else:
                th = np.asarray(thr, dtype=np.float32)[i].reshape(1, -1, 1, 1)
                cnt = ((x32 > th[:, None]) if kind == ABOVE else (x32 < th[:, None])).sum(axis=1)
                want = np.float32(cnt) / np.float32(E)
                want, exact = np.where(np.isnan(th), np.float32(np.nan), want).astype(np.float32), True
            want = np.where(bad, np.nan, want).astype(np.float32 if exact else np.float64)
            planes.append(Plane(kind, exact, want, lo, hi, M, E, equal & ~bad))
    return planes


def bound(p):
    """The bound of the module docstring for a bounded plane (NaN points count as 0)."""
    r, E, u = np.nan_to_num(np.abs(p.want)), p.E, 2.0 ** -53
    lim = (2.0 ** -24 + 2.0 ** -40) * r
    if p.kind == MEAN:
        return lim + (E + 2) * u * p.M
    if p.kind == STD:
        return lim + (E + 6) * u * r + 4 * (E + 2) * u * p.M
    return lim + 2.0 ** -52 * (np.abs(p.lo.astype(np.float64)) + np.abs(p.hi.astype(np.float64)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def assert_products(got, planes, what=""):
    """``got`` ``[B, K, Cs, H, W]`` fp32 (no scale, no shift) against ``reference``: NaN exactly where the reference has it, the
    exact planes bit for bit, the others within ``bound`` (and ``lo <= got <= hi``, and ``+0`` for the spread of equal members).
    Prints the worst error over the bound per bounded plane before it asserts."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape[1] == len(planes), (what, got.dtype, got.shape)
    for i, p in enumerate(planes):
        g = got[:, i]
        nan = np.isnan(p.want)
        assert np.array_equal(np.isnan(g), nan), (what, i, "NaN pattern")
        ok = ~nan
        if p.exact:
            assert np.array_equal(bits(g[ok]), bits(p.want[ok])), (what, i, "an exact plane differs")
            continue
        err, lim = np.abs(g.astype(np.float64) - p.want)[ok], bound(p)[ok]
        worst = float((err[lim > 0] / lim[lim > 0]).max()) if (lim > 0).any() else 0.0
        print(f"{what} plane {i} (kind {p.kind}): worst error / bound = {worst:.3e}")
        assert (err <= lim).all(), (what, i, worst)
        if p.kind == ORDER:
            assert ((p.lo[ok] <= g[ok]) & (g[ok] <= p.hi[ok])).all(), (what, i, "outside [x_(k), x_(k+1)]")
        if p.kind == STD:
            assert not bits(g[p.equal]).any(), (what, i, "the spread of equal members is not +0")


def affine(plain, kinds, scale, shift):
    """``plain`` ``[B, K, Cs, H, W]`` fp32 with scale and shift ``[Cs]`` applied in fp32 on the host, one rounding per operation:
    mean and order statistics ``v * s + t``, the spread ``v * s``, the counts as they are."""
    out = np.array(plain, dtype=np.float32)
    s, t = (np.asarray(a, dtype=np.float32).reshape(1, -1, 1, 1) for a in (scale, shift))
    for i, kind in enumerate(kinds):
        if kind <= ORDER:
            out[:, i] = out[:, i] * s
            if kind != STD:
                out[:, i] = out[:, i] + t
    return out


def as_bf16(a):
    """fp32 numpy rounded to bf16 (to nearest even), as fp32 numpy."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def assert_same_bits(got, want, what=""):
    """Equal bit for bit outside NaN, NaN at the same places."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN pattern")
    assert np.array_equal(bits(got[~nan]), bits(want[~nan])), (what, "bits differ")
