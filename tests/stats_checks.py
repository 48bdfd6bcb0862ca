"""Shared checks of the dataset-statistics tests (a plain module, imported by test_stats_cpu.py and test_stats_gpu.py).

The criterion for every sum of ``mk_field_stats`` / ``ops.field_stats``: the truth is the EXACT value of the sum over the
fp32 inputs -- every fp32 number is an integer multiple of 2^-149, so the terms ``w d``, ``w d^2``, ``w e``, ``w e^2``, ``m``,
``m^2`` are formed and added as python integers and rounded once at the end -- and a result may be off by at most

    (N + 3) * 2^-53 * sum |term|,        N the number of terms,

which is the bound of recursive summation in ANY order (N - 1 additions, each a relative 2^-53 of a partial sum that is at
most ``sum |term|``) plus the three roundings a term can meet before it is added: the difference, the square (or the
product with the weight) and the weight.  Derived, not measured.  ``test_stats_cpu.py`` shows that a defect lies far
outside it: a dropped row, a dropped tail column, a dropped first difference.
"""
import numpy as np

U = 2.0 ** -53
_ONE = 1 << 149


def to_int(a):
    """``a * 2^149`` as python integers (an object array of the same shape); ``a`` holds fp32 values."""
    a = np.asarray(a)
    assert np.isfinite(a).all()
    flat = np.empty(a.size, dtype=object)
    for i, v in enumerate(a.astype(np.float64).ravel().tolist()):
        n, d = v.as_integer_ratio()
        flat[i] = n * (_ONE // d)
    return flat.reshape(a.shape)


def _total(terms, bits):
    """(exact sum rounded once, sum of magnitudes, number of terms) of integer terms at scale 2^-bits."""
    if terms.size == 0:
        return 0.0, 0.0, 0
    return int(terms.sum()) / (1 << bits), int(np.abs(terms).sum()) / (1 << bits), terms.size


def exact_sums(x, prev, pivot, wrow):
    """Per channel the four sums of ``mk_field_stats`` as [(truth, sum |term|, N)] * 4: ``x`` [T, C, H, W] fp32 numpy,
    ``prev`` [C, H, W] or None, ``pivot`` [C] or None, ``wrow`` [H]."""
    T, C, H, W = x.shape
    xi, wi = to_int(x), to_int(wrow).reshape(1, H, 1)
    pi = to_int(pivot) if pivot is not None else [0] * C
    out = []
    for c in range(C):
        d = xi[:, c] - pi[c]
        seq = xi[:, c] if prev is None else np.concatenate([to_int(prev[c])[None], xi[:, c]], axis=0)
        e = seq[1:] - seq[:-1]
        wd, we = wi * d, wi * e
        out.append([_total(wd, 298), _total(wd * d, 447), _total(we, 298), _total(we * e, 447)])
    return out


def wind_magnitude(x, u, v):
    """fp32 ``sqrt(u u + v v)`` with one rounding per operation and a correctly rounded root (numpy's)."""
    a, b = x[:, u].astype(np.float32), x[:, v].astype(np.float32)
    return np.sqrt(a * a + b * b)


def exact_wind_sums(x, u, v):
    """[(truth, sum |term|, N)] * 2 for the unweighted sums of the magnitude and of its square."""
    m = to_int(wind_magnitude(x, u, v))
    return [_total(m, 149), _total(m * m, 298)]


def bound(mag, n):
    return (n + 3) * U * mag


def check_sum(got, truth, mag, n, what):
    """Asserts ``|got - truth| <= (n + 3) 2^-53 mag`` (exact zero for no terms); returns the ratio of error to bound."""
    err, b = abs(float(got) - truth), bound(mag, n)
    if b == 0.0:
        assert err == 0.0, f"{what}: {got!r} for an empty or all-zero sum"
        return 0.0
    assert err <= b, f"{what}: got {float(got)!r}, exact {truth!r}, error {err:.3e} over the bound {b:.3e} ({err / b:.2f} x, N = {n})"
    return err / b


def sequential_time_sum(start, x):
    """``(..((start + x_0) + x_1) ..)`` in float64, the formulation ``tsum`` must equal bit for bit."""
    ts = np.array(start, dtype=np.float64, copy=True)
    for t in range(x.shape[0]):
        ts = ts + x[t].astype(np.float64)
    return ts
