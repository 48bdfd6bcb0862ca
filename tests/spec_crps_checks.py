"""What the tests of the spectral ensemble CRPS share (a plain module, imported by tests/test_spec_crps_cpu.py,
tests/test_spec_crps_dist_cpu.py and tests/test_spec_crps_gpu.py): packed spectra as numpy arrays, references that share no
step with the kernels, and bounds derived from the operands.

The quantity.  ``cp`` ``[L, M, B E C]`` complex64 (row ``(b E + e) C + c``) are the members' packed spectra, ``ct`` ``[L, M, B C]``
the target's, of the global degrees ``l_off + l`` and orders ``m_off + m``; only ``l_off + l >= m_off + m`` is stored.  Per stored
coefficient, ``(b, c)`` and component ``k`` in (re, im): ``a_k = (1/E) sum_e |x_e - y|``, ``g_k = (1/E^2) sum_ef |x_e - x_f|`` and

    S[bc, l, 0] = sum_m w (a_re + a_im),   S[bc, l, 1] = sum_m w (g_re + g_im),   w(0) = 1, w(m > 0) = 2.

References.  ``sums`` forms ``g`` from the SORTED differences ``d_(i)`` of the members to the target, ``g = (2/E^2) sum_i (2 i - E + 1) d_(i)``
(no pair is ever formed), in numpy's extended precision (asserted below to carry at least 64 significant bits), so that the
cancellation between the rank weights, which the all-pairs form does not have, stays 2^-11 below the float64 bound.  ``grad``
counts the members below and above each member by COMPARISON, as integers, as ``ens_loss_checks.grad`` does.

Bounds (derived, not tuned).
* Sums: a float64 sum of N non-negative terms in ANY order is off by at most ``(N - 1) 2^-53`` times the sum to first order
  (adding an exact zero, an empty chunk or a fresh accumulator, does not round); every term ``|x - y|`` carries one rounding
  of the subtraction, the scales ``1 / E`` and ``2 / E^2`` one rounding each and one for the product.  ``bound`` allows
  ``(n + 4) 2^-53 sum |terms|`` per ``(b, c, l)`` with ``n`` the number of terms of the all-pairs form over the stored orders:
  ``2 E`` per coefficient for ``S0`` and ``E (E - 1)`` (the pairs ``e < f``, two components) for ``S1``; ``sum |terms|`` is the sum itself.
* Gradient: a float64 value rounded ONCE to fp32: ``(2^-24 + 2^-40) |r|`` per component (``ens_loss_checks.ROUND``), exactly
  zero where the reference is zero (the unstored triangle, ties, the imaginary parts of ``m = 0``), NaN in both components of
  every member of a NaN coefficient."""
import functools

import numpy as np

import ens_loss_checks as lc

U = 2.0 ** -53
LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the sorted-members reference needs numpy's extended precision (x87 long double)"

KINDS = ("normal", "ties", "nan")


def stored_mask(L, M, l_off=0, m_off=0):
    """``[L, M]`` bool: the coefficients the Legendre kernels write."""
    return (np.arange(L)[:, None] + l_off) >= (np.arange(M)[None, :] + m_off)


def order_weights(M, m_off=0):
    return np.where(np.arange(M) + m_off == 0, 1.0, 2.0)


def nan_points(dims, l_off=0, m_off=0):
    """The NaN coefficients of ``kind="nan"``: ``((l, m, b, c), "member" | "target")``: the real part of the LAST member at the
    last stored coefficient of the last degree (sample 0, channel 0) and the imaginary part of the target at the first stored
    coefficient (last sample, last channel)."""
    L, M, B, E, C = dims
    st = stored_mask(L, M, l_off, m_off)
    assert st.any(), "nothing stored in this shard"
    rows = np.nonzero(st.any(axis=1))[0]
    return [((L - 1, int(np.nonzero(st[L - 1])[0][-1]), 0, 0), "member"), ((int(rows[0]), 0, B - 1, C - 1), "target")]


@functools.lru_cache(maxsize=None)
def problem(dims, kind="normal", l_off=0, m_off=0, seed=0):
    """``(cp [L, M, B E C] complex64, ct [L, M, B C] complex64, gs [B C, L, 2] float64)`` for ``dims = (L, M, B, E, C)``.
    ``"normal"``: the target N(0, 1) per component, the members the target plus 0.5 N(0, 1); the global coefficient (0, 0), where
    the shard holds it, is temperature-like: 250 +- 1.  ``"ties"``: integer components in -2 ... 2.  ``"nan"``: ``"normal"`` with the
    coefficients of ``nan_points``.  The imaginary parts of global order 0 are zero, the unstored triangle is NaN in every
    kind.  ``gs`` is random with a zero and a negative entry.  Shared between tests: do not write to the arrays."""
    L, M, B, E, C = dims
    rng = np.random.default_rng(seed + 131 * E + 7 * l_off + 3 * m_off + sum(dims))
    if kind == "ties":
        y = rng.integers(-2, 3, size=(2, L, M, B, 1, C)).astype(np.float64)
        x = rng.integers(-2, 3, size=(2, L, M, B, E, C)).astype(np.float64)
    else:
        y = rng.standard_normal((2, L, M, B, 1, C))
        x = y + 0.5 * rng.standard_normal((2, L, M, B, E, C))
        if l_off == 0 and m_off == 0:
            y[0, 0, 0] = 250.0 + rng.uniform(-1, 1, size=(B, 1, C))
            x[0, 0, 0] = 250.0 + rng.uniform(-1, 1, size=(B, E, C))
    if m_off == 0:
        y[1, :, 0] = 0.0
        x[1, :, 0] = 0.0
    x, y = x.astype(np.float32), y.astype(np.float32)
    if kind == "nan":
        for (l, m, b, c), where in nan_points(dims, l_off, m_off):
            if where == "member":
                x[0, l, m, b, E - 1, c] = np.nan
            else:
                y[1, l, m, b, 0, c] = np.nan
    hole = ~stored_mask(L, M, l_off, m_off)
    x[:, hole] = np.nan
    y[:, hole] = np.nan
    cp = (x[0] + 1j * x[1]).astype(np.complex64).reshape(L, M, B * E * C)
    ct = (y[0] + 1j * y[1]).astype(np.complex64).reshape(L, M, B * C)
    gs = rng.standard_normal((B * C, L, 2))
    gs.reshape(-1)[0] = 0.0
    gs.reshape(-1)[1] = -abs(gs.reshape(-1)[1]) - 0.5
    for a in (cp, ct, gs):
        a.setflags(write=False)
    return cp, ct, gs


def components(cp, ct, dims):
    """``(x [2, L, M, B, E, C], y [2, L, M, B, 1, C])`` float32: the (re, im) components of the members and the target."""
    L, M, B, E, C = dims
    x = np.stack([cp.real, cp.imag]).reshape(2, L, M, B, E, C)
    y = np.stack([ct.real, ct.imag]).reshape(2, L, M, B, 1, C)
    return x, y


def _degree_sums(term, L, M, l_off, m_off):
    """``sum_m w (term_re + term_im)`` over the stored orders: ``term`` ``[2, L, M, B, C]`` -> ``[B C, L]`` (same dtype)."""
    st = stored_mask(L, M, l_off, m_off)[:, :, None, None]
    w = order_weights(M, m_off).astype(term.dtype)[None, :, None, None]
    t = np.where(st, term[0] + term[1], 0) * w
    return np.moveaxis(t.sum(axis=1), 0, -1).reshape(-1, L)           # [B, C, L] -> [B C, L]


def sums(cp, ct, dims, l_off=0, m_off=0):
    """``S`` ``[B C, L, 2]`` float64 by the sorted-members identity in extended precision; NaN where a coefficient of ``(b, c, l)`` is."""
    L, M, B, E, C = dims
    x, y = components(cp, ct, dims)
    with np.errstate(invalid="ignore"):
        d = np.sort(x.astype(LD) - y.astype(LD), axis=4)              # NaN sorts last
        a = np.abs(d).sum(axis=4) / LD(E)
        rank = (2 * np.arange(E) - E + 1).astype(LD).reshape(1, 1, 1, 1, E, 1)
        g = (d * rank).sum(axis=4) * (LD(2) / LD(E * E))
        out = np.stack([_degree_sums(a, L, M, l_off, m_off), _degree_sums(g, L, M, l_off, m_off)], axis=-1)
    return out.astype(np.float64)


def stored_counts(L, M, l_off=0, m_off=0):
    """``[L]``: the number of stored orders of every local degree."""
    return stored_mask(L, M, l_off, m_off).sum(axis=1)


def bound(want, dims, l_off=0, m_off=0):
    """``(n + 4) 2^-53 sum |terms|`` per element of ``want`` ``[B C, L, 2]`` (the module docstring); NaN where ``want`` is."""
    L, M, B, E, C = dims
    nm = stored_counts(L, M, l_off, m_off).astype(np.float64)
    n = np.stack([2 * E * nm, E * (E - 1) * nm], axis=-1)[None]      # [1, L, 2]
    return (n + 4) * U * np.abs(want)


def assert_sums(got, cp, ct, dims, l_off=0, m_off=0, what="", want=None):
    """``got`` ``[B C, L, 2]`` against ``sums`` within ``bound``; NaN exactly where the reference is; exactly zero for the degrees
    with nothing stored.  Prints the worst error over the bound before it asserts and returns it."""
    got = np.asarray(got, dtype=np.float64)
    want = sums(cp, ct, dims, l_off, m_off) if want is None else want
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN pattern", int(np.isnan(got).sum()), int(nan.sum()))
    lim = bound(want, dims, l_off, m_off)
    empty = np.broadcast_to((stored_counts(dims[0], dims[1], l_off, m_off) == 0)[None, :, None], want.shape)
    assert (got[empty] == 0).all(), (what, "a degree with nothing stored is not zero")
    rest = ~nan & (want != 0)
    assert (got[~nan & (want == 0)] == 0).all(), (what, "not zero where every term is zero")
    err = np.abs(got - want)[rest]
    worst = float((err / lim[rest]).max()) if err.size else 0.0
    print(f"{what}: worst sum error / bound = {worst:.3e} over {err.size} sums, {int(nan.sum())} NaN")
    assert worst <= 1.0, (what, worst)
    return worst


def bad_coefficients(cp, ct, dims):
    """``[L, M, B, C]`` bool: a component of the target or of a member is NaN (the unstored triangle included)."""
    x, y = components(cp, ct, dims)
    return np.isnan(x).any(axis=(0, 4)) | np.isnan(y).any(axis=(0, 4))


def grad(cp, ct, gs, dims, l_off=0, m_off=0, by_sorted_index=False):
    """The gradient of ``sum gs S`` with respect to ``cp``, complex128 ``[L, M, B E C]`` (``d/d re + i d/d im``): per component
    ``w (gs0 sgn(x_e - y) / E + gs1 2 (L_e - G_e) / E^2)`` with the counts by comparison; zero in the unstored triangle, NaN in
    both components of every member of a NaN coefficient.  ``by_sorted_index``: the WRONG gradient that differentiates the
    sorted form (``2 i - E + 1`` of the member's position in a stable sort), which hands tied members different values."""
    L, M, B, E, C = dims
    x, y = components(cp, ct, dims)
    with np.errstate(invalid="ignore"):
        if by_sorted_index:
            pos = np.argsort(np.argsort(x, axis=4, kind="stable"), axis=4, kind="stable")
            diff = 2 * pos - E + 1
        else:
            lo, hi = np.zeros(x.shape, dtype=np.int64), np.zeros(x.shape, dtype=np.int64)
            for f in range(E):
                lo += x[:, :, :, :, f:f + 1] < x
                hi += x[:, :, :, :, f:f + 1] > x
            diff = lo - hi
        sg = (x > y).astype(np.int64) - (x < y).astype(np.int64)
    g = np.moveaxis(np.asarray(gs, dtype=np.float64).reshape(B, C, L, 2), 2, 0)[:, None, :, None]     # [L, 1, B, 1, C, 2]
    w = order_weights(M, m_off).reshape(1, M, 1, 1, 1)
    r = w * (g[..., 0] * sg / E + g[..., 1] * (2 * diff) / (E * E))                                # [2, L, M, B, E, C]
    st = stored_mask(L, M, l_off, m_off)[None, :, :, None, None, None]
    bad = bad_coefficients(cp, ct, dims)[None, :, :, :, None, :]
    r = np.where(st, np.where(bad, np.nan, r), 0.0)
    return (r[0] + 1j * r[1]).reshape(L, M, B * E * C)


def assert_grad(got, cp, ct, gs, dims, l_off=0, m_off=0, what=""):
    """``got`` complex ``[L, M, B E C]`` against ``grad``, per component: NaN exactly where the reference is, exactly zero where it
    is zero, ``|got - r| <= (2^-24 + 2^-40) |r|`` elsewhere.  Prints the worst error over the bound before it asserts."""
    want = grad(cp, ct, gs, dims, l_off, m_off)
    got = np.asarray(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    got = np.stack([got.real, got.imag]).astype(np.float64)
    want = np.stack([want.real, want.imag])
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN pattern", int(np.isnan(got).sum()), int(nan.sum()))
    zero = (want == 0) & ~nan
    assert (got[zero] == 0).all(), (what, "not zero where the reference is", int((got[zero] != 0).sum()))
    rest = ~nan & ~zero
    lim = (lc.ROUND["float32"] + 2.0 ** -40) * np.abs(want)
    err = np.abs(got - want)[rest]
    worst = float((err / lim[rest]).max()) if err.size else 0.0
    print(f"{what}: worst gradient error / bound = {worst:.3e} over {err.size} components, {int(zero.sum())} exact zeros, {int(nan.sum())} NaN")
    assert worst <= 1.0, (what, worst)
    return worst


def emulate_sums(cp, ct, dims, l_off=0, m_off=0, chunk=16, skip_order=None, w0=1.0, member_major=True):
    """The forward kernel's arithmetic in numpy float64, addition by addition in its order: per coefficient and component
    ``sum_e |x_e - y|`` in ascending e and ``sum_{e < f} |x_e - x_f|`` in lexicographic (e, f), re + im, ``acc += w (.)`` in ascending m
    within chunks of ``chunk`` local orders, the chunks in ascending order, times ``1 / E`` and ``2 / E^2``.  The keyword arguments
    plant the errors the tests must see: ``skip_order`` (a local order left out), ``w0`` (the weight of global order 0) and
    ``member_major=False`` (the members of a (b, c) read at the neighbour's stride: row ``(b C + c) E + e``)."""
    L, M, B, E, C = dims
    if member_major:
        x, y = components(cp, ct, dims)
    else:
        x = np.moveaxis(np.stack([cp.real, cp.imag]).reshape(2, L, M, B, C, E), -1, -2)
        y = np.stack([ct.real, ct.imag]).reshape(2, L, M, B, 1, C)
    x, y = x.astype(np.float64), y.astype(np.float64)
    st = stored_mask(L, M, l_off, m_off)
    total = np.zeros((2, L, B, C))
    with np.errstate(invalid="ignore"):
        for m0 in range(0, M, chunk):
            acc = np.zeros((2, L, B, C))
            for m in range(m0, min(m0 + chunk, M)):
                if m == skip_order:
                    continue
                a, g = np.zeros((2, L, B, C)), np.zeros((2, L, B, C))
                for e in range(E):
                    a = a + np.abs(x[:, :, m, :, e] - y[:, :, m, :, 0])
                for e in range(E):
                    for f in range(e + 1, E):
                        g = g + np.abs(x[:, :, m, :, e] - x[:, :, m, :, f])
                bad = (np.isnan(x[:, :, m]).any(axis=(0, 3)) | np.isnan(y[:, :, m, :, 0]).any(axis=0))
                w = w0 if m_off + m == 0 else 2.0
                t = np.stack([np.where(bad, np.nan, a[0] + a[1]), np.where(bad, np.nan, g[0] + g[1])])
                acc = np.where(st[None, :, m, None, None], acc + w * t, acc)
            total = total + acc
    out = np.stack([total[0] * (1.0 / E), total[1] * (2.0 / (E * E))], axis=-1)          # [L, B, C, 2]
    return np.moveaxis(out, 0, 2).reshape(B * C, L, 2)


def loss_bound(want, dims, chw, kappa, l_off=0, m_off=0):
    """What ``sum_bc chw_c (S0 - kappa / 2 S1)`` (degree weights one, scale one) may be off by when the sums keep ``bound``."""
    L, M, B, E, C = dims
    lim = bound(want, dims, l_off, m_off).reshape(B, C, L, 2)
    chw = np.abs(np.asarray(chw, dtype=np.float64)).reshape(1, C, 1)
    return float((chw * (lim[..., 0] + 0.5 * kappa * lim[..., 1])).sum())
