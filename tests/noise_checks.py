"""The independent restatement of the spherical-noise draw (``mk_noise_spectrum``, ``ops.noise_spectrum``) and the bounds its
tests hold the package to.  Plain numpy: ``uint64`` Philox4x32-10, float64 Box-Muller, the coefficient rule, the AR(1) step.
Nothing here imports ``makani_amd``.

The draw.  For global row ``r``, degree ``gl``, order ``gm`` and step ``T``: the words of Philox4x32-10 with counter
``(r >> 1, gl, gm, T)`` and key ``(seed & 0xffffffff, seed >> 32)``; ``(a, b)`` = words (0, 1) for even ``r``, (2, 3) for odd ``r``;
``u1 = ((a >> 8) + 1) 2^-24``, ``u2 = (b >> 8) 2^-24``, ``rad = sqrt(-2 ln u1)``, ``z = rad (cos 2 pi u2, sin 2 pi u2)``;
``xi = s sigma_l z_re`` for order 0 and ``s sigma_l / sqrt 2 (z_re + i z_im)`` otherwise, zero where ``gl < gm``.

The bound, per element and per component: ``K 2^-24 s sigma_l rad``.  ``u1`` and ``u2`` are exact in fp32 (24-bit integers times a
power of two) and so is ``2 u2``, so the error is that of the fp32 functions and products alone.  In units of ``2^-24`` (one
rounding to nearest is at most one unit, relative), with the accuracy figures of the HIP math functions (``logf`` 1 ulp,
``sincospif`` 2 ulp, ``sqrtf`` correctly rounded; no copy of the HIP documentation was at hand where this was written, the
figures are those the feature was specified with):

* ``rad = sqrtf(-2 logf(u1))``: ``logf`` within 1 ulp is at most 2 units relative, the factor -2 is exact, the square root halves
  an incoming relative error and adds its own rounding: at most 3 units relative to ``rad``;
* ``sincospif`` within 2 ulp of a value of magnitude at most 1, whose ulp is at most ``2^-23``: at most 4 units, absolute, and
  so 4 units of ``rad`` after the product;
* the product ``rad * c``: 1 unit.

That is 8 to first order; ``K_NORMAL = 10`` is the figure the feature was specified with and leaves 2 units for the
second-order terms.  The coefficient adds the rounding of the ``sigma_l / sqrt 2`` entry (1), its product with the normal (1)
and, with a row scale, the product ``s * entry`` (1): 11 to first order, ``K_COEF = 12``.  The bound is stated with ``sigma_l``,
not ``sigma_l / sqrt 2``, for every order.  The tests check that it is not vacuous: a draw with the real and imaginary parts
swapped, without the ``1 / sqrt 2``, or with the odd row on words (0, 1) falls outside it.

The AR(1) step ``S' = fl(fl(phi S) + fl(c xi))`` with ``c = fl(sqrt(1 - phi^2))`` is restated exactly (``phi`` the fp32 value, ``c``
unrounded).  Its error is ``phi`` times the error of ``S``, ``c`` times the bound of ``xi``, and one unit each for the product
``phi S``, the rounding of ``c``, the product ``c xi`` and the sum: ``2^-24 (|phi S| + 2 |c xi| + |S'|)`` per component, inflated by
``1 + 2^-16`` for the second-order terms (the roundings act on the computed values, not the exact ones).
"""
import numpy as np

U = 2.0 ** -24
K_NORMAL, K_COEF = 10.0, 12.0
SEEDS = (0, 0x9E3779B97F4A7C15)
_M0, _M1, _W0, _W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), 0x9E3779B9, 0xBB67AE85
_MASK, _32 = np.uint64(0xFFFFFFFF), np.uint64(32)

KNOWN_ANSWERS = [      # (counter, key, words): the Random123 known-answer vectors of philox4x32-10
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays that hold 32-bit values (broadcast against each other): the four output words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3))
    k0, k1 = int(k0), int(k1)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                          # below 2^64: both factors are below 2^32
        c0, c1, c2, c3 = (p1 >> _32) ^ c1 ^ np.uint64(k0), p1 & _MASK, (p0 >> _32) ^ c3 ^ np.uint64(k1), p0 & _MASK
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def words(seed, q, l, m, t):
    """The four words of counter (q, l, m, t) under ``seed`` as Python ints."""
    return [int(w) for w in philox(q, l, m, t, seed & 0xFFFFFFFF, seed >> 32)]


def restate(sigma32, L, M, BC, seed, T, l_off=0, m_off=0, row0=0, row_scale=None, variant=None):
    """The draw of a shard in float64: ``(xi complex128 [L, M, BC], bound float64 [L, M, BC], rad [L, M, BC])``; the bound is zero
    where the entry must be an exact zero.  ``sigma32``: the fp32 ``[L]`` table the package was given.  ``variant`` makes a wrong
    draw on purpose (``"swap"``: real and imaginary parts exchanged; ``"nosqrt2"``: no ``1 / sqrt 2``; ``"odd01"``: the odd row takes
    words (0, 1) like the even one)."""
    assert row0 % 2 == 0
    rows = row0 + np.arange(BC, dtype=np.uint64)
    q = (rows >> np.uint64(1)).reshape(1, 1, BC)
    gl = (l_off + np.arange(L, dtype=np.uint64)).reshape(L, 1, 1)
    gm = (m_off + np.arange(M, dtype=np.uint64)).reshape(1, M, 1)
    w = [np.broadcast_to(x, (L, M, BC)) for x in philox(q, gl, gm, np.uint64(T & 0xFFFFFFFF), seed & 0xFFFFFFFF, seed >> 32)]
    odd = np.broadcast_to((rows & np.uint64(1)).reshape(1, 1, BC) == 1, (L, M, BC))
    if variant == "odd01":
        odd = np.zeros_like(odd)
    a, b = np.where(odd, w[2], w[0]), np.where(odd, w[3], w[1])
    u1 = ((a >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * U
    u2 = (b >> np.uint64(8)).astype(np.float64) * U
    rad = np.sqrt(-2.0 * np.log(u1))
    z = rad * np.exp(2j * np.pi * u2)
    if variant == "swap":
        z = z.imag + 1j * z.real
    sig = np.asarray(sigma32, dtype=np.float32).astype(np.float64).reshape(L, 1, 1)
    s = np.ones((1, 1, BC)) if row_scale is None else np.asarray(row_scale, dtype=np.float32).astype(np.float64).reshape(1, 1, BC)
    order0 = np.broadcast_to(gm == 0, (L, M, BC))
    xi = np.where(order0, s * sig * z.real + 0j, s * sig * (1.0 if variant == "nosqrt2" else np.sqrt(0.5)) * z)
    valid = np.broadcast_to(gl >= gm, (L, M, BC))
    xi = np.where(valid, xi, 0.0)
    bound = np.where(valid, K_COEF * U * s * sig * rad, 0.0)
    return xi, bound, np.where(valid, rad, 0.0)


def ar1(S, bS, xi, bxi, phi):
    """One AR(1) step restated: ``(S', bound of S')`` from the restated state ``S`` with bound ``bS`` and the restated draw ``xi``
    with bound ``bxi`` (module docstring)."""
    phi = float(np.float32(phi))
    c = np.sqrt(1.0 - phi * phi)
    S1 = phi * S + c * xi

    def comp(f):
        return phi * np.abs(f(S)), c * np.abs(f(xi)), np.abs(f(S1))

    b = np.zeros(S.shape)
    for f in (np.real, np.imag):
        p, x, s1 = comp(f)
        b = np.maximum(b, U * (p + 2.0 * x + s1))
    return S1, (phi * bS + c * bxi + b) * (1.0 + 2.0 ** -16)


def components(y):
    y = np.asarray(y)
    return np.stack([y.real, y.imag], axis=-1).astype(np.float64)


def worst_ratio(y, ref, bound, factor=1.0):
    """The largest ``|y - ref| / (factor * bound)`` over both components of the entries with a bound; entries whose bound is zero
    must be exact zeros (asserted)."""
    y, ref = np.asarray(y), np.asarray(ref)
    assert y.shape == ref.shape == bound.shape, (y.shape, ref.shape, bound.shape)
    assert np.isfinite(components(y)).all(), "a value is not finite"
    zero = bound == 0
    assert (y[zero] == 0).all(), f"{int((y[zero] != 0).sum())} entries that must be exact zeros are not"
    err = np.abs(components(y) - components(ref))[~zero]
    return float((err / (factor * bound[~zero])[..., None]).max()) if err.size else 0.0


def area_variance(x, wlat):
    """Per row of ``x`` ``[rows, nlat, nlon]`` the area-weighted mean of ``x^2`` (``wlat``: quadrature weights of the latitudes)."""
    x = np.asarray(x, dtype=np.float64)
    return ((x ** 2).mean(axis=-1) * (wlat / wlat.sum())[None, :]).sum(axis=-1)
