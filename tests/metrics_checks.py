"""Shared checks of the metric-kernel tests (a plain module, imported by test_metrics_checks_cpu.py and
test_metrics_guard_gpu.py): the exact value of the five integrals of ``mk_geo_metric_sums``, the bound a result is held to, an
fp32 emulation of how ``geo_sums_kernel`` (csrc/metrics.hip) adds a row, and the kernel's rule for which rows it vectorises.

Truth.  ``s0 = sum w |p - t|``, ``s1 = sum w (p - t)^2``, ``s2 = sum w (p - c)(t - c)``, ``s3 = sum w (p - c)^2`` and
``s4 = sum w (t - c)^2`` over the fp32 operands (a bf16 prediction as the fp32 number it widens to, no climatology as c = 0) are
formed as python integers (``stats_checks.to_int``) and rounded once.  Next to each stands the magnitude ``mag_k = sum w |term_k|``,
which is the sum itself for every k but 2: the terms of ``s2`` have either sign, and with independent anomalies ``s2`` is a small
difference of large numbers that no bound relative to ``|s2|`` could hold.

Bound, from the arithmetic of ``accum()``.  A lane takes 8 consecutive points per step of the vector body, steps 64 lanes apart,
and at most one point of the scalar head / tail (fewer than 16 points, one per lane); a row that runs scalar gives a lane every
64th point.  So a lane adds at most ``n = 8 ceil(W / 512) + 1 <= W / 64 + 9`` terms in fp32.  A term carries at most ``2u``
(``u = 2^-24``): ``d = p - t``, ``p - c`` and ``t - c`` are each rounded once, and the product and its addition are one fma
(``|d|`` carries ``u``).  A sequential sum of n terms adds ``(n - 1) u`` of the lane's magnitude.  The row's lane sums go into
fp64 with the row's weight by an fma each, ``64 H`` terms per (sample, channel) in a fixed order.  Every sum is held to

    bound_k = ((W / 64 + 10) 2^-24 + 64 H 2^-53) mag_k,

the worst case to first order, not taken from the kernel's output.

Measured on the CPU with the emulation below (tests/test_metrics_checks_cpu.py: W in {1, 5, 9, 61, 513, 1441}, H = 3, the three
input families of ``fields``, fp32 and bf16 predictions, vector rows behind heads of 0, 3 and 7 points and scalar rows):

    worst error / bound of the emulation                          0.184  (W = 1, family (a); 0.02 at W = 1441)
    smallest error / bound with every row's last point dropped    2.4    (W = 1441, family (c); 5.2 in (a), 2.8 in (b);
                                                                          at least 35 at W = 513, 128 at W = 61)

so a result is expected under half the bound, and one dropped point per row lies outside it in every sum at every width,
nearest at the widest row, where a point is the smallest share of the sum (the GPU shapes stop at W = 1441 for that reason).
"""
import numpy as np

import stats_checks as sc

U = 2.0 ** -24
U64 = 2.0 ** -53
F = np.float32
KK = 5
FAMILIES = ("a", "b", "c")


def to_bf16(a):
    """fp32 values rounded to nearest even onto bf16 numbers (held in fp32); finite input."""
    b = np.ascontiguousarray(a, dtype=F).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(F).reshape(np.shape(a))


def fields(family, shape, seed, bf16=False):
    """(prediction, target, climatology, row weights), fp32 numpy, ``shape = (B, C, H, W)``, climatology [C, H, W]:

    (a) the fields of tests/test_metrics_gpu.py: N(0, 1) around a 0.5 N(0, 1) climatology, ``s2`` large and positive;
    (b) a climatology much larger than the anomalies: ``c = 5e4 + 300 N``, ``t = c + 100 N``, ``p = t + 40 N``;
    (c) prediction and target anomalies independent, so ``s2`` is near 0 against large terms."""
    B, C, H, W = shape
    rng = np.random.default_rng(seed)
    n = lambda *s: rng.standard_normal(s)
    if family == "a":
        clim = (0.5 * n(C, H, W)).astype(F)
        tar = (clim + n(B, C, H, W)).astype(F)
        prd = (0.8 * tar + 0.4 * n(B, C, H, W) + 0.1).astype(F)
    elif family == "b":
        clim = (5e4 + 300.0 * n(C, H, W)).astype(F)
        tar = (clim + 100.0 * n(B, C, H, W)).astype(F)
        prd = (tar + 40.0 * n(B, C, H, W)).astype(F)
    else:
        assert family == "c"
        clim = (0.5 * n(C, H, W)).astype(F)
        tar = (clim + n(B, C, H, W)).astype(F)
        prd = (clim + n(B, C, H, W)).astype(F)
    if bf16:
        prd = to_bf16(prd)
    wrow = (rng.random(H) + 0.1).astype(F)
    return prd, tar, clim, wrow


def exact_sums(prd, tar, clim, wrow):
    """(truth, mag), each [B, C, 5] float64: the exact five sums and the exact ``sum w |term|``, rounded once.  ``prd``, ``tar``
    [B, C, H, W], ``clim`` [C, H, W] or None and ``wrow`` [H] hold fp32 values (numpy)."""
    B, C, H, W = prd.shape
    pi, ti, wi = sc.to_int(prd), sc.to_int(tar), sc.to_int(wrow).reshape(1, 1, H, 1)
    ci = sc.to_int(clim)[None] if clim is not None else 0
    d, pa, ta = pi - ti, pi - ci, ti - ci
    terms = (wi * np.abs(d), wi * d * d, wi * pa * ta, wi * pa * pa, wi * ta * ta)
    truth, mag = np.empty((B, C, KK)), np.empty((B, C, KK))
    for k in range(KK):
        bits = 298 if k == 0 else 447
        for b in range(B):
            for c in range(C):
                truth[b, c, k] = int(terms[k][b, c].sum()) / (1 << bits)
                mag[b, c, k] = int(np.abs(terms[k][b, c]).sum()) / (1 << bits)
    return truth, mag


def sums_bound(mag, H, W):
    return ((W / 64 + 10) * U + 64 * H * U64) * mag


def _fma(a, b, c):
    """fp32 ``fmaf(a, b, c)``: the product of two fp32 numbers is exact in float64."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def lane_sums(pr, tr, cr, head, vec):
    """The fp32 sums [64, 5] the lanes of a wave hold after one row of ``geo_sums_kernel``: ``pr`` / ``tr`` / ``cr`` the row's
    prediction, target and climatology (fp32 values, ``cr`` None without one), ``head`` the scalar points in front of the
    prediction's 16-byte boundary, ``vec`` whether the streams agree on it (else the whole row runs scalar)."""
    W = len(pr)
    pr, tr = np.asarray(pr, dtype=F), np.asarray(tr, dtype=F)
    cr = np.zeros(W, dtype=F) if cr is None else np.asarray(cr, dtype=F)
    r = np.zeros((64, KK), dtype=F)

    def accum(lanes, i):
        p, t, c = pr[i], tr[i], cr[i]
        d, pa, ta = p - t, p - c, t - c
        r[lanes, 0] = r[lanes, 0] + np.abs(d)
        r[lanes, 1] = _fma(d, d, r[lanes, 1])
        r[lanes, 2] = _fma(pa, ta, r[lanes, 2])
        r[lanes, 3] = _fma(pa, pa, r[lanes, 3])
        r[lanes, 4] = _fma(ta, ta, r[lanes, 4])

    head = min(head, W)
    nv = (W - head) // 8 if vec else 0
    vend = head + nv * 8 if vec else 0
    for j0 in range(0, nv, 64):
        js = np.arange(j0, min(nv, j0 + 64))
        for e in range(8):
            accum(js - j0, head + 8 * js + e)
    nhead = head if vec else 0
    nscal = nhead + (W - vend)
    for q0 in range(0, nscal, 64):
        qs = np.arange(q0, min(nscal, q0 + 64))
        accum(qs - q0, np.where(qs < nhead, qs, vend + qs - nhead))
    return r


def emulated_sums(prd, tar, clim, wrow, head, vec):
    """[C, 5] for one sample: rows through ``lane_sums``, the fold in float64."""
    C, H, W = prd.shape
    out = np.zeros((C, KK))
    for c in range(C):
        for h in range(H):
            cr = None if clim is None else clim[c, h]
            out[c] += np.float64(wrow[h]) * lane_sums(prd[c, h], tar[c, h], cr, head, vec).astype(np.float64).sum(0)
    return out


def row_plan(pred_ptr, tar_ptr, clim_ptr, itemsize, B, C, H, W):
    """(head, vec), integer / boolean arrays [passes, C, H]: for every row the kernel walks -- a pass is NB = min(B, 2) samples
    that share one walk -- the scalar points in front of the 16-byte boundary of the pass's first prediction row, and whether the
    row is vectorised, by the rule of ``geo_sums_kernel``: every stream of every sample of the pass is 16-byte aligned behind that
    head.  Pointers are addresses; ``itemsize`` is the prediction's (4 or 2); ``clim_ptr`` None or 0 means no climatology."""
    NB = 1 if B == 1 else 2
    HW, CHW = H * W, C * H * W
    passes = range(0, B, NB)
    head = np.zeros((len(passes), C, H), dtype=np.int64)
    vec = np.zeros((len(passes), C, H), dtype=bool)
    for k, b0 in enumerate(passes):
        nb = min(NB, B - b0)
        for c in range(C):
            for h in range(H):
                row = c * HW + h * W
                pr = pred_ptr + ((b0 * C + c) * HW + h * W) * itemsize
                tr = tar_ptr + ((b0 * C + c) * HW + h * W) * 4
                hd = min(((16 - pr % 16) % 16) // itemsize, W)
                ok = not clim_ptr or (clim_ptr + (row + hd) * 4) % 16 == 0
                for b in range(nb):
                    ok = ok and (pr + (b * CHW + hd) * itemsize) % 16 == 0 and (tr + (b * CHW + hd) * 4) % 16 == 0
                head[k, c, h], vec[k, c, h] = hd, ok
    return head, vec
