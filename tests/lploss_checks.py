"""Shared checks of the Lp-loss kernel tests (a plain module, imported by test_lploss_checks_cpu.py and
test_lploss_guard_gpu.py): the exact value of the two integrals of ``mk_geo_lp_sums``, the bound a result is held to, and an fp32
emulation of how ``geo_lp_sums_kernel`` (csrc/lploss.hip) adds a row.

Truth.  ``s0 = sum w |p - t|^P`` and ``s1 = sum w |t|^P`` over the fp32 operands (a bf16 prediction as the fp32 number it
widens to) are formed as python integers (``stats_checks.to_int``: every fp32 number is a multiple of 2^-149) and rounded once.

Bound.  A lane adds its share of a row in fp32 and the row's lane sums go into fp64 with the row's weight.  A lane takes 8
consecutive points per step of the vector body, steps 64 lanes apart, and at most one point of the scalar head / tail (fewer than
16 points, one per lane); a row that runs scalar gives a lane every 64th point.  So a lane adds at most
``n = 8 ceil(W / 512) + 1 < W / 64 + 9`` terms; a sequential fp32 sum of n non-negative terms, the first addition to zero exact,
is off by at most ``(n - 1) u`` of the lane's sum, and a term carries the rounding of ``d = p - t`` (``u`` for ``|d|``, ``2u`` for
``d^2``; the square and its addition are one fma), ``t^2`` and ``|t|`` none.  The worst lane of the worst row therefore stays under
``(W / 64 + 10) u`` of ITS sum, which it reaches only if every rounding goes the same way at full size and all of the row's
magnitude sits in that lane.  The bound the rows are held to spreads the count over the row,

    (W / 64 + 8) 2^-24 sum_row |terms|        per row, times the row's weight,

two roundings under that corner case: the emulation below, with every lane in the kernel's order, reaches 0.13 of it at W = 1 ... 9
(one or two roundings against 8 allowed) and 0.01 on rows of 513 and 1441 points, and a dropped point lies far outside
(tests/test_lploss_checks_cpu.py).  The fp64 fold adds one term per (row, lane) by an fma, in a fixed order of lanes, waves and
slabs: ``n 2^-53`` of the sum for its ``n = 64 H`` terms (any order).
"""
import numpy as np

import stats_checks as sc

U = 2.0 ** -24
U64 = 2.0 ** -53
F = np.float32


def exact_sums(prd, tar, wrow, p):
    """[B, C, 2] float64: the exact ``sum w |prd - tar|^p`` and ``sum w |tar|^p``, rounded once.  ``prd``, ``tar`` [B, C, H, W] and
    ``wrow`` [H] hold fp32 values (numpy)."""
    B, C, H, W = prd.shape
    pi, ti, wi = sc.to_int(prd), sc.to_int(tar), sc.to_int(wrow).reshape(1, 1, H, 1)
    d = np.abs(pi - ti)
    t = np.abs(ti)
    terms = (wi * d, wi * t) if p == 1 else (wi * d * d, wi * t * t)
    bits = 298 if p == 1 else 447
    out = np.empty((B, C, 2), dtype=np.float64)
    for b in range(B):
        for c in range(C):
            for k in range(2):
                out[b, c, k] = int(terms[k][b, c].sum()) / (1 << bits)
    return out


def sums_bound(truth, H, W):
    """Every term is non-negative, so ``sum |terms|`` is the truth itself."""
    return ((W / 64 + 8) * U + 64 * H * U64) * truth


def lane_sums(pr, tr, p, head, vec):
    """The fp32 sums [64, 2] the lanes of a wave hold after one row of ``geo_lp_sums_kernel``: ``pr`` / ``tr`` the row's prediction
    and target (fp32 values), ``head`` the scalar points in front of the 16-byte boundary, ``vec`` whether the streams agree on it
    (else the whole row runs scalar)."""
    W = len(pr)
    pr, tr = np.asarray(pr, dtype=F), np.asarray(tr, dtype=F)
    r = np.zeros((64, 2), dtype=F)

    def accum(lanes, i):
        d = pr[i] - tr[i]
        t = tr[i]
        if p == 2:
            r[lanes, 0] = (d.astype(np.float64) ** 2 + r[lanes, 0].astype(np.float64)).astype(F)
            r[lanes, 1] = (t.astype(np.float64) ** 2 + r[lanes, 1].astype(np.float64)).astype(F)
        else:
            r[lanes, 0] = r[lanes, 0] + np.abs(d)
            r[lanes, 1] = r[lanes, 1] + np.abs(t)

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


def emulated_sums(prd, tar, wrow, p, head, vec):
    """[C, 2] for one sample: rows through ``lane_sums``, the fold in float64."""
    C, H, W = prd.shape
    out = np.zeros((C, 2))
    for c in range(C):
        for h in range(H):
            out[c] += np.float64(wrow[h]) * lane_sums(prd[c, h], tar[c, h], p, head, vec).astype(np.float64).sum(0)
    return out
