"""Checks of the checker of the metric sums (tests/metrics_checks.py), without a GPU: an fp32 emulation of how ``geo_sums_kernel``
adds a row -- every lane in the kernel's order, vector body behind a scalar head or the whole row scalar -- meets the bound
against the exact sums for the three input families, stays under half of it, and misses it in all five sums once the last
point of every row is dropped.  ``row_plan`` is checked against alignments worked out by hand."""
import numpy as np
import pytest

import metrics_checks as mc

# (head, vector row, bf16 prediction, with climatology)
CONFIGS = [(0, True, False, True), (3, True, False, True), (7, True, True, True), (0, False, False, True), (5, False, True, True),
           (2, True, False, False), (0, False, True, False)]
WORST = {}


@pytest.mark.parametrize("family", mc.FAMILIES)
@pytest.mark.parametrize("W", [1, 5, 9, 61, 513, 1441])
def test_emulated_row_sums_meet_the_bound(W, family):
    C, H = 2, 3
    worst, nearest = 0.0, np.inf
    for seed, (head, vec, bf16, with_clim) in enumerate(CONFIGS):
        prd, tar, clim, wrow = mc.fields(family, (1, C, H, W), 10 * W + seed, bf16)
        clim = clim if with_clim else None
        truth, mag = mc.exact_sums(prd, tar, clim, wrow)
        truth, mag = truth[0], mag[0]
        assert np.array_equal(truth[:, [0, 1, 3, 4]], mag[:, [0, 1, 3, 4]]) and (np.abs(truth[:, 2]) <= mag[:, 2]).all()
        bound = mc.sums_bound(mag, H, W)
        got = mc.emulated_sums(prd[0], tar[0], clim, wrow, head, vec)
        ratio = np.abs(got - truth) / bound
        assert (ratio <= 1.0).all(), f"head {head} vec {vec} bf16 {bf16} clim {with_clim}: {ratio}"
        worst = max(worst, float(ratio.max()))
        # the sums without the last point of every row lie outside, all five
        short = mc.emulated_sums(prd[0][..., :W - 1], tar[0][..., :W - 1], None if clim is None else clim[..., :W - 1], wrow,
                                 head, vec)
        miss = np.abs(short - truth) / bound
        assert (miss > 1.0).all(), f"head {head} vec {vec} bf16 {bf16} clim {with_clim}: a dropped point within the bound: {miss}"
        nearest = min(nearest, float(miss.min()))
    print(f"W = {W} family ({family}): worst error / bound {worst:.3f}, nearest dropped point {nearest:.1f}")
    assert worst < 0.5


def test_family_c_has_a_small_s2_against_large_terms():
    prd, tar, clim, wrow = mc.fields("c", (1, 1, 3, 1441), 5)
    truth, mag = mc.exact_sums(prd, tar, clim, wrow)
    assert abs(truth[0, 0, 2]) < 0.1 * mag[0, 0, 2]
    prd, tar, clim, wrow = mc.fields("b", (1, 1, 3, 61), 5)
    assert np.abs(clim).min() > 100 * np.abs(tar[0] - clim).max() / 6


def test_exact_sums_against_float64():
    prd, tar, clim, wrow = mc.fields("a", (2, 3, 4, 9), 1)
    w = wrow.astype(np.float64).reshape(1, 1, -1, 1)
    p, t = prd.astype(np.float64), tar.astype(np.float64)
    for c in (clim, None):
        cc = 0.0 if c is None else c.astype(np.float64)[None]
        terms = [np.abs(p - t), (p - t) ** 2, (p - cc) * (t - cc), (p - cc) ** 2, (t - cc) ** 2]
        got, mag = mc.exact_sums(prd, tar, c, wrow)
        assert got.shape == mag.shape == (2, 3, 5)
        for k in range(5):
            np.testing.assert_allclose(got[..., k], (w * terms[k]).sum((-2, -1)), rtol=1e-13, atol=1e-13)
            np.testing.assert_allclose(mag[..., k], (w * np.abs(terms[k])).sum((-2, -1)), rtol=1e-13)


def test_to_bf16_rounds_to_nearest_even():
    import torch
    a = np.random.default_rng(0).standard_normal(4096).astype(np.float32) * 1e3
    want = torch.from_numpy(a).to(torch.bfloat16).float().numpy()
    assert np.array_equal(mc.to_bf16(a), want)


def test_row_plan_by_hand():
    base = 1 << 20
    # one sample, fp32, W = 9: row h starts h * 9 floats in, so heads are (4 - (off + 9 h) % 4) % 4
    head, vec = mc.row_plan(base + 4, base, base + 16, 4, 1, 1, 4, 9)
    assert head.shape == (1, 1, 4) and head[0, 0].tolist() == [3, 2, 1, 0]
    # the target is one float behind the prediction: never aligned together
    assert not vec.any()
    head, vec = mc.row_plan(base + 4, base + 4, base + 4, 4, 1, 1, 4, 9)
    assert vec.all()
    head, vec = mc.row_plan(base + 4, base + 4, base, 4, 1, 1, 4, 9)
    assert not vec.any()
    assert mc.row_plan(base + 4, base + 4, None, 4, 1, 1, 4, 9)[1].all()
    # two samples whose stride is 2 floats modulo 4: the second sample is never aligned where the first is
    assert not mc.row_plan(base, base, None, 4, 2, 2, 5, 1441)[1].any()
    # three samples: a pass of two and a ragged pass of one, which vectorises where the pair cannot
    head, vec = mc.row_plan(base, base, None, 4, 3, 1, 33, 61)
    assert head.shape == (2, 1, 33) and not vec[0].any() and vec[1].all()
    # bf16: the head counts 2-byte points, up to 7; the fp32 target agrees when the offsets agree modulo 4
    head, vec = mc.row_plan(base + 2, base + 4, None, 2, 1, 1, 2, 16)
    assert head[0, 0].tolist() == [7, 7] and vec.all()
    assert not mc.row_plan(base + 6, base + 4, None, 2, 1, 1, 2, 16)[1].any()
    # a row shorter than its head
    assert mc.row_plan(base + 4, base + 4, None, 4, 1, 1, 1, 2)[0].tolist() == [[[2]]]
