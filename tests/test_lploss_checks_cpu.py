"""Checks of the checker of the Lp-loss sums (tests/lploss_checks.py), without a GPU: an fp32 emulation of how
``geo_lp_sums_kernel`` adds a row -- every lane in the kernel's order, vector body behind a scalar head or the whole row scalar --
meets the bound against the exact sums, and a dropped point misses it."""
import numpy as np
import pytest

import lploss_checks as lc

F = np.float32


def fields(shape, seed, bf16=False):
    rng = np.random.default_rng(seed)
    tar = rng.standard_normal(shape).astype(F)
    prd = (0.8 * tar + 0.4 * rng.standard_normal(shape) + 0.1).astype(F)
    if bf16:
        prd = (prd.view(np.uint32) & np.uint32(0xffff0000)).view(F)          # some bf16 numbers
    wrow = (rng.random(shape[1]) + 0.1).astype(F)
    return prd, tar, wrow


@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("W", [1, 3, 5, 7, 9, 61, 513, 1441])
def test_emulated_row_sums_meet_the_bound(W, p):
    C, H = 2, 5
    worst = 0.0
    for seed, (head, vec, bf16) in enumerate([(0, True, False), (3, True, False), (7, True, True), (0, False, False),
                                              (5, False, True)]):
        prd, tar, wrow = fields((C, H, W), 10 * W + seed, bf16)
        truth = lc.exact_sums(prd[None], tar[None], wrow, p)[0]
        got = lc.emulated_sums(prd, tar, wrow, p, head, vec)
        bound = lc.sums_bound(truth, H, W)
        assert (np.abs(got - truth) <= bound).all(), f"head {head} vec {vec}: {np.abs(got - truth) / bound}"
        worst = max(worst, float((np.abs(got - truth) / bound).max()))
        # the sums without the row's last point, or without its first, lie outside
        for cut in (slice(0, W - 1), slice(1, W)):
            if W > 1:
                short = lc.emulated_sums(prd[..., cut], tar[..., cut], wrow, p, head, vec)
                assert (np.abs(short - truth) > bound).all()
    print(f"W = {W} p = {p}: worst error / bound {worst:.3f}")
    assert worst < 0.8


def test_exact_sums_against_float64():
    prd, tar, wrow = fields((3, 4, 9), 1)
    prd, tar = prd[None].repeat(2, 0), tar[None].repeat(2, 0)
    for p in (1, 2):
        want = (wrow.astype(np.float64).reshape(1, 1, -1, 1) * np.abs(prd.astype(np.float64) - tar) ** p).sum((-2, -1))
        got = lc.exact_sums(prd, tar, wrow, p)
        assert got.shape == (2, 3, 2)
        np.testing.assert_allclose(got[..., 0], want, rtol=1e-14)
        assert np.array_equal(got[0], got[1])
