"""``mk_geo_metric_sums`` (csrc/metrics.hip) held to the three criteria of tests/kernel_checks.py through the C ABI: fp32 and bf16
predictions, with and without climatology, the three input families of tests/metrics_checks.py.

Each of the [B][C][5] sums is held to the derived bound of tests/metrics_checks.py against the exact sum, a bound relative to
``sum w |term|`` and not to the sum, which for ``s2`` of family (c) is near zero.  Prediction, target and climatology each sit 0
and 1 elements past a 16-byte boundary in every combination (bf16: prediction 3 and target 1 as well), which
``metrics_checks.row_plan``, the kernel's rule restated on the host, shows to reach rows vectorised behind a non-empty head and rows
that run wholly scalar.  Inputs lie between NaN bands with a NaN in front of an offset view and must come back bit for bit;
workspace and sums are guarded; two calls are bitwise equal.

Climatology 2 elements off with the other two aligned is there for (3, 1, 33, 61): its ragged last sample starts 2 floats modulo 4
into the field, the climatology row does not, so with offsets of 0 and 1 alone no row of that shape vectorises with a climatology.
(2, 2, 5, 1441) never vectorises: its sample stride is 2 floats modulo 4, so the second sample of the pair is never aligned where
the first is.  (1, 2, 5, 1441) is the same field with one sample, whose rows do take the three 512-point steps of the vector body.
"""
import itertools

import numpy as np
import pytest
import torch

import metrics_checks as mc
import optim_checks as oc
from kernel_checks import guarded
from stream_checks import code, put, stream, unchanged

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1), (1, 2, 3, 5), (2, 3, 17, 7), (3, 2, 16, 9), (3, 1, 33, 61), (2, 2, 5, 1441), (1, 2, 5, 1441)]
BOTH_BRANCHES = [(3, 2, 16, 9), (3, 1, 33, 61), (1, 2, 5, 1441)]      # shapes whose offset matrix must reach both branches
DTYPES = [torch.float32, torch.bfloat16]
_CACHE = {}


def problem(shape, dtype, family):
    key = (shape, dtype, family)
    if key not in _CACHE:
        B, C, H, W = shape
        _CACHE[key] = mc.fields(family, shape, 7000 + 13 * H * W + mc.FAMILIES.index(family), dtype == torch.bfloat16)
    return _CACHE[key]


def truth(shape, dtype, family, with_clim):
    key = (shape, dtype, family, with_clim)
    if key not in _CACHE:
        prd, tar, clim, wrow = problem(shape, dtype, family)
        _CACHE[key] = mc.exact_sums(prd, tar, clim if with_clim else None, wrow)
    return _CACHE[key]


def offsets(dtype):
    combos = list(itertools.product((0, 1), repeat=3)) + [(0, 0, 2)]
    return combos + ([(3, 1, 0), (3, 1, 1)] if dtype == torch.bfloat16 else [])


@pytest.mark.parametrize("family", mc.FAMILIES)
@pytest.mark.parametrize("with_clim", [True, False], ids=["clim", "noclim"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sums_against_the_exact_sums(dev, shape, dtype, with_clim, family):
    from makani_amd import _lib
    lib = _lib.load()
    B, C, H, W = shape
    prd, tar, clim, wrow = problem(shape, dtype, family)
    want, mag = truth(shape, dtype, family, with_clim)
    bound = mc.sums_bound(mag, H, W)
    prd_t = torch.from_numpy(prd).to(dtype)
    assert np.array_equal(prd_t.float().numpy(), prd)                    # the cast loses nothing: bf16 cases hold bf16 numbers
    wd, wwhole, wflat = put(torch.from_numpy(wrow), 0, dev)
    worst, n_vec_head, n_scalar = 0.0, 0, 0
    for po, to, co in offsets(dtype):
        if not with_clim and co:
            continue
        what = f"offsets pred {po} tar {to} clim {co}"
        pd, pwhole, pflat = put(prd_t, po, dev)
        td, twhole, tflat = put(torch.from_numpy(tar), to, dev)
        held = [(pwhole, pflat), (twhole, tflat), (wwhole, wflat)]
        cptr = None
        if with_clim:
            cd, cwhole, cflat = put(torch.from_numpy(clim), co, dev)
            held.append((cwhole, cflat))
            cptr = cd.data_ptr()
        head, vec = mc.row_plan(pd.data_ptr(), td.data_ptr(), cptr, prd_t.element_size(), B, C, H, W)
        n_vec_head += int((vec & (head > 0) & ((W - head) >= 8)).sum())
        n_scalar += int((~vec).sum())
        ws, wchk = guarded((lib.mk_geo_metric_workspace(B, C, H),), torch.float64, dev)
        sums, schk = guarded((B, C, 5), torch.float64, dev)
        runs = []
        for _ in range(2):
            _lib.check(lib.mk_geo_metric_sums(pd.data_ptr(), code(dtype), td.data_ptr(), cptr, wd.data_ptr(), ws.data_ptr(),
                                              sums.data_ptr(), B, C, H, W, stream()), "mk_geo_metric_sums")
            torch.cuda.synchronize()
            wchk(what + ": workspace")
            schk(what + ": sums")
            runs.append(sums.cpu().numpy())
        got = runs[1]
        assert np.array_equal(runs[0], got), f"{what}: the sums of two calls differ"
        for whole, flat in held:
            unchanged(whole, flat, what)
        worst = max(worst, oc.worst_ratio(got, want, bound, what))
    print("RATIO mk_geo_metric_sums", "x".join(map(str, shape)), dtype, f"clim={with_clim} family={family}",
          f"rows vectorised behind a head={n_vec_head} scalar={n_scalar} worst={worst:.3f}")
    if shape in BOTH_BRANCHES:
        assert n_vec_head > 0 and n_scalar > 0, "the offset matrix must reach the vector body behind a head and the scalar walk"
