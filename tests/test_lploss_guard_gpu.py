"""``mk_geo_lp_bwd`` and ``mk_geo_lp_sums`` (csrc/lploss.hip) held to the three criteria of tests/kernel_checks.py through the C
ABI, fp32 and bf16 predictions, p = 1 and 2.

Every element of the gradient is checked (exact ties ``pred == tar`` planted): for p = 1 it is ``+-fl(g w)`` or 0 bit for bit (bf16:
the one rounding of that fp32 number); for p = 2 it is within ``3u |ref|`` of the float64 value (``2 g w`` rounds once, ``p - t``
once, their product once), in bf16 one bf16 ulp on top.  Each of the [B][C][2] sums is held to the derived bound of
tests/lploss_checks.py against the exact sum.  Prediction, target and gradient each sit 0 and 1 elements past a 16-byte boundary
in every combination (vector body behind a scalar head, and rows that run scalar); inputs lie between NaN bands with a NaN in
front of an offset view and must come back bit for bit; gradient, workspace and sums are guarded.  (5, 3, 2200, 3) has 33 000
rows, more than the 32 768 the backward's grid covers in one trip; odd B leaves the sums kernel a ragged last pair of samples.
"""
import itertools

import numpy as np
import pytest
import torch

import lploss_checks as lc
import optim_checks as oc
from kernel_checks import SENTINEL, bf16_elementwise, guarded, poisoned

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1), (1, 2, 3, 5), (2, 3, 17, 7), (3, 2, 16, 9), (2, 2, 5, 1441), (5, 3, 2200, 3)]
DTYPES = [torch.float32, torch.bfloat16]
U = 2.0 ** -24
_CACHE = {}


def problem(shape, dtype):
    """(prediction in ``dtype``, target, row weights, upstream gradient) on the host, with exact ties planted; computed once."""
    key = (shape, dtype)
    if key not in _CACHE:
        B, C, H, W = shape
        g = torch.Generator().manual_seed(1000 + H * W)
        tar = torch.randn(shape, generator=g)
        prd = (0.8 * tar + 0.4 * torch.randn(shape, generator=g) + 0.1).to(dtype)
        flat = tar.view(-1)
        flat[3::7] = prd.view(-1)[3::7].float()                           # exact ties, every seventh element
        wrow = torch.rand(H, generator=g) + 0.1
        up = (torch.rand(B, C, generator=g) + 0.5) * torch.where(torch.rand(B, C, generator=g) < 0.5, -1.0, 1.0)
        _CACHE[key] = (prd, tar, wrow, up)
    return _CACHE[key]


def truth(shape, dtype, p):
    key = (shape, dtype, p)
    if key not in _CACHE:
        prd, tar, wrow, _ = problem(shape, dtype)
        _CACHE[key] = lc.exact_sums(prd.float().numpy(), tar.numpy(), wrow.numpy(), p)
    return _CACHE[key]


def put(t, off, dev):
    """``t`` on the device ``off`` elements past a 16-byte boundary between NaN bands, a NaN in front of an offset view; returns
    (view, whole buffer view, its input) for the comparison after the launch."""
    flat = torch.cat([torch.full((off,), float("nan"), dtype=t.dtype), t.reshape(-1)])
    whole = poisoned(flat, dev)
    return whole[off:].view(t.shape), whole, flat


def unchanged(whole, flat, what):
    kind = torch.int32 if flat.dtype == torch.float32 else torch.int16
    assert torch.equal(whole.cpu().view(kind), flat.view(kind)), f"{what}: a read-only input was written"


def _code(dtype):
    return 0 if dtype == torch.float32 else 1


def _st():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gradient_every_element(dev, shape, dtype, p):
    from makani_amd import _lib
    lib = _lib.load()
    B, C, H, W = shape
    prd, tar, wrow, up = problem(shape, dtype)
    d = prd.float() - tar                                                # the sign of the fp32 difference is exact
    assert int((d == 0).sum()) == len(range(3, d.numel(), 7))
    k = up.view(B, C, 1, 1) * wrow.view(1, 1, H, 1)                       # fl(g w), one fp32 rounding
    if p == 1:
        want = torch.where(d > 0, k, torch.where(d < 0, -k, torch.zeros(()))).to(dtype)
    else:
        ref = 2.0 * up.double().view(B, C, 1, 1) * wrow.double().view(1, 1, H, 1) * (prd.double() - tar.double())
    wd, wwhole, wflat = put(wrow, 0, dev)
    ud, uwhole, uflat = put(up, 0, dev)
    worst = 0.0
    for po, to, go in itertools.product((0, 1), repeat=3):
        what = f"offsets pred {po} tar {to} grad {go}"
        pd, pwhole, pflat = put(prd, po, dev)
        td, twhole, tflat = put(tar, to, dev)
        gbuf, chk = guarded((prd.numel() + go,), dtype, dev)
        gp = gbuf[go:].view(shape)
        assert pd.data_ptr() % 16 == po * prd.element_size() and gp.data_ptr() % 16 == go * prd.element_size()
        _lib.check(lib.mk_geo_lp_bwd(pd.data_ptr(), _code(dtype), td.data_ptr(), wd.data_ptr(), ud.data_ptr(), gp.data_ptr(), p, B, C,
                                     H, W, _st()), "mk_geo_lp_bwd")
        torch.cuda.synchronize()
        chk(what)
        if go:
            assert float(gbuf[0]) == SENTINEL, f"{what}: the element in front of the gradient was written"
        for whole, flat in ((pwhole, pflat), (twhole, tflat), (wwhole, wflat), (uwhole, uflat)):
            unchanged(whole, flat, what)
        got = gp.cpu()
        if p == 1:
            kind = torch.int32 if dtype == torch.float32 else torch.int16
            bad = got.view(kind) != want.view(kind)
            assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements are not +-fl(g w) or 0 bit for bit, the first at " \
                                        f"{tuple(int(i) for i in torch.nonzero(bad)[0])}"
        elif dtype == torch.float32:
            worst = max(worst, oc.worst_ratio(got.numpy(), ref.numpy(), 3 * U * ref.abs().numpy(), what))
        else:
            worst = max(worst, bf16_elementwise(got, ref, 3 * U * ref.abs(), what))
            assert not bool(got[d == 0].any()), f"{what}: a tie must give an exact zero"
    print("RATIO mk_geo_lp_bwd", "x".join(map(str, shape)), dtype, f"p={p} worst={worst:.3f}")


@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sums_against_the_exact_sums(dev, shape, dtype, p):
    from makani_amd import _lib
    lib = _lib.load()
    B, C, H, W = shape
    prd, tar, wrow, _ = problem(shape, dtype)
    want = truth(shape, dtype, p)
    bound = lc.sums_bound(want, H, W)
    wd, wwhole, wflat = put(wrow, 0, dev)
    worst = 0.0
    for po, to in itertools.product((0, 1), repeat=2):
        what = f"offsets pred {po} tar {to}"
        pd, pwhole, pflat = put(prd, po, dev)
        td, twhole, tflat = put(tar, to, dev)
        ws, wchk = guarded((lib.mk_geo_lp_workspace(B, C, H),), torch.float64, dev)
        sums, schk = guarded((B, C, 2), torch.float64, dev)
        runs = []
        for _ in range(2):
            _lib.check(lib.mk_geo_lp_sums(pd.data_ptr(), _code(dtype), td.data_ptr(), wd.data_ptr(), ws.data_ptr(), sums.data_ptr(),
                                          p, B, C, H, W, _st()), "mk_geo_lp_sums")
            torch.cuda.synchronize()
            wchk(what + ": workspace")
            schk(what + ": sums")
            runs.append(sums.cpu().numpy())
        got = runs[1]
        assert np.array_equal(runs[0], got), f"{what}: the sums of two calls differ"
        for whole, flat in ((pwhole, pflat), (twhole, tflat), (wwhole, wflat)):
            unchanged(whole, flat, what)
        worst = max(worst, oc.worst_ratio(got, want, bound, what))
    print("RATIO mk_geo_lp_sums", "x".join(map(str, shape)), dtype, f"p={p} worst={worst:.3f}")
