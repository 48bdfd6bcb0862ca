"""``mk_degree_power`` and ``mk_degree_power_bwd`` (csrc/specnorm.hip) held to the three criteria of tests/kernel_checks.py through
the C ABI, on ``packed_spectrum`` (NaN in the triangle the Legendre kernels leave unwritten) placed between NaN bands.

``P[l][bc]`` is held to ``(M + 2) 2^-53 P_exact``: the terms are non-negative and the squares exact in fp64, so of the at most 2 M
additions the M that form ``re^2 + im^2`` round one term each, a relative 2^-53 of ``P`` in all, and the at most M that feed the
accumulators and fold the chunks (the first addition of each chain is to zero and exact) a relative 2^-53 each of a partial sum
that never exceeds the total.  ``P_exact`` adds the exact squares with ``math.fsum`` and rounds once.  The gradient is within one fp32 ulp of the float64 product
``2 w gP c`` on the stored triangle and exactly ``+0`` elsewhere.  ``P``, the workspace and ``gc`` are guarded, ``c`` and ``gP``
come back bit for bit, two calls are bitwise equal.

Shapes (L, M, BC): one element; M = 7, under the unroll of 8; a full chunk of 32; 33, a second chunk of one order; 40 = 32 + 8,
where the unroll fits exactly; 45, remainder 5 with ``BC = 1``.  Offsets (l_off, m_off): (2, 37) cuts the stored orders mid-unroll
and leaves whole rows empty.
"""
import math

import numpy as np
import pytest
import torch

import optim_checks as oc
from kernel_checks import SENTINEL, guarded, poisoned
from stream_checks import bits, stream
from test_specnorm_cpu import packed_spectrum

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (5, 7, 3), (9, 32, 5), (9, 33, 2), (12, 40, 7), (20, 45, 1)]
OFFSETS = [(0, 0), (3, 0), (0, 5), (2, 37)]


def stored(L, M, l_off, m_off):
    l = np.arange(L).reshape(L, 1) + l_off
    m = np.arange(M).reshape(1, M) + m_off
    return l >= m                                                         # [L, M]


def exact_power(c, l_off, m_off):
    """[L, BC] float64: the exact ``sum_m w |c|^2`` over the stored orders, rounded once (the squares of fp32 numbers and their
    doubles are exact in float64; ``math.fsum`` adds without error)."""
    L, M, BC = c.shape
    keep = stored(L, M, l_off, m_off)
    re, im = c.real.astype(np.float64), c.imag.astype(np.float64)
    w = np.where(np.arange(M) + m_off == 0, 1.0, 2.0)
    out = np.zeros((L, BC))
    for l in range(L):
        ms = np.nonzero(keep[l])[0]
        for b in range(BC):
            out[l, b] = math.fsum([w[m] * re[l, m, b] ** 2 for m in ms] + [w[m] * im[l, m, b] ** 2 for m in ms])
    return out


@pytest.mark.parametrize("offs", OFFSETS, ids=lambda o: f"l{o[0]}m{o[1]}")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_degree_power_every_sum(dev, shape, offs):
    from makani_amd import _lib
    lib = _lib.load()
    L, M, BC = shape
    l_off, m_off = offs
    c = packed_spectrum(L, M, BC, l_off, m_off, seed=L * M + BC)
    keep = stored(L, M, l_off, m_off)
    assert bool(torch.isnan(c.real[torch.from_numpy(~keep)]).all())
    want = exact_power(c.numpy(), l_off, m_off)
    cd = poisoned(c, dev)
    nws = lib.mk_degree_power_workspace(L, M, BC)
    assert nws == L * ((M + 31) // 32) * BC
    ws, wchk = guarded((nws,), torch.float64, dev)
    P, pchk = guarded((L, BC), torch.float64, dev)
    runs = []
    for _ in range(2):
        _lib.check(lib.mk_degree_power(cd.data_ptr(), ws.data_ptr(), P.data_ptr(), L, M, BC, l_off, m_off, stream()),
                   "mk_degree_power")
        torch.cuda.synchronize()
        wchk("workspace")
        pchk("P")
        runs.append(P.cpu().numpy())
    assert np.array_equal(runs[0], runs[1]), "the sums of two calls differ"
    assert torch.equal(bits(cd.cpu()), bits(c)), "the spectrum is read-only and was written"
    got = runs[1]
    assert (got[~keep.any(1)] == 0).all(), "a degree with nothing stored is not zero"
    worst = oc.worst_ratio(got, want, (M + 2) * 2.0 ** -53 * want, f"offsets {offs}")
    print("RATIO mk_degree_power", "x".join(map(str, shape)), f"l_off={l_off} m_off={m_off} worst={worst:.3f}")


@pytest.mark.parametrize("offs", OFFSETS, ids=lambda o: f"l{o[0]}m{o[1]}")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_degree_power_gradient_every_element(dev, shape, offs):
    from makani_amd import _lib
    lib = _lib.load()
    L, M, BC = shape
    l_off, m_off = offs
    c = packed_spectrum(L, M, BC, l_off, m_off, seed=L * M + BC)
    g = torch.Generator().manual_seed(31 * L + M)
    gP = (torch.randn(L, BC, generator=g, dtype=torch.float64) * 3.0)
    keep = np.broadcast_to(stored(L, M, l_off, m_off)[:, :, None, None], (L, M, BC, 2))
    w = np.where(np.arange(M) + m_off == 0, 2.0, 4.0).reshape(1, M, 1, 1)
    cr = torch.view_as_real(c).numpy().astype(np.float64)                 # [L, M, BC, 2]
    ref = np.where(keep, w * gP.numpy().reshape(L, 1, BC, 1) * np.where(keep, cr, 0.0), 0.0)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    cd, gd = poisoned(c, dev), poisoned(gP, dev)
    gc, gchk = guarded((L, M, BC), torch.complex64, dev)
    runs = []
    for _ in range(2):
        _lib.check(lib.mk_degree_power_bwd(cd.data_ptr(), gd.data_ptr(), gc.data_ptr(), L, M, BC, l_off, m_off, stream()),
                   "mk_degree_power_bwd")
        torch.cuda.synchronize()
        gchk("gc")
        runs.append(gc.cpu())
    assert torch.equal(bits(runs[0]), bits(runs[1])), "the gradients of two calls differ"
    assert torch.equal(bits(cd.cpu()), bits(c)) and torch.equal(bits(gd.cpu()), bits(gP)), "a read-only input was written"
    got = torch.view_as_real(runs[1]).numpy()
    assert not (got == np.float32(SENTINEL)).any(), "an element of the gradient was not written"
    empty = got.view(np.int32)[~keep]
    assert (empty == 0).all(), f"{int((empty != 0).sum())} elements of the empty triangle are not +0"
    worst = oc.worst_ratio(np.where(keep, got, 0.0), ref, np.where(keep, ulp, 0.0), f"offsets {offs}")
    print("RATIO mk_degree_power_bwd", "x".join(map(str, shape)), f"l_off={l_off} m_off={m_off} worst={worst:.3f}")
