"""CPU tests of the per-degree power of a packed spectrum (``ops.degree_power``, torch float64 on CPU tensors) and of
``GeometricH1Loss.norms_from_spectrum`` on the shards of one spectrum.  The packed layout is ``[L, M, BC]`` complex64; the
rows with ``l_off + l < m_off + m`` are the ones the Legendre kernels never write, so they are filled with NaN here and must
not reach any sum."""
import numpy as np
import pytest
import torch

import capi_checks as capi

from makani_amd import ops
from makani_amd.distributed import compute_split_shapes

L, M = 33, 17          # uneven under a 2-way split: 17 + 16 degrees, 9 + 8 orders


def packed_spectrum(nl, nm, bc, l_off=0, m_off=0, seed=0, fill=float("nan")):
    """Random complex64 ``[nl, nm, bc]`` with ``fill`` in the empty triangle of the shard at (l_off, m_off)."""
    g = torch.Generator().manual_seed(seed)
    c = torch.complex(torch.randn(nl, nm, bc, generator=g), torch.randn(nl, nm, bc, generator=g))
    l = torch.arange(nl).reshape(nl, 1) + l_off
    m = torch.arange(nm).reshape(1, nm) + m_off
    c[(l < m).expand(nl, nm)] = complex(fill, fill)
    return c


def degree_power_numpy(c, l_off=0, m_off=0):
    """``[BC, L]`` float64 by the formula: sum over the stored orders of w |c|^2, w(0) = 1, w(m > 0) = 2."""
    c = c.numpy()
    nl, nm, bc = c.shape
    out = np.zeros((bc, nl), dtype=np.float64)
    for l in range(nl):
        for m in range(nm):
            if l_off + l >= m_off + m:
                a = c[l, m].real.astype(np.float64) ** 2 + c[l, m].imag.astype(np.float64) ** 2
                out[:, l] += (1.0 if m_off + m == 0 else 2.0) * a
    return out


def norms_numpy(c, batch, l_off=0, m_off=0):
    p = degree_power_numpy(c, l_off, m_off).reshape(batch, -1, c.shape[0])
    l = np.arange(c.shape[0], dtype=np.float64) + l_off
    return np.stack([p.sum(axis=(1, 2)), (p * (l * (l + 1))).sum(axis=(1, 2))], axis=-1)


@pytest.mark.parametrize("shape", [(5, 7, 3), (33, 17, 6), (1, 1, 1)])
@pytest.mark.parametrize("offs", [(0, 0), (16, 0), (0, 5), (16, 33)])
def test_degree_power_cpu_matches_numpy(shape, offs):
    c = packed_spectrum(*shape, *offs, seed=3)
    got = ops.degree_power(c, *offs)
    want = degree_power_numpy(c, *offs)
    assert got.dtype == torch.float64 and tuple(got.shape) == (shape[2], shape[0])
    assert torch.isfinite(got).all()
    assert np.abs(got.numpy() - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300)


def test_degree_power_cpu_gradient_ignores_the_empty_triangle():
    offs = (2, 4)
    c = packed_spectrum(6, 7, 3, *offs, seed=5).requires_grad_(True)
    g = torch.randn(3, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(6))
    (ops.degree_power(c, *offs) * g).sum().backward()
    cd = c.detach()
    l = torch.arange(6).reshape(6, 1, 1) + offs[0]
    m = torch.arange(7).reshape(1, 7, 1) + offs[1]
    w = torch.where(m == 0, 1.0, 2.0).double()
    k = 2 * w * g.t().reshape(6, 1, 3)
    stored = (l >= m).expand(6, 7, 3)
    want = torch.where(stored, torch.complex((k * cd.real.double()).float(), (k * cd.imag.double()).float()),
                       torch.zeros_like(cd))
    assert torch.equal(c.grad[~stored], torch.zeros_like(c.grad[~stored]))
    assert (c.grad[stored] - want[stored]).abs().max() <= 1e-6 * want[stored].abs().max()


def test_degree_power_rejects_bad_input():
    with pytest.raises(ValueError):
        ops.degree_power(torch.zeros(3, 4, 5))
    with pytest.raises(ValueError):
        ops.degree_power(torch.zeros(3, 4, dtype=torch.complex64))
    with pytest.raises(ValueError):
        ops.degree_power(torch.zeros(3, 4, 5, dtype=torch.complex64), -1, 0)


@pytest.mark.parametrize("lsplit,msplit", [(2, 1), (1, 2), (2, 2)])
def test_norms_from_spectrum_adds_up_over_shards(lsplit, msplit):
    from makani_amd.losses import GeometricH1Loss
    batch, chans = 2, 3
    loss = GeometricH1Loss((L, 2 * (M - 1)))
    assert (loss.sht.lmax, loss.sht.mmax) == (L, M)
    c = packed_spectrum(L, M, batch * chans, seed=11)
    whole = loss.norms_from_spectrum(c, batch)
    assert whole.dtype == torch.float64 and tuple(whole.shape) == (batch, 2)
    want = norms_numpy(c, batch)
    assert np.abs(whole.numpy() / want - 1).max() <= 1e-12
    ls, ms = compute_split_shapes(L, lsplit), compute_split_shapes(M, msplit)
    total = torch.zeros_like(whole)
    for i in range(lsplit):
        for j in range(msplit):
            l0, m0 = sum(ls[:i]), sum(ms[:j])
            shard = c[l0:l0 + ls[i], m0:m0 + ms[j]].contiguous()
            total = total + loss.norms_from_spectrum(shard, batch, l0, m0)
    assert ((total - whole).abs() <= 1e-12 * whole.abs()).all()


# ---------------------------------------------------------------------------------------------------------------------
# misaligned pointers: refused by the host checks, with the message of the check (tests/capi_checks.py)
# ---------------------------------------------------------------------------------------------------------------------
_A = capi.A
MISALIGNED = [      # entry point, its arguments in front of the stream with one pointer moved off its alignment, the refusal
    ("mk_degree_power", (_A + 4, _A, _A, 4, 5, 6, 0, 0), "buffer not 8-byte aligned"),
    ("mk_degree_power", (_A, _A, _A + 4, 4, 5, 6, 0, 0), "buffer not 8-byte aligned"),
    ("mk_degree_power_bwd", (_A, _A, _A + 4, 4, 5, 6, 0, 0), "buffer not 8-byte aligned"),
]


@pytest.mark.parametrize("case", MISALIGNED, ids=capi.case_ids(MISALIGNED))
def test_misaligned_pointer_is_refused_before_any_launch(case):
    capi.assert_refused(*case)
