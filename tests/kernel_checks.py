"""Shared checks for kernel tests (a plain module, imported by the test files; not a conftest).

Three criteria a kernel test here should apply, and the helpers that implement them:

* every element: ``bf16_elementwise`` bounds EACH element of a bf16 result in bf16 ulps against a float64 reference (a norm over
  the tensor lets a handful of completely wrong elements pass); fp32 results use a relative L2 norm per output row (``row_rel``);
* guard bands: ``guarded`` gives an output buffer with sentinel bands around it and a function that asserts the bands still hold
  the sentinel bit for bit, so a store past a ragged tile is seen;
* NaN bands: ``poisoned`` puts an input between NaN bands, so a read past the logical end shows up as a NaN in the output.

The error model behind the bf16 bound (``gemm_gamma`` and the ``slack_*`` functions): the kernel multiplies exact bf16 operands
(every product is exact in fp32), accumulates in fp32 in some order, applies its epilogue in fp32 and rounds to bf16 once.  Against
the float64 value of the same expression the fp32 accumulation is off by at most ``gamma = K * 2^-23 * (|W| @ |X|)`` (the standard
forward error bound of a dot product, valid for any order), the epilogue adds what the ``slack_*`` functions state, and the final
rounding is at most half a bf16 ulp; the bound allows one whole ulp at the larger of the two magnitudes plus the slack.
``tests/test_kernel_checks_cpu.py`` runs an fp32 emulation of that arithmetic against the bound.
"""
import math

import numpy as np
import torch

BAND_BYTES = 4096
SENTINEL = -77.0                       # a store of a result never equals it bit for bit over a whole band
SENTINEL_C = complex(-77.0, 55.0)      # the same for complex64 (tests/test_specattn_gpu.py uses this value)
GELU_GRAD_MAX = 1.13                   # max |gelu'| = 1.1290, reached at x = sqrt(2)


# ---------------------------------------------------------------------------------------------------------------------
# buffers with bands
# ---------------------------------------------------------------------------------------------------------------------
def _bits(t):
    t = torch.view_as_real(t) if t.is_complex() else t
    return t.contiguous().view(-1).view(torch.uint8)     # shares the storage of a contiguous ``t``


def _banded(shape, dtype, device, fill):
    """A flat buffer of ``fill`` with a contiguous, 16-byte-aligned view of ``shape`` at least ``BAND_BYTES`` from either end.
    Returns (buffer, view, first element, one past the last element)."""
    shape = tuple(int(s) for s in shape)
    item = torch.empty((), dtype=dtype).element_size()
    n = int(np.prod(shape, dtype=np.int64)) if shape else 1
    band = BAND_BYTES // item
    buf = torch.full((2 * band + n + 16 // min(item, 16) + 1,), fill, dtype=dtype, device=device)
    off = (-(buf.data_ptr() + band * item)) % 16
    assert off % item == 0, "the allocator returned a buffer that is not aligned to its element size"
    lo = band + off // item
    view = buf[lo:lo + n].view(shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    assert lo * item >= BAND_BYTES and (buf.numel() - lo - n) * item >= BAND_BYTES
    return buf, view, lo, lo + n


def guarded(shape, dtype, device, fill=None):
    """An output buffer between two bands of ``fill``: returns (view, check).  The view (contiguous, 16-byte aligned, ``shape``)
    holds ``fill`` too; ``check(what="")`` asserts that every byte of both bands still is what was written there.  ``fill``
    defaults to the sentinel for floating-point and complex types.  ``check.buffer`` and ``check.span`` (first element, one
    past the last) expose the whole allocation to the tests of this module."""
    if fill is None:
        fill = SENTINEL_C if dtype.is_complex else SENTINEL
    buf, view, lo, hi = _banded(shape, dtype, device, fill)
    want_lo, want_hi = _bits(buf[:lo]).clone(), _bits(buf[hi:]).clone()

    def check(what=""):
        for name, got, want in (("front", _bits(buf[:lo]), want_lo), ("back", _bits(buf[hi:]), want_hi)):
            if not torch.equal(got, want):
                bad = torch.nonzero(got != want).flatten()
                raise AssertionError(f"{what}: the {name} guard band was written: {bad.numel()} bytes changed, the first at byte "
                                     f"{int(bad[0])} of {got.numel()} (the band ends / starts at the tensor)")

    check.buffer, check.span = buf, (lo, hi)
    return view, check


def poisoned(t, device=None):
    """A bit-equal copy of ``t`` (floating point or complex) between two NaN bands, as a contiguous 16-byte-aligned view on
    ``device`` (default: where ``t`` is).  Only the bands are NaN: the copy holds exactly the bits of ``t``."""
    assert t.is_floating_point() or t.is_complex()
    device = t.device if device is None else device
    fill = complex(float("nan"), float("nan")) if t.is_complex() else float("nan")
    buf, view, lo, hi = _banded(t.shape, t.dtype, device, fill)
    view.copy_(t)
    assert bool(torch.isnan(torch.view_as_real(buf[:lo]) if t.is_complex() else buf[:lo]).all())
    assert bool(torch.isnan(torch.view_as_real(buf[hi:]) if t.is_complex() else buf[hi:]).all())
    return view


# ---------------------------------------------------------------------------------------------------------------------
# the bf16 criterion
# ---------------------------------------------------------------------------------------------------------------------
def bf16_ulp(v):
    """Spacing of bf16 (8 significant bits) at the magnitude of ``v`` (> 0)."""
    return torch.exp2(torch.floor(torch.log2(v)) - 7)


def bf16_elementwise(y, ref64, slack64=None, what=""):
    """Asserts for EVERY element ``|y - ref| <= ulp_bf16(max(|y|, |ref|, rms(ref) / 256)) + slack`` and that ``y`` is finite.
    Returns the worst ``|y - ref| / bound``; on failure reports it with its index."""
    assert tuple(y.shape) == tuple(ref64.shape), f"{what}: shape {tuple(y.shape)} against reference {tuple(ref64.shape)}"
    ref = ref64.double()
    yd = y.to(ref.device).double()
    assert bool(torch.isfinite(yd).all()), f"{what}: {int((~torch.isfinite(yd)).sum())} elements are NaN or Inf"
    rms = ref.square().mean().sqrt()
    tol = bf16_ulp(torch.maximum(torch.maximum(yd.abs(), ref.abs()), rms / 256))
    if slack64 is not None:
        tol = tol + slack64.double().to(ref.device)
    ratio = (yd - ref).abs() / tol
    flat = int(torch.argmax(ratio))
    worst = float(ratio.flatten()[flat])
    if not worst <= 1.0:
        idx = tuple(int(i) for i in np.unravel_index(flat, tuple(ratio.shape)))
        raise AssertionError(f"{what}: worst |y - ref| / bound = {worst:.3f} at {idx}: y = {float(yd[idx])!r}, ref = {float(ref[idx])!r}, "
                             f"bound = {float(tol[idx]):.3e}; {int((ratio > 1).sum())} of {ratio.numel()} elements exceed the bound")
    return worst


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def gemm_gamma(w64, x64):
    """``K * 2^-23 * (|W| @ |X|)``: what an fp32 accumulation of the exact products of ``w64 [M, K] @ x64 [..., K, P]`` can be
    off by, in any order of summation (float64)."""
    return w64.shape[-1] * 2.0 ** -23 * torch.matmul(w64.abs(), x64.abs())


def slack_plain(gamma):
    return gamma


def slack_pre(gamma, pre64):
    """The stored pre-activation ``acc + bias``: the accumulation and one fp32 addition."""
    return gamma + 2.0 ** -23 * pre64.abs()


def slack_gelu(gamma, pre64):
    """``gelu(acc + bias)``: the error of the argument times max |gelu'|.  The error of the epilogue's CDF (Abramowitz-Stegun
    7.1.26, under 1.5e-7 absolute) and the fp32 product lie under the ``rms / 256`` floor and the half ulp the bound leaves."""
    return GELU_GRAD_MAX * (gamma + 2.0 ** -23 * pre64.abs())


def slack_aux(gamma):
    """``acc * gelu'(aux)``: the accumulation error times max |gelu'|."""
    return GELU_GRAD_MAX * gamma


def slack_addend(gamma, term64, y64):
    """``acc + (a * addend + b)``: the accumulation, one fused multiply-add for the term and one fp32 addition."""
    return gamma + 2.0 ** -23 * (term64.abs() + y64.abs())


# ---------------------------------------------------------------------------------------------------------------------
# fp32 results
# ---------------------------------------------------------------------------------------------------------------------
def row_rel(got, want):
    """Relative L2 error of every row (the last axis) of ``got`` against ``want`` (numpy, float64 / complex128)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    assert np.isfinite(got).all(), f"{int((~np.isfinite(got)).sum())} elements are NaN or Inf"
    num = np.sqrt((np.abs(got.astype(want.dtype) - want) ** 2).sum(-1))
    den = np.sqrt((np.abs(want) ** 2).sum(-1))
    assert (den > 0).all(), "a reference row is all zero: choose other inputs"
    return num / den
