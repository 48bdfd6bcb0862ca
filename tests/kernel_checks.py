"""Shared checks for kernel tests (a plain module, imported by the test files; not a conftest).

Three criteria a kernel test here should apply, and the helpers that implement them:

* every element: ``bf16_elementwise`` bounds EACH element of a bf16 result in bf16 ulps against a float64 reference (a norm over
  the tensor lets a handful of completely wrong elements pass); fp32 results use a relative L2 norm per output row (``row_rel``),
  those of the bf16x3 engine and the fp32-MFMA kernels a bound on EACH element in units of ``2^-23 (|A| @ |B|)``
  (``x3_elementwise``, with ``absdot`` and the ``x3_slack_*`` functions; its constant comes from a CPU emulation of the engine);
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


# ---------------------------------------------------------------------------------------------------------------------
# the fp32-result criterion of the bf16x3 engine (csrc/x3_engine.h) and of the fp32-MFMA kernels (csrc/gemm.hip)
# ---------------------------------------------------------------------------------------------------------------------
X3_C = 9.0          # bf16x3 engine: twice the emulation's worst ratio (4.46), rounded up, see ``x3_elementwise``
F32_C = 5.0         # fp32 MFMA (an fmaf chain): twice the emulation's worst ratio (2.30), rounded up


def x3_split(t, exact=True):
    """The exact three-way truncation split of an fp32 tensor, ``split3`` of csrc/x3_engine.h: ``t = h + m + l`` with every
    piece a bf16 number held in fp32 (h: the upper 16 bits of t; m: the upper 16 bits of t - h; l: the rest, at most 8
    significant bits).  Asserts that the pieces are bf16 numbers and add back to ``t`` exactly.
    ``exact=False`` is what the kernel does with ANY input: the third piece is cut to its upper 16 bits as well (``pack_hi``) and
    nothing is asserted.  The two differ only below 2^-110, where a piece falls into the subnormal range (``x3_slack_underflow``)."""
    assert t.dtype == torch.float32
    t = t.contiguous()

    def trunc(v):
        return (v.view(torch.int32) & -65536).view(torch.float32)

    h = trunc(t)
    r1 = t - h                        # exact: the low 16 bits of the significand
    m = trunc(r1)
    lo = r1 - m                       # exact
    if not exact:
        return h, m, trunc(lo)
    assert torch.equal(trunc(lo), lo), "the third piece does not fit bf16: the input holds subnormal or non-finite values"
    assert torch.equal(h.double() + m.double() + lo.double(), t.double()), "the three pieces do not add back to the input"
    return h, m, lo


def _parts(t):
    t = t.double() if not t.is_complex() else t.to(torch.complex128)
    return (t.real.abs(), t.imag.abs()) if t.is_complex() else (t.abs(), None)


def absdot(eq, a, b):
    """The float64 magnitude ``|A| @ |B|`` of the contraction ``einsum(eq, a, b)``: what the error of an fp32 evaluation scales
    with.  Real operands give a real tensor.  If either operand is complex the result is complex128 and carries the magnitude
    of each COMPONENT of the product: its real part is ``|ar||br| + |ai||bi|`` (the terms of ``re(sum a b)``), its imaginary
    part ``|ar||bi| + |ai||br|``; a conjugate on either side only changes signs, so conjugated forms take the same call."""
    (ar, ai), (br, bi) = _parts(a), _parts(b)
    if ai is None and bi is None:
        return torch.einsum(eq, ar, br)
    zero = lambda t: torch.zeros_like(t)
    ai = zero(ar) if ai is None else ai
    bi = zero(br) if bi is None else bi
    return torch.complex(torch.einsum(eq, ar, br) + torch.einsum(eq, ai, bi), torch.einsum(eq, ar, bi) + torch.einsum(eq, ai, br))


def _components(t, device=None):
    """float64 view of a real tensor, or of the (re, im) components of a complex one (a trailing axis of 2)."""
    t = t.detach()
    t = t if device is None else t.to(device)
    return torch.view_as_real(t.to(torch.complex128)) if t.is_complex() else t.double()


def x3_slack_add(ref64):
    """One extra fp32 addition in an epilogue (a bias, the soft-shrink's ``v -/+ lambda``, the two-accumulator sum of
    ``DftEpi``): the sum is rounded once more, ``2^-24 |sum|`` to first order; allowed: ``2^-23 |ref|`` per component."""
    c = _components(ref64).abs() * 2.0 ** -23
    return torch.view_as_complex(c) if ref64.is_complex() else c


def x3_slack_sum(g, mag64):
    """A fixed-order fp32 sum of ``g`` partial panels, or ``g`` fp32 atomic adds: each of the g - 1 additions rounds a partial
    sum that is at most ``mag`` in magnitude, ``(g - 1) 2^-24 mag`` in all; allowed: ``g * 2^-23 * mag``."""
    return g * 2.0 ** -23 * mag64


def _ones(t):
    return torch.ones_like(t) * (complex(1.0, 1.0) if t.is_complex() else 1.0)


def x3_slack_underflow(eq, a, b):
    """What the three-way split loses at the bottom of the exponent range, for ``einsum(eq, a, b)`` on the bf16x3 engine.  A
    piece is a bf16 number, the upper half of an fp32 word, and in the subnormal range those are 2^-133 apart: of an operand
    element below 2^-110 the split keeps everything above 2^-133 and drops less than 2^-133 (whichever pieces fall there), so a
    product is off by less than ``2^-133 (|a| + |b|)``; the accumulator, fp32, is exact to 2^-149 there, 12 roundings per
    k-term at most.  For operands of order 1 this is 1e-38 times the contraction length: it only matters for outputs whose
    every term is that small, as the Legendre synthesis of a high mode at the latitude next to a pole, where the table falls
    from 1e-35 through the subnormals to zero (found on the MI355X at m = 34, nlat = 131: those elements, exact to 2^-133 per term, reach 65 ... 92
    times ``2^-23 mag``; ``tests/test_kernel_checks_cpu.py`` reproduces it)."""
    ua, ub = _ones(a), _ones(b)
    return 2.0 ** -133 * (absdot(eq, ua, b) + absdot(eq, a, ub)) + 12 * 2.0 ** -149 * absdot(eq, ua, ub)


def x3_elementwise(y, ref64, mag64, c=X3_C, slack64=None, what=""):
    """The fp32-result criterion: asserts that EVERY element of ``y`` is finite and ``|y - ref| <= c * 2^-23 * mag + slack``
    (complex tensors: every component, with ``mag`` / ``slack`` complex tensors that hold the components' values, as ``absdot``
    returns them).  ``ref64`` is the float64 value of the contraction, ``mag64`` its ``absdot``.  Returns the worst
    ``|y - ref| / (2^-23 mag)`` (slack subtracted from the error first); on failure reports it with its index.

    The unit: an fp32 dot product summed in any order is off by at most ``K * 2^-24 * mag`` to first order, and for operands
    without structure by a small multiple of ``2^-23 * mag``, which the ratio measures.  A defect is far away: one of the
    three 2^-16-weight piece products of the engine not issued costs about ``2^-16 mag / sqrt(K)``.

    The constant ``c`` is NOT taken from the kernels.  ``tests/test_kernel_checks_cpu.py`` emulates the arithmetic of
    ``x3_tile`` on the CPU (``x3_split``, the six piece products in the order PA = {2,0,1,1,0,0}, PB = {0,2,1,0,1,0} per 16-k
    sub-step, fp32 accumulation) for 64 x 96 outputs of N(0,1) operands at the contraction lengths of the GPU tests,
    K = 4, 12, 36, 70, 131, 260, 280, real and complex, and measures the worst ratio of

        one fp32 add per 16-k piece product (the matrix core adding a product group at once):   0.9 ... 2.4  (2.36 at K = 4)
        one fp32 add per scalar product, sequentially (the pessimistic order):                  1.3 ... 4.5  (4.46 at K = 280)
        one of the three 2^-16-weight pieces not issued:     at least 27 (K = 280), 28 (260), 41 (131), 68 (70), 70 (36),
                                                             143 (12), 196 (4); whole-tensor rel 8.2e-6 ... 1.2e-5
        one element missing one k-term:                      at least 4,990

    ``X3_C = 9`` is twice the worst ratio of the sequential order, rounded up, and lies three times under the smallest ratio a
    single dropped piece reaches at any of those lengths (the CPU test asserts both, which is why the GPU shapes keep
    K <= ~300: the ratio of a dropped piece falls as 1 / sqrt(K)).
    The fp32-MFMA kernels of csrc/gemm.hip (``v_mfma_f32_32x32x2_f32``: an fmaf chain over k) are held to ``F32_C``, from an
    fp32 emulation without the split on the same rule: a sequential chain of fused, or of rounded, multiply-adds reaches
    1.1 ... 2.3 (2.30 at K = 260), ``F32_C = 5``.
    On an MI355X the kernels reach 2.8 (bf16x3) and 2.6 (fp32 MFMA) over the shapes of tests/test_x3_guard_gpu.py: records,
    not limits.

    Slack terms (``slack64``): ``x3_slack_add`` for an epilogue's extra addition, ``x3_slack_sum`` for partial panels or
    atomics, ``x3_slack_underflow`` where an operand reaches down to the subnormals; ReLU and soft-shrink are 1-Lipschitz
    (|f(a) - f(b)| <= |a - b|) and need none."""
    assert tuple(y.shape) == tuple(ref64.shape) == tuple(mag64.shape), \
        f"{what}: shapes {tuple(y.shape)}, reference {tuple(ref64.shape)}, magnitude {tuple(mag64.shape)}"
    assert y.is_complex() == ref64.is_complex() == mag64.is_complex(), f"{what}: real and complex tensors mixed"
    ref = _components(ref64)
    yd, mag = _components(y, ref.device), _components(mag64, ref.device)
    bad = ~torch.isfinite(yd)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements are NaN or Inf, the first at {tuple(int(i) for i in torch.nonzero(bad)[0])}"
    unit = 2.0 ** -23 * mag
    err = (yd - ref).abs()
    if slack64 is not None:
        err = (err - _components(slack64, ref.device)).clamp_min(0.0)
    # an element without magnitude (every product is zero) must be exact: ratio 0 if it is, inf if not
    ratio = torch.where(unit > 0, err / unit.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).to(err.dtype))
    flat = int(torch.argmax(ratio))
    worst = float(ratio.flatten()[flat])
    if not worst <= c:
        idx = tuple(int(i) for i in np.unravel_index(flat, tuple(ratio.shape)))
        raise AssertionError(f"{what}: worst |y - ref| / (2^-23 mag) = {worst:.1f} (limit {c}) at {idx}: y = {float(yd[idx])!r}, "
                             f"ref = {float(ref[idx])!r}, mag = {float(mag[idx]):.3e}; {int((ratio > c).sum())} of {ratio.numel()} "
                             f"elements exceed the limit")
    return worst


def node_kinds(y):
    """The class names of every autograd node behind ``y``: which of the package's functions, and which of torch's, a graph holds."""
    seen, stack = set(), [y.grad_fn]
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        stack += [f for f, _ in fn.next_functions]
    return [type(f).__name__ for f in seen]
