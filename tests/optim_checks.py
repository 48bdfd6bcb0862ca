"""Shared checks of the optimizer-kernel tests (a plain module, imported by test_optim_checks_cpu.py and
test_optim_guard_gpu.py; not a conftest).  Three parts:

* float64 restatements of what ``mk_mt_adam``, ``mk_adam_step``, ``mk_mt_lamb`` (both stages), ``mk_mt_sumsq`` /
  ``mk_mt_norm_finish`` and ``mk_mt_scale`` compute (include/makani_amd.h, the comments of csrc/optim.hip and csrc/adam.hip),
  evaluated on the same fp32 inputs and the same fp32 scalars; the bias corrections are formed in double and rounded once to
  fp32, as the kernels do.  The functions take numpy arrays or torch tensors (the grid-stride cases of the GPU tests evaluate
  them in float64 torch on the device);
* a bound for EVERY element of p, m and v (and for the per-tensor sums, the norm and the coefficients), derived by first-order
  propagation of one rounding ``u = 2^-24`` per fp32 operation through the kernels' expressions.  The bounds are written in
  terms of the magnitudes of the operands of each operation, never in units of the result alone: in Adam's L2 mode
  ``g' = wd p + g coef`` can cancel, and the error of the two terms then is hundreds of units of ``u v'``.  Nothing in a bound is
  measured on a kernel; ``tests/test_optim_checks_cpu.py`` runs an fp32 emulation of the kernels' arithmetic against them
  (worst error / bound 0.3 ... 0.7) and shows that a skipped or doubled update, a neighbour's step count or trust ratio, a gradient
  multiplier not applied and a LAMB update formed from the new parameter all lie outside;
* ``build_list``: a tensor list for the C ABI in which every stream the kernel writes is a ``kernel_checks.guarded`` buffer of its
  own, every stream it only reads sits between NaN bands, and any stream may start 0 ... 3 floats past a 16-byte boundary.

Rounding model.  Every fp32 operation (+, -, *, /, sqrtf, fmaf) returns its exact result times ``1 + d``, ``|d| <= u``: hipcc
compiles fp32 division and square root correctly rounded by default, and a contraction of ``a * b + c`` into an fma only removes
a rounding.  Terms of second order in ``u`` are dropped except where a first-order term can vanish (the square of the gradient
error, the root of a tiny ``v``).
"""
import ctypes
import math

import numpy as np
import torch

from kernel_checks import SENTINEL, guarded, poisoned

U = 2.0 ** -24          # unit roundoff of fp32
U64 = 2.0 ** -53        # unit roundoff of fp64
CHUNK = 16384           # kChunk of csrc/optim.hip: reals per norm partial
TINY = 1e-300


def f32(x):
    """``x`` rounded once to fp32, as a python float."""
    return float(np.float32(x))


# ---------------------------------------------------------------------------------------------------------------------
# numpy / torch dispatch (the references use only these and the arithmetic operators)
# ---------------------------------------------------------------------------------------------------------------------
def _is_t(x):
    return isinstance(x, torch.Tensor)


def _f64(x):
    return x.double() if _is_t(x) else np.asarray(x, dtype=np.float64)


def _sqrt(x):
    return torch.sqrt(x) if _is_t(x) else np.sqrt(x)


def _abs(x):
    return x.abs() if _is_t(x) else np.abs(x)


def _min(a, b):
    return torch.minimum(a, b) if _is_t(a) else np.minimum(a, b)


def _floor_at(x, s):
    return x.clamp_min(s) if _is_t(x) else np.maximum(x, s)


def _sum(x):
    return float(x.sum())


def bias_corrections(beta1, beta2, step):
    """(bc1, bc2, sqrt(bc2)) as the kernels form them: in double from the fp32 betas, rounded once to fp32."""
    bc2 = 1.0 - beta2 ** step
    return f32(1.0 - beta1 ** step), f32(bc2), f32(math.sqrt(bc2))


def _root_error(e, root):
    """What an error ``e >= 0`` of a non-negative radicand does to its root: ``e / (2 root)`` to first order, and never more than
    ``sqrt(e)`` (``|sqrt(a) - sqrt(b)| <= sqrt(|a - b|)``), which takes over where the radicand is as small as its error.  The
    first-order form is used without its factor 1/2, which covers the second-order term for ``e <= root^2``."""
    return _min(e / _floor_at(root, TINY), _sqrt(e))


# ---------------------------------------------------------------------------------------------------------------------
# AdamW / Adam (mk_mt_adam, mk_adam_step)
# ---------------------------------------------------------------------------------------------------------------------
def adam_ref(p, g, m, v, *, lr, beta1, beta2, eps, wd, adamw, coef, step):
    """One step of ``AdamOp::one`` (csrc/optim.hip) in float64 with its per-element bounds.  ``mk_adam_step`` (``adam1`` of
    csrc/adam.hip) is the case ``adamw = 0, coef = 1``.  All scalars are python floats that hold fp32 values.  Returns a dict with
    the new ``p``, ``m``, ``v``, the bounds ``e_p``, ``e_m``, ``e_v`` and ``upd`` (what the step subtracts from the decayed p).

    The kernel, with l2 = wd and decay = 1 in Adam (L2) mode, l2 = 0 and decay = fl(1 - fl(lr wd)) in AdamW mode:

        g' = fmaf(l2, p, fl(g coef))                 2 roundings, each of a quantity <= |l2 p| + |g coef|:
                                                     e_g = 2u (|l2 p| + |g coef|)       (NOT 2u |g'|: the terms can cancel)
        m' = fmaf(b1, m, fl(fl(1 - b1) g'))          the error of g' times (1 - b1); 1 - b1, the product and the fma round the
                                                     second term 3 times, the fma the first once:
                                                     e_m = (1 - b1) e_g + 3u (|b1 m| + (1 - b1) |g'|)
        v' = fmaf(b2, v, fl(fl(fl(1 - b2) g') g'))   (g' + e)^2 - g'^2 = 2 g' e + e^2; 4 roundings of the second term, 1 of the
                                                     first, both terms >= 0:
                                                     e_v = (1 - b2) (2 |g'| e_g + e_g^2) + 4u v'
        r  = sqrtf(v')                               e_r = min(e_v / r, sqrt(e_v))       (``_root_error``)
        den = fl(fl(r / bc2s) + eps)                 root, quotient and sum round once each, all <= den:
                                                     e_den = e_r / bc2s + 3u den
        p' = fl(fl(p decay) - fl(ss fl(m' / den)))   decay rounds twice and the product once (3u |p decay|); ss = fl(lr / bc1), the
                                                     quotient and the product round the update three times (3u |upd|); the
                                                     subtraction once (u |p'|); the errors of m' and den enter through
                                                     m / den: e_m / den + |m'| e_den / (den (den - e_den)), the last factor not
                                                     below eps, the smallest value den can take:
                                                     e_p = 3u |p decay| + u |p'| + ss (e_m / den + |m'| e_den / (den max(den - e_den, eps)))
                                                           + 3u |upd|
    """
    P, G, M, V = _f64(p), _f64(g), _f64(m), _f64(v)
    l2 = 0.0 if adamw else wd
    bc1, _, bc2s = bias_corrections(beta1, beta2, step)
    gc = G * coef
    g2 = l2 * P + gc
    pd = P * (1.0 - lr * wd) if adamw else P
    m2 = beta1 * M + (1.0 - beta1) * g2
    v2 = beta2 * V + (1.0 - beta2) * g2 * g2
    root = _sqrt(v2)
    den = root / bc2s + eps
    ss = lr / bc1
    upd = ss * m2 / den
    p2 = pd - upd
    e_g = 2 * U * (_abs(l2 * P) + _abs(gc))
    e_m = (1.0 - beta1) * e_g + 3 * U * (_abs(beta1 * M) + (1.0 - beta1) * _abs(g2))
    e_v = (1.0 - beta2) * (2 * _abs(g2) * e_g + e_g * e_g) + 4 * U * v2
    e_den = _root_error(e_v, root) / bc2s + 3 * U * den
    e_p = (3 * U * _abs(pd) + U * _abs(p2) + ss * (e_m / den + _abs(m2) * e_den / (den * _floor_at(den - e_den, eps)))
           + 3 * U * _abs(upd))
    return dict(p=p2, m=m2, v=v2, e_p=e_p, e_m=e_m, e_v=e_v, upd=upd)


# ---------------------------------------------------------------------------------------------------------------------
# LAMB (mk_mt_lamb)
# ---------------------------------------------------------------------------------------------------------------------
def lamb_scalars(*, beta1, beta2, beta3, eps, wd, adamw, bias_correction, div, step):
    bc1, bc2, _ = bias_corrections(beta1, beta2, step) if bias_correction else (1.0, 1.0, 1.0)
    return dict(b1=beta1, b2=beta2, b3=beta3, eps=eps, wd=wd, adamw=adamw, bc1=bc1, bc2=bc2, div=div)


def lamb_update(m2, v2, P, e_m, e_v, k):
    """``LambCoef::update``: ``u = (m / bc1) / (sqrtf(v / bc2) + eps)``, plus ``wd p`` by an fma in AdamW mode; returns (u, e_u).

        a = fl(m / bc1)               e_a = e_m / bc1 + u |a|
        w = fl(v / bc2)               e_w = e_v / bc2 + u w
        s = sqrtf(w)                  e_s = min(e_w / s, sqrt(e_w)) + u s
        den = fl(s + eps)             e_den = e_s + u den
        u0 = fl(a / den)              e_u0 = e_a / den + |a| e_den / (den max(den - e_den, eps)) + u |u0|
        u = fmaf(wd, p, u0)           e_u = e_u0 + u |u|                          (AdamW mode only)
    """
    a = m2 / k["bc1"]
    w = v2 / k["bc2"]
    s = _sqrt(w)
    den = s + k["eps"]
    u0 = a / den
    e_a = e_m / k["bc1"] + U * _abs(a)
    e_w = e_v / k["bc2"] + U * w
    e_s = _root_error(e_w, s) + U * s
    e_den = e_s + U * den
    e_u = e_a / den + _abs(a) * e_den / (den * _floor_at(den - e_den, k["eps"])) + U * _abs(u0)
    if k["adamw"]:
        u = k["wd"] * P + u0
        return u, e_u + U * _abs(u)
    return u0, e_u


def sumsq_bound(n, total, e_terms=0.0):
    """An fp64 sum of ``n`` non-negative terms in any order (the lanes' fma chains, the shuffle tree, the waves, the chunk partials
    in order) is off by at most ``n 2^-53`` of the sum: at most n - 1 additions, each a relative 2^-53 of a partial sum that never
    exceeds the total; the squares are exact in fp64 (an fma).  ``e_terms``: what the terms themselves are off by, in all."""
    return e_terms + n * U64 * (total + e_terms)


def lamb1_ref(p, g, m, v, k):
    """Stage 1 (``LambCoef::moments``, ``Lamb1Op``): new m and v with bounds, the sums of squares of the OLD p and of the update u
    with bounds.

        g1 = fl(g / div)
        g' = fmaf(wd, p, g1)   (L2 mode only)     the quotient rounds g1, the fma a quantity <= |wd p| + |g1|; as for Adam
                                                  e_g = 2u (|l2 p| + |g1|),  l2 = wd in L2 mode, else 0
        m' = fmaf(b1, m, fl(b3 g'))               b3 is given, not formed: the product and the fma round the second term, the
                                                  fma the first; one rounding more is allowed on either (two roundings at their
                                                  worst reach a two-rounding bound, and the dropped second-order terms would
                                                  decide):  e_m = b3 e_g + u (2 |b1 m| + 3 b3 |g'|)
        v' as in Adam                             e_v = (1 - b2) (2 |g'| e_g + e_g^2) + 4u v'
        u from (m', v', p)                        ``lamb_update`` with e_m, e_v
        sum u^2: each square is off by 2 |u| e_u + e_u^2, the fp64 sum by ``sumsq_bound``; sum p^2 has exact terms.
    """
    P, G, M, V = _f64(p), _f64(g), _f64(m), _f64(v)
    g1 = G / k["div"]
    l2 = 0.0 if k["adamw"] else k["wd"]
    g2 = l2 * P + g1
    e_g = 2 * U * (_abs(l2 * P) + _abs(g1))
    m2 = k["b1"] * M + k["b3"] * g2
    v2 = k["b2"] * V + (1.0 - k["b2"]) * g2 * g2
    e_m = k["b3"] * e_g + U * (2 * _abs(k["b1"] * M) + 3 * k["b3"] * _abs(g2))
    e_v = (1.0 - k["b2"]) * (2 * _abs(g2) * e_g + e_g * e_g) + 4 * U * v2
    u, e_u = lamb_update(m2, v2, P, e_m, e_v, k)
    n = P.numel() if _is_t(P) else P.size
    sp, su = _sum(P * P), _sum(u * u)
    return dict(m=m2, v=v2, e_m=e_m, e_v=e_v, u=u, e_u=e_u, sp=sp, su=su, e_sp=sumsq_bound(n, sp),
                e_su=sumsq_bound(n, su, _sum(2 * _abs(u) * e_u + e_u * e_u)))


def lamb2_ref(p, m2, v2, k, *, lr, trust):
    """Stage 2 (``Lamb2Op``) on the fp32 moments stage 1 left: ``p' = p - ratio u(m', v', p)``.  The norms are the reference's OWN
    (float64 sums over this tensor), never the kernel's ``tsum``, so a kernel that reads another tensor's sums fails.

        pn = (float)sqrt(tsum_p)      tsum is off by ``sumsq_bound`` (relative d), the root halves it, sqrt and the cast round:
                                      relative d_pn = d_p / (2 (1 - d_p)) + 2^-53 + u; the same for un, whose terms u^2 carry the
                                      roundings of ``lamb_update`` on exact inputs
        ratio = fl(lr fl(pn / un))    2 roundings:  e_ratio = ratio (d_pn + d_un + 2u); ratio = lr exactly without ``trust`` or
                                      with a zero norm
        p' = fl(p - fl(ratio u))      product and difference round once each; each is allowed twice, because a lone rounding
                                      meets ``u |x|`` exactly just above a power of two:
                                      e_p = |u| e_ratio + ratio e_u + 2u |ratio u| + 2u |p'|
    """
    P, M2, V2 = _f64(p), _f64(m2), _f64(v2)
    zero = 0.0 * P
    u, e_u = lamb_update(M2, V2, P, zero, zero, k)
    n = P.numel() if _is_t(P) else P.size
    sp, su = _sum(P * P), _sum(u * u)
    ratio, e_ratio = lr, 0.0
    if trust and sp != 0.0 and su != 0.0:
        e_sp = sumsq_bound(n, sp)
        e_su = sumsq_bound(n, su, _sum(2 * _abs(u) * e_u + e_u * e_u))
        d_p, d_u = e_sp / sp, e_su / su
        assert d_p < 0.5 and d_u < 0.5, "the update norm is lost in its own error: choose other inputs"
        ratio = lr * math.sqrt(sp) / math.sqrt(su)
        e_ratio = ratio * (d_p / (2 * (1 - d_p)) + d_u / (2 * (1 - d_u)) + 2 * (U64 + U) + 2 * U)
    p2 = P - ratio * u
    e_p = _abs(u) * e_ratio + ratio * e_u + 2 * U * _abs(ratio * u) + 2 * U * _abs(p2)
    return dict(p=p2, e_p=e_p, ratio=ratio, e_ratio=e_ratio, sp=sp, su=su)


# ---------------------------------------------------------------------------------------------------------------------
# norm and clip coefficients (finish_total of csrc/optim.hip)
# ---------------------------------------------------------------------------------------------------------------------
def exact_sumsq(x):
    """(sum of squares, bound of the kernel's fp64 sum) of an fp32 array: the squares are exact in float64 and ``math.fsum`` adds
    them without error before one rounding."""
    x = np.asarray(x, dtype=np.float64).ravel()
    s = math.fsum((x * x).tolist())
    return s, sumsq_bound(x.size, s)


def clip_ref(tsums, e_tsums, max_norm, clip_mode):
    """``G = (float)sqrt(sum_t tsum[t])`` and the coefficient of ``clip_mode`` 1 (torch: min(1, max / (G + 1e-6))), 2 (apex LAMB's
    divisor: G > max ? G / max : 1) or 3 (none) with their bounds: (G, e_G, coef, e_coef); coef is None in mode 3.

    The total adds T doubles (``T 2^-53``) that are off by ``e_tsums``; the root halves the relative error, sqrt and the cast to
    fp32 round once each.  Mode 1: ``fl(G + 1e-6f)`` and the quotient round once each, and 1e-6f is the fp32 number next to 1e-6;
    mode 2: one quotient.  The clamp ``min(1, .)`` and the comparison are monotone, so a coefficient within its bound of the
    reference's stays within it; the tests keep G away from ``max_norm`` where the branch of mode 2 would flip."""
    T = len(tsums)
    s = math.fsum(tsums)
    e_s = math.fsum(e_tsums) + T * U64 * s
    G = math.sqrt(s)
    d_G = (e_s / s) / (2 * (1 - e_s / s)) + U64 + U if s > 0 else 0.0
    if clip_mode == 3:
        return G, G * d_G, None, None
    if clip_mode == 1:
        c = max_norm / (G + f32(1e-6))
        if c >= 1.0:
            return G, G * d_G, 1.0, (0.0 if c * (1 - d_G - 2 * U) >= 1.0 else d_G + 2 * U)
        return G, G * d_G, c, c * (d_G + 2 * U)
    assert abs(G - max_norm) > 4 * G * d_G, "G sits on the branch of clip_mode 2: choose another max_norm"
    if G > max_norm:
        return G, G * d_G, G / max_norm, (G / max_norm) * (d_G + U)
    return G, G * d_G, 1.0, 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the criterion
# ---------------------------------------------------------------------------------------------------------------------
def worst_ratio(got, ref, bound, what=""):
    """Asserts that EVERY element of ``got`` is finite and ``|got - ref| <= bound`` (an element whose bound is zero must be
    exact); returns the worst ``|got - ref| / bound``.  numpy arrays or torch tensors."""
    if _is_t(ref):
        g = got.to(ref.device).double()
        assert bool(torch.isfinite(g).all()), f"{what}: {int((~torch.isfinite(g)).sum())} elements are NaN or Inf"
        err = (g - ref).abs()
        ratio = torch.where(bound > 0, err / bound.clamp_min(TINY), torch.where(err > 0, float("inf"), 0.0).to(err.dtype))
        i = int(torch.argmax(ratio))
        worst = float(ratio.flatten()[i])
        bad = int((ratio > 1).sum())
    else:
        g = np.asarray(got, dtype=np.float64)
        ref, bound = np.asarray(ref, dtype=np.float64), np.broadcast_to(np.asarray(bound, dtype=np.float64), g.shape)
        assert g.shape == ref.shape, f"{what}: shape {g.shape} against reference {ref.shape}"
        assert np.isfinite(g).all(), f"{what}: {int((~np.isfinite(g)).sum())} elements are NaN or Inf"
        err = np.abs(g - ref)
        ratio = np.where(bound > 0, err / np.maximum(bound, TINY), np.where(err > 0, np.inf, 0.0))
        i = int(np.argmax(ratio)) if ratio.size else 0
        worst = float(ratio.ravel()[i]) if ratio.size else 0.0
        bad = int((ratio > 1).sum())
    if not worst <= 1.0:
        raise AssertionError(f"{what}: worst |got - ref| / bound = {worst:.3g} at flat index {i}: got {float(g.flatten()[i])!r}, "
                             f"ref {float(ref.flatten()[i])!r}, bound {float(bound.flatten()[i]):.3e}; {bad} of {ratio.size if not _is_t(ratio) else ratio.numel()} "
                             f"elements exceed the bound")
    return worst


def exceeds(got, ref, bound):
    """The worst ``|got - ref| / bound`` without asserting (the mutation checks); numpy."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    return float(np.max(np.where(bound > 0, err / np.maximum(bound, TINY), np.where(err > 0, np.inf, 0.0))))


def scalar_ratio(got, ref, bound, what=""):
    """One value against its bound; returns the ratio."""
    got, err = float(got), abs(float(got) - ref)
    assert math.isfinite(got), f"{what}: {got!r}"
    if bound == 0.0:
        assert err == 0.0, f"{what}: got {got!r}, must be {ref!r} exactly"
        return 0.0
    assert err <= bound, f"{what}: got {got!r}, reference {ref!r}, error {err:.3e} over the bound {bound:.3e} ({err / bound:.2f} x)"
    return err / bound


# ---------------------------------------------------------------------------------------------------------------------
# tensor lists for the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def _bits32(t):
    return t.contiguous().view(torch.int32)


class TensorList:
    """What ``build_list`` returns: ``T`` tensors of ``D`` streams each.  ``ptrs`` (uint64, tensor-major: stream d of tensor t at
    ``[D t + d]``) and ``n`` (int64) are the host tables of the C ABI; ``view(t, d)`` is the device tensor, ``host(t, d)`` a numpy
    copy of it.  ``check(what)`` asserts, after a launch, that every guard band and every sentinel in front of an offset view still
    holds the sentinel bit for bit and that every read-only stream, its leading NaNs included, equals its input bit for bit."""

    def __init__(self, T, D):
        self.T, self.D = T, D
        self.views = [[None] * D for _ in range(T)]
        self._rw, self._ro = [], []
        self.ptrs = (ctypes.c_uint64 * (T * D))()
        self.n = (ctypes.c_longlong * T)()

    def view(self, t, d):
        return self.views[t][d]

    def host(self, t, d):
        return self.views[t][d].cpu().numpy()

    def check(self, what=""):
        for t, d, whole, off, band_check in self._rw:
            band_check(f"{what}: tensor {t} stream {d}")
            if off:
                lead = whole[:off]
                assert torch.equal(_bits32(lead), _bits32(torch.full_like(lead, SENTINEL))), \
                    f"{what}: tensor {t} stream {d}: the {off} floats in front of the offset view were written"
        for t, d, whole, orig in self._ro:
            assert torch.equal(_bits32(whole), _bits32(orig)), f"{what}: tensor {t} stream {d} is read-only and was written"


def build_list(dev, data, offsets, readonly):
    """A tensor list on ``dev``.  ``data[t][d]``: the fp32 values of stream d of tensor t (a numpy array or a torch tensor, 1-D);
    ``offsets``: one tuple of D offsets in floats (0 ... 3) past a 16-byte boundary for all tensors, or one tuple per tensor;
    ``readonly[d]``: the kernel only reads stream d.

    A written stream is a ``guarded`` buffer of its own (4 KB of the sentinel on either side, checked bit for bit) and the floats
    in front of an offset view hold the sentinel too; a read-only stream is ``poisoned`` (NaN bands) with NaNs in front of an
    offset view, so a vector load that starts before the tensor, or a read past its end, puts a NaN into a result."""
    T, D = len(data), len(readonly)
    if not isinstance(offsets[0], (tuple, list)):
        offsets = [tuple(offsets)] * T
    L = TensorList(T, D)
    for t in range(T):
        assert len(data[t]) == D and len(offsets[t]) == D
        for d in range(D):
            a = data[t][d]
            a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)) if isinstance(a, np.ndarray) else a
            assert a.dtype == torch.float32 and a.dim() == 1 and a.numel() >= 1
            off, n = int(offsets[t][d]), a.numel()
            assert 0 <= off <= 3
            if readonly[d]:
                flat = torch.cat([torch.full((off,), float("nan"), dtype=torch.float32, device=a.device), a])
                whole = poisoned(flat, dev)
                L._ro.append((t, d, whole, flat.to(dev)))
            else:
                whole, band_check = guarded((n + off,), torch.float32, dev)
                whole[off:].copy_(a)
                L._rw.append((t, d, whole, off, band_check))
            v = whole[off:]
            assert v.data_ptr() % 16 == 4 * off and v.numel() == n
            L.views[t][d] = v
            L.ptrs[t * D + d] = v.data_ptr()
        L.n[t] = data[t][0].shape[0]
        assert all(x.shape[0] == L.n[t] for x in data[t])
    return L


def i32(vals):
    return (ctypes.c_int * max(1, len(vals)))(*[int(v) for v in vals])


def chunks(n):
    return (n + CHUNK - 1) // CHUNK
