"""What the tests of the latitude interpolation share (a plain module, not a conftest): the recorded reference tables, the
general tables, float64 references with their per-element bounds, and strided buffers with NaN / sentinel gaps.

Forward bound.  The kernel forms, from fp32 operands a', b' (normalised in fp32 exactly as numpy does) and the fp32 weight w,
``d = fl(b' - a')`` and ``y = fma(w, d, a')`` for ``|w| < 0.5``, else ``y = fma(fl(w - 1), d, b')``.  With u = 2^-24 and against the
float64 lerp with the float64 weight: rounding w costs at most ``u |w| |b' - a'|``, rounding d at most ``u |w| |b' - a'|`` (or
``u |w - 1| |b' - a'|`` in the second form, where ``fl(w - 1)`` is exact for w in [0.5, 2]), the final rounding ``u |y|``; for
``|w| <= 1`` that is below ``3 u (|a'| + |b'|)``.  For extrapolating weights the three terms grow with ``max(1, |w|, |w - 1|)``, by
which the bound is scaled.

Backward bound.  ``gx = (fma chain over t terms of c_t gy_t) / scale`` with ``c_t`` = ``1 - w`` or ``w``, each rounded once from
float64 to fp32 (so its error is RELATIVE to the coefficient; ``fl(1 - fl(w))`` would not do: next to the equator w is close to 1
and the rounding of w is not small against 1 - w): one rounding per chain step (t), one for ``1 - w``, one for the weight, one
for the division, each at most u times the sum of the magnitudes: ``(t + 3) u sum |c_t gy_t| / |scale|`` against float64.
"""
import os

import numpy as np
import torch

from kernel_checks import SENTINEL, bf16_elementwise, guarded, poisoned

U = 2.0 ** -24
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_grids.npz")
NLATS = (2, 3, 4, 5, 8, 33, 721)
BIAS = np.array([0.3, -1.2, 2.5], dtype=np.float32)
SCALE = np.array([0.7, 1.9, 3.3], dtype=np.float32)
_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        with np.load(GOLDEN) as f:
            _fixture = {k: f[k] for k in f.files}
    return _fixture


def converter_table(nlat):
    """(global source rows int64, float64 weights, Hs) of the recorded reference run for fp32 latitudes."""
    f = fixture()
    return f[f"n{nlat}_f32_indices"].astype(np.int64), f[f"n{nlat}_f32_interp_weights"].reshape(-1).astype(np.float64), nlat


def general_table(name):
    """Tables the converter never builds: (rows, weights, Hs)."""
    if name == "nonmono":       # any order, repeats, rows never asked for (2 and 3 of 7 are b-rows only / unused)
        return np.array([4, 0, 4, 5, 0, 1, 4], dtype=np.int64), np.array([0.3, 0.77, 0.3, 0.0, 1.0, 0.5, 0.61]), 7
    if name == "extrap":        # weights outside [0, 1]
        return np.array([0, 1, 2, 2], dtype=np.int64), np.array([-0.5, 1.5, 0.25, 1.5]), 4
    if name == "hd1":
        return np.array([1], dtype=np.int64), np.array([0.4]), 3
    if name == "hd2hs":         # Hd = 2 Hs
        hs = 5
        i = np.minimum(np.arange(2 * hs) // 2, hs - 2).astype(np.int64)
        return i, np.linspace(0.0, 1.0, 2 * hs), hs
    raise KeyError(name)


TABLES = [f"conv{n}" for n in (2, 3, 5, 33)] + ["nonmono", "extrap", "hd1", "hd2hs"]


def table(name):
    return converter_table(int(name[4:])) if name.startswith("conv") else general_table(name)


def dense_matrix(idx, w, hs):
    """The float64 interpolation matrix [Hd, Hs]: row k has 1 - w_k at i_k and w_k at i_k + 1."""
    m = np.zeros((len(idx), hs))
    for k, (i, wk) in enumerate(zip(idx, w)):
        m[k, i] += 1.0 - wk
        m[k, i + 1] += wk
    return m


def csr_to_dense(tables):
    """[Hs, Hd] float64 from the CSR transpose of ``ops.LatInterpTables`` (what the fp32 coefficients hold), and the terms per row."""
    rp, tr, tc = tables.rowptr.cpu().numpy(), tables.term_row.cpu().numpy(), tables.term_coef.cpu().numpy()
    m = np.zeros((tables.n_src_rows, tables.n_dst_rows))
    for j in range(tables.n_src_rows):
        for t in range(rp[j], rp[j + 1]):
            m[j, tr[t]] += float(tc[t])
    return m, np.diff(rp)


def field(shape, seed, bf16=False):
    """fp32 values of a few units around an offset (cancellation in b - a, no structure along any axis)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g) * 3.0 + 1.0
    return (x.bfloat16().float() if bf16 else x).numpy()


def normalised(x, norm):
    """x [P, H, W] fp32 -> the loader's numpy fp32 expression per plane, channel = plane mod C."""
    if not norm:
        return x
    c = np.arange(x.shape[0]) % len(BIAS)
    return ((x - BIAS[c, None, None]) / SCALE[c, None, None]).astype(np.float32)


def forward_reference(x, idx, w, norm):
    """(float64 lerp of the fp32 operands with the float64 weights, the per-element bound) for x [P, Hs, W] fp32."""
    xn = normalised(x, norm).astype(np.float64)
    a, b = xn[:, idx], xn[:, idx + 1]
    wk = w[None, :, None]
    ref = a + wk * (b - a)
    grow = np.maximum(1.0, np.maximum(np.abs(w), np.abs(w - 1.0)))[None, :, None]
    return ref, 3.0 * U * (np.abs(a) + np.abs(b)) * grow


def backward_reference(gy, idx, w, hs, norm):
    """(float64 transpose applied to gy [P, Hd, W], the per-element bound, terms per source row)."""
    m = dense_matrix(idx, w, hs)                                  # [Hd, Hs]
    g = gy.astype(np.float64)
    ref = np.einsum("kj,pkw->pjw", m, g)
    mag = np.einsum("kj,pkw->pjw", np.abs(m), np.abs(g))
    terms = np.bincount(np.concatenate([idx, idx + 1]), minlength=hs)
    if norm:
        s = SCALE[np.arange(gy.shape[0]) % len(SCALE)].astype(np.float64)[:, None, None]
        ref, mag = ref / s, mag / np.abs(s)
    return ref, (terms[None, :, None] + 3.0) * U * mag, terms


def assert_within(got, ref, bound, out_dtype, what):
    """fp32 results: every element within ``bound``; bf16 results: ``bf16_elementwise`` with the bound as slack.  Returns the worst
    error in units of the bound (fp32) or of the bf16 criterion."""
    if out_dtype == torch.bfloat16:
        return bf16_elementwise(got, torch.from_numpy(ref), torch.from_numpy(bound), what)
    g = got.double().numpy()
    assert np.isfinite(g).all(), f"{what}: NaN or Inf in the result"
    err = np.abs(g - ref)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max())
    assert worst <= 1.0, f"{what}: worst |y - ref| / bound = {worst:.3f} at {np.unravel_index(int(ratio.argmax()), ratio.shape)}"
    return worst


class Strided:
    """A [P, H, W] field inside a flat buffer: base ``off`` elements past a 16-byte boundary, row stride ``W + pad``, plane stride
    ``H`` rows ``+ pgap``.  ``source(values)`` puts it between NaN bands with NaN in every gap; ``sink()`` gives a guarded
    buffer of sentinels and ``rows(host)`` / ``assert_gaps(host)`` read it back."""

    def __init__(self, P, H, W, off=0, pad=0, pgap=0):
        self.shape, self.off = (P, H, W), off
        self.rs = W + pad
        self.ps = H * self.rs + pgap
        self.n = off + (P - 1) * self.ps + (H - 1) * self.rs + W + 2

    def _view(self, flat):
        return flat.as_strided(self.shape, (self.ps, self.rs, 1), self.off)

    def source(self, values, dtype, dev):
        flat = torch.full((self.n,), float("nan"), dtype=dtype)
        self._view(flat).copy_(torch.as_tensor(values).to(dtype))
        d = poisoned(flat, dev)
        return d, d.data_ptr() + self.off * d.element_size()

    def sink(self, dtype, dev):
        out, check = guarded((self.n,), dtype, dev)
        return out, out.data_ptr() + self.off * out.element_size(), check

    def rows(self, host):
        return self._view(host).clone()

    def assert_gaps(self, host, what):
        gap = torch.ones(self.n, dtype=torch.bool)
        self._view(gap).fill_(False)
        want = torch.full((int(gap.sum()),), SENTINEL, dtype=host.dtype)
        assert torch.equal(host[gap].view(torch.uint8), want.view(torch.uint8)), f"{what}: a store outside the rows"


def code(dtype):
    return {torch.float32: 0, torch.bfloat16: 1}[dtype]


def launch_fwd(dev, x, idx, w, hs, xdtype, ydtype, norm, xlay=(0, 0, 0), ylay=(0, 0, 0), C=3):
    """One ``mk_lat_lerp_fwd`` call on x [P, Hs, W] (numpy fp32 values; bf16 sources must hold bf16 numbers) with LOCAL rows
    ``idx``; layouts are (offset, row pad, plane gap).  Returns the result [P, Hd, W] on the host in ``ydtype``."""
    from makani_amd import _lib
    lib = _lib.load()
    P, _, W = x.shape
    hd = len(idx)
    src, dst = Strided(P, hs, W, *xlay), Strided(P, hd, W, *ylay)
    keep, xptr = src.source(x, xdtype, dev)
    idx_d = torch.from_numpy(np.asarray(idx, dtype=np.int32)).to(dev)
    w_d = poisoned(torch.from_numpy(np.asarray(w, dtype=np.float64).astype(np.float32)), dev)
    b_d = poisoned(torch.from_numpy(BIAS[:C].copy()), dev) if norm else None
    s_d = poisoned(torch.from_numpy(SCALE[:C].copy()), dev) if norm else None
    out, yptr, check = dst.sink(ydtype, dev)
    rc = lib.mk_lat_lerp_fwd(xptr, code(xdtype), src.ps, src.rs, yptr, code(ydtype), dst.ps, dst.rs, idx_d.data_ptr(), w_d.data_ptr(),
                             b_d.data_ptr() if norm else None, s_d.data_ptr() if norm else None, C, P, hs, hd, W,
                             torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "mk_lat_lerp_fwd")
    torch.cuda.synchronize()
    check("mk_lat_lerp_fwd")
    host = out.cpu()
    dst.assert_gaps(host, "mk_lat_lerp_fwd")
    return dst.rows(host)


def launch_bwd(dev, gy, tables, gydtype, gxdtype, norm, glay=(0, 0, 0), xlay=(0, 0, 0), C=3):
    """One ``mk_lat_lerp_bwd`` call on gy [P, Hd, W] with the device tables of ``ops.lat_interp_tables``; returns gx [P, Hs, W]."""
    from makani_amd import _lib
    lib = _lib.load()
    P, hd, W = gy.shape
    hs = tables.n_src_rows
    src, dst = Strided(P, hd, W, *glay), Strided(P, hs, W, *xlay)
    keep, gptr = src.source(gy, gydtype, dev)
    s_d = poisoned(torch.from_numpy(SCALE[:C].copy()), dev) if norm else None
    out, xptr, check = dst.sink(gxdtype, dev)
    rc = lib.mk_lat_lerp_bwd(gptr, code(gydtype), src.ps, src.rs, xptr, code(gxdtype), dst.ps, dst.rs, tables.rowptr.data_ptr(),
                             tables.term_row.data_ptr(), tables.term_coef.data_ptr(), s_d.data_ptr() if norm else None, C, P, hs, hd,
                             W, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "mk_lat_lerp_bwd")
    torch.cuda.synchronize()
    check("mk_lat_lerp_bwd")
    host = out.cpu()
    dst.assert_gaps(host, "mk_lat_lerp_bwd")
    return dst.rows(host)
