"""Autograd operators over the C ABI (include/makani_amd.h).

Tensors cross the boundary as raw device pointers + sizes; torch is only the
allocator and the stream owner.  Every launch goes to torch's *current* HIP
stream, so the ops are capturable in a HIP graph exactly like the reference's
step is captured in ``makani/utils/trainer.py:84-152``.

Private layouts (see the header): ``xf`` = complex64 ``[M, K, BC]``, spectrum =
complex64 ``[L, M, BC]`` (channels last), dhconv weight = complex64 ``[L, I, O]``.
"""
import ctypes
import math
import os
import typing

import numpy as np
import torch

from . import _lib

GRIDS = {"equiangular": 0, "legendre-gauss": 1}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _need_cuda(*tensors):
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError("makani_amd: the spectral ops run only on a HIP device (got a CPU tensor); "
                               "there is no CPU fallback")


_HIP_TORCH, _OFF_ON = ("hip", "torch"), ("0", "1")
# Every switch of the package with a closed value set, and that set (README "Environment knobs" says what each one selects).  The
# free-form variables (MK_COLLECTIVE_TIMEOUT, MK_WGRAD_SPLIT, MK_LIB_OVERRIDE, MK_EXTRA_HIPCC_FLAGS) are read where they are used.
KNOBS = {
    **dict.fromkeys(("MK_PLANAR_FFT", "MK_SPEC_ATTN", "MK_AFNO", "MK_AFNOV1", "MK_ATTN", "MK_ATTN_FP32", "MK_TOKEN_NORM",
                     "MK_TOKEN_LINEAR", "MK_TOKEN_LINEAR_FP32", "MK_PATCH", "MK_ROLLOUT", "MK_STATS", "MK_HIST", "MK_ENSEMBLE", "MK_ENS_LOSS", "MK_ENS_PRODUCTS", "MK_GRID", "MK_NOISE", "MK_ROWSUM", "MK_SPEC_CRPS"),
                    _HIP_TORCH),
    "MK_SPEC_DIAG": ("fused", "public"),
    "MK_SPECTRAL_GEMM": ("bf16x3", "f32"),
    "MK_CONV_ENGINE": ("pce", "blas"),
    "MK_CONV_FP32": ("x3", "torch"),
    "MK_CONV_WGRAD": ("hip", "blas"),
    **dict.fromkeys(("MK_FFT_LEGACY", "MK_IRFFT_SUMS", "MK_IRFFT_AFFINE_ADD", "MK_SPEC_MIX", "MK_NORM_SKIP_FUSION", "MK_MLP_FUSED",
                     "MK_ENGINE_ARENA"), _OFF_ON),
}


def _knob(env, default):
    """The value of switch ``env`` (``default`` where it is unset), read at call time; a value outside ``KNOBS[env]`` is an error."""
    mode, values = os.environ.get(env, default), KNOBS[env]
    if mode not in values:
        raise ValueError(f"unknown {env} {mode!r} ({' | '.join(values)})")
    return mode


def _hip_or_torch(env, default):
    """A family's ``hip | torch`` switch, read and validated at call time; True for ``hip``."""
    return _knob(env, default) == "hip"


def _ptr(t):
    return t.data_ptr() if t is not None else None


_LOWP = (torch.float32, torch.bfloat16)                     # the element types the streaming kernels read and write
_DTYPE_CODE = {torch.float32: 0, torch.bfloat16: 1}         # ... and their codes in the C ABI


def _lowp(t):
    """``t`` as the kernels take it: fp32 and bf16 as they are, anything else as fp32."""
    return t if t.dtype in _LOWP else t.float()


def _f32(t):
    """A detached contiguous fp32 tensor of ``t``; None stays None."""
    return t.detach().float().contiguous() if t is not None else None


def _autocast_dtype():
    """The device's autocast dtype, or None outside autocast."""
    if not torch.is_autocast_enabled():
        return None
    return torch.get_autocast_dtype("cuda") if hasattr(torch, "get_autocast_dtype") else torch.get_autocast_gpu_dtype()


# ----------------------------------------------------------------------------
# host-side precompute (float64 in C, no GPU needed)
# ----------------------------------------------------------------------------
def quadrature(grid, nlat):
    """(colatitudes ascending from the north pole, quadrature weights) as float64 numpy."""
    if grid not in GRIDS:
        raise ValueError(f"Unknown quadrature mode {grid}")
    lib = _lib.load()
    theta = np.empty(nlat, dtype=np.float64)
    w = np.empty(nlat, dtype=np.float64)
    _lib.check(lib.mk_quadrature(GRIDS[grid], nlat, theta.ctypes.data, w.ctypes.data), "mk_quadrature")
    return theta, w


def legendre_kpad(nlat):
    return _lib.load().mk_legendre_kpad(nlat)


def legendre_table(grid, nlat, lmax, mmax, with_quad_weights):
    """fp32 table [mmax, lmax, kpad] (zero padded along k) as a CPU torch tensor."""
    if grid not in GRIDS:
        raise ValueError(f"Unknown quadrature mode {grid}")
    lib = _lib.load()
    kp = lib.mk_legendre_kpad(nlat)
    out = torch.empty(mmax, lmax, kp, dtype=torch.float32)
    _lib.check(lib.mk_legendre_table(GRIDS[grid], nlat, lmax, mmax, int(bool(with_quad_weights)), out.data_ptr()),
               "mk_legendre_table")
    return out


def fft_twiddles(nlon):
    lib = _lib.load()
    out = torch.empty(lib.mk_fft_twiddle_len(nlon), dtype=torch.float32)
    _lib.check(lib.mk_fft_twiddles(nlon, out.data_ptr()), "mk_fft_twiddles")
    return out


def latdft_table(nlat, lmax, first=None):
    """Cosine / sine tables of the truncated latitude DFT of the planar transform (``mk_latdft_table``: the analysis matrix
    ``[2, lmax, pad4(nlat)]`` followed by its transpose ``[2, nlat, pad4(lmax)]``) as a flat fp32 CPU tensor.  ``first``: the
    ``lmax`` frequencies ``(first + l) mod nlat`` in place of the truncation's (``mk_latdft_table_window``: the window of the
    channels-last AFNO)."""
    lib = _lib.load()
    n = lib.mk_latdft_table_len(int(nlat), int(lmax))
    if n <= 0:
        raise ValueError(f"latdft_table: need nlat >= 2 and 2 <= lmax <= nlat, got nlat={nlat}, lmax={lmax}")
    out = torch.empty(n, dtype=torch.float32)
    if first is None:
        _lib.check(lib.mk_latdft_table(int(nlat), int(lmax), out.data_ptr()), "mk_latdft_table")
    else:
        if not 0 <= int(first) < nlat:
            raise ValueError(f"latdft_table: need 0 <= first < nlat, got first={first}, nlat={nlat}")
        _lib.check(lib.mk_latdft_table_window(int(nlat), int(lmax), int(first), out.data_ptr()), "mk_latdft_table_window")
    return out


# ----------------------------------------------------------------------------
# raw (non-differentiable) launches
# ----------------------------------------------------------------------------
def _fft_split(nlon, mmax):
    """The split FFT kernels apply: a production length, no mode above 240, not switched off (``MK_FFT_LEGACY=1``).  They alone
    have bf16 output rows, the peer-major layout, the row statistics and the affine-add epilogue."""
    return nlon in (480, 1440) and mmax <= 241 and _knob("MK_FFT_LEGACY", "0") != "1"


def _xf_dims(xf, kmajor=False, chans=0, cpp=0):
    """(m, k, bc) of contiguous complex64 Fourier rows ``[M, K, BC]``, ``[K, M, BC]`` (``kmajor``) or peer-major
    ``[chans / cpp, K, M, B * cpp]`` (``cpp`` > 0)."""
    assert xf.dim() == (4 if cpp else 3) and xf.is_contiguous() and xf.dtype == torch.complex64
    if cpp:
        _, k, m, bcp = xf.shape
        return m, k, (bcp // cpp) * chans
    return (xf.shape[1], xf.shape[0], xf.shape[2]) if kmajor else tuple(xf.shape)


def rfft_raw(x, twiddles, mmax, s0, sm, sh, kmajor=False):
    """x real [BC, K, N] (fp32 or bf16) -> xf complex64 [mmax, K, BC], or [K, mmax, BC] with ``kmajor``."""
    _need_cuda(x, twiddles)
    assert x.dim() == 3 and x.is_contiguous()
    bc, k, n = x.shape
    xf = torch.empty((k, mmax, bc) if kmajor else (mmax, k, bc), dtype=torch.complex64, device=x.device)
    _lib.check(_lib.load().mk_rfft_ex(x.data_ptr(), _pw_dtype(x), xf.data_ptr(), twiddles.data_ptr(), bc, k, n, mmax,
                                      s0, sm, sh, int(bool(kmajor)), _stream()), "mk_rfft")
    return xf


def irfft_bf16_rows(nlon, mmax):
    """bf16 output rows are built for the production lengths (the split kernels) only."""
    return _fft_split(nlon, mmax)


def irfft_sums_supported(nlon, mmax):
    """The inverse FFT can deliver the row statistics of its output (``mk_irfft_sums``: the split kernels)."""
    return _fft_split(nlon, mmax) and _knob("MK_IRFFT_SUMS", "1") != "0"


def irfft_sums_raw(xf, twiddles, nlon, out_dtype, kmajor=False, chans=0, cpp=0, scale=1.0, exact=False):
    """``irfft`` (scales 1, 1, 1, or ``scale`` three times) of plain (``[M, K, BC]`` / ``[K, M, BC]``) or peer-major (``cpp`` > 0:
    ``[chans / cpp, K, M, B * cpp]``) Fourier rows -> (x ``[BC, K, nlon]``, fp64 ``[BC, 2]`` sums and sums of squares of its rows)."""
    _need_cuda(xf, twiddles)
    m, k, bc = _xf_dims(xf, kmajor, chans, cpp)
    x = torch.empty(bc, k, nlon, dtype=out_dtype, device=xf.device)
    sums = torch.zeros(bc, 2, dtype=torch.float64, device=xf.device)
    if exact:
        # float64 sums of the stored rows, reproducible: per-latitude shares in a workspace, added in a fixed order by a second launch
        ws = torch.empty(k, bc, 2, dtype=torch.float64, device=xf.device)
        _lib.check(_lib.load().mk_irfft_sums_ws(xf.data_ptr(), x.data_ptr(), _pw_dtype(x), twiddles.data_ptr(), bc, k, nlon, m,
                                                scale, scale, scale, int(bool(kmajor)), int(chans), int(cpp), sums.data_ptr(),
                                                ws.data_ptr(), _stream()), "mk_irfft_sums_ws")
        return x, sums
    _lib.check(_lib.load().mk_irfft_sums(xf.data_ptr(), x.data_ptr(), _pw_dtype(x), twiddles.data_ptr(), bc, k, nlon, m,
                                         scale, scale, scale, int(bool(kmajor)), int(chans), int(cpp), sums.data_ptr(),
                                         _stream()), "mk_irfft_sums")
    return x, sums


def irfft_affine_add_supported(nlon, mmax):
    """The inverse FFT can add ``a * z + b`` per row in its store epilogue (``mk_irfft_affine_add``: the split kernels);
    ``MK_IRFFT_AFFINE_ADD=0`` keeps the separate streaming pass (``affine_add``) -- the A/B switch of the variant."""
    return _fft_split(nlon, mmax) and _knob("MK_IRFFT_AFFINE_ADD", "1") != "0"


def irfft_affine_add_raw(xf, twiddles, nlon, z, affine, kmajor=False):
    """``irfft(xf) + a * z + b`` per row: ``xf`` as for ``irfft_raw`` (scales 1, 1, 1), ``z`` a contiguous field of ``BC`` rows
    ``[K, nlon]`` (fp32 / bf16, the dtype of the result), ``affine`` fp32 ``[BC, 2]`` = (a, b) (``instance_norm_coeffs``)."""
    _need_cuda(xf, twiddles, z, affine)
    m, k, bc = _xf_dims(xf, kmajor)
    assert z.is_contiguous() and z.numel() == bc * k * nlon
    assert affine.dtype == torch.float32 and affine.is_contiguous() and affine.numel() == 2 * bc
    x = torch.empty_like(z)
    _lib.check(_lib.load().mk_irfft_affine_add(xf.data_ptr(), x.data_ptr(), _pw_dtype(z), twiddles.data_ptr(), bc, k, nlon, m,
                                               1.0, 1.0, 1.0, int(bool(kmajor)), z.data_ptr(), affine.data_ptr(), _stream()),
               "mk_irfft_affine_add")
    return x


def irfft_raw(xf, twiddles, nlon, s0, sm, sh, out_dtype=torch.float32, kmajor=False):
    """xf complex64 [M, K, BC] ([K, M, BC] with ``kmajor``) -> x [BC, K, nlon] in fp32, or bf16 where the kernel
    fuses the cast."""
    _need_cuda(xf, twiddles)
    m, k, bc = _xf_dims(xf, kmajor)
    fused = out_dtype == torch.bfloat16 and irfft_bf16_rows(nlon, m)
    x = torch.empty(bc, k, nlon, dtype=torch.bfloat16 if fused else torch.float32, device=xf.device)
    _lib.check(_lib.load().mk_irfft_ex(xf.data_ptr(), x.data_ptr(), int(fused), twiddles.data_ptr(), bc, k, nlon, m,
                                       s0, sm, sh, int(bool(kmajor)), _stream()), "mk_irfft")
    return x if x.dtype == out_dtype else x.to(out_dtype)


def fft_pm_supported(nlon, mmax, chans, chans_per_peer):
    """Peer-major Fourier rows (mk_rfft_pm / mk_irfft_pm): split kernels, even channel blocks that are multiples of 24."""
    return _fft_split(nlon, mmax) and chans_per_peer > 0 and chans % chans_per_peer == 0 and chans_per_peer % 24 == 0


def rfft_pm_raw(x, twiddles, mmax, s0, sm, sh, chans, chans_per_peer):
    """x real [B*chans, K, N] -> xf complex64 [chans / cpp, K, mmax, B * cpp] (peer-major, see the header)."""
    _need_cuda(x, twiddles)
    assert x.dim() == 3 and x.is_contiguous()
    bc, k, n = x.shape
    xf = torch.empty(chans // chans_per_peer, k, mmax, (bc // chans) * chans_per_peer, dtype=torch.complex64, device=x.device)
    _lib.check(_lib.load().mk_rfft_pm(x.data_ptr(), _pw_dtype(x), xf.data_ptr(), twiddles.data_ptr(), bc, k, n, mmax,
                                      s0, sm, sh, chans, chans_per_peer, _stream()), "mk_rfft_pm")
    return xf


def irfft_pm_raw(xf, twiddles, nlon, s0, sm, sh, chans, chans_per_peer, out_dtype=torch.float32):
    """xf complex64 [chans / cpp, K, M, B * cpp] -> x [B*chans, K, nlon] (fp32 or bf16 rows)."""
    _need_cuda(xf, twiddles)
    m, k, bc = _xf_dims(xf, True, chans, chans_per_peer)
    fused = out_dtype == torch.bfloat16
    x = torch.empty(bc, k, nlon, dtype=torch.bfloat16 if fused else torch.float32, device=xf.device)
    _lib.check(_lib.load().mk_irfft_pm(xf.data_ptr(), x.data_ptr(), int(fused), twiddles.data_ptr(), bc, k, nlon, m,
                                       s0, sm, sh, chans, chans_per_peer, _stream()), "mk_irfft_pm")
    return x if x.dtype == out_dtype else x.to(out_dtype)


# Arithmetic of the spectral GEMMs (Legendre, dhconv): "bf16x3" = exact three-way bf16 split of every fp32
# operand, six bf16 MFMA products, fp32 accumulation (fp32-accurate, csrc/x3_engine.h and the x3_*.hip families); "f32" = fp32 MFMA
# (csrc/gemm.hip).  Both meet the 1e-5 parity budget; bf16x3 is the faster one on gfx950.
SPECTRAL_GEMM = os.environ.get("MK_SPECTRAL_GEMM", "bf16x3")


def _gemm_mode(mode):
    mode = mode or SPECTRAL_GEMM
    if mode not in KNOBS["MK_SPECTRAL_GEMM"]:
        raise ValueError(f"unknown spectral GEMM mode {mode!r} (bf16x3 | f32)")
    return mode


def legendre_x3_image(table, nlat, inverse):
    """Pre-split tile image of a device fp32 Legendre table (built once, cached on the tensor object).

    The image is built on whatever stream needs it first; the cache entry carries the event recorded behind the
    build, and a hit from another stream waits for it (two micro-batch streams start cold together, pipeline.py)."""
    _need_cuda(table)
    cache = table.__dict__.setdefault("_mk_x3", {})
    key = (int(nlat), int(bool(inverse)))
    entry = cache.get(key)
    if entry is None:
        lib = _lib.load()
        mg, lmax, kp = table.shape
        assert kp == legendre_kpad(nlat) and table.is_contiguous() and table.dtype == torch.float32
        nbytes = lib.mk_legendre_x3_bytes(nlat, lmax, mg, key[1])
        img = torch.empty(nbytes, dtype=torch.uint8, device=table.device)
        _lib.check(lib.mk_legendre_x3_split(table.data_ptr(), img.data_ptr(), nlat, lmax, mg, key[1], _stream()),
                   "mk_legendre_x3_split")
        ev = torch.cuda.Event()
        ev.record()
        cache[key] = entry = [img, ev]
        return img
    if entry[1] is not None:
        if torch.cuda.is_current_stream_capturing():
            # inside a stream capture the event may neither be queried nor waited for (it belongs to uncaptured work:
            # hipErrorStreamCaptureIsolation).  Nothing to do: the build was issued before the capture began, either on this
            # stream (ordered before every replay) or on one the caller has joined before capturing, as for any other input
            return entry[0]
        elif entry[1].query():
            entry[1] = None                     # built and finished: nothing to order any more
        else:
            torch.cuda.current_stream().wait_event(entry[1])
    return entry[0]


def legendre_fwd_raw(xf, table, lmax, m_off=0, mode=None, kmajor=False):
    """xf [Mloc, K, BC] ([K, Mloc, BC] with ``kmajor``: bf16x3 kernels only) -> spectrum [lmax, Mloc, BC]; rows l < m
    are left unwritten."""
    _need_cuda(xf, table)
    assert xf.is_contiguous() and xf.dtype == torch.complex64 and table.dtype == torch.float32
    if kmajor:
        k, mloc, bc = xf.shape
        mode = "bf16x3"
    else:
        mloc, k, bc = xf.shape
    mg, lt, kp = table.shape
    assert lt == lmax and kp == legendre_kpad(k), "Legendre table does not match the operand"
    c = torch.empty(lmax, mloc, bc, dtype=torch.complex64, device=xf.device)
    if _gemm_mode(mode) == "bf16x3":
        img = legendre_x3_image(table, k, 0)
        _lib.check(_lib.load().mk_legendre_fwd_x3_ex(xf.data_ptr(), img.data_ptr(), c.data_ptr(), bc, k, lmax, mloc,
                                                     m_off, mg, int(bool(kmajor)), _stream()), "mk_legendre_fwd_x3")
    else:
        _lib.check(_lib.load().mk_legendre_fwd(xf.data_ptr(), table.data_ptr(), c.data_ptr(), bc, k, lmax, mloc,
                                               m_off, mg, _stream()), "mk_legendre_fwd")
    return c


def legendre_inv_raw(c, table, nlat, m_off=0, mode=None, kmajor=False):
    """spectrum [L, Mloc, BC] -> xf [Mloc, nlat, BC] ([nlat, Mloc, BC] with ``kmajor``: bf16x3 kernels only)."""
    _need_cuda(c, table)
    assert c.is_contiguous() and c.dtype == torch.complex64 and table.dtype == torch.float32
    lmax, mloc, bc = c.shape
    mg, lt, kp = table.shape
    assert lt == lmax and kp == legendre_kpad(nlat), "Legendre table does not match the operand"
    xf = torch.empty((nlat, mloc, bc) if kmajor else (mloc, nlat, bc), dtype=torch.complex64, device=c.device)
    if kmajor:
        mode = "bf16x3"
    if _gemm_mode(mode) == "bf16x3":
        img = legendre_x3_image(table, nlat, 1)
        _lib.check(_lib.load().mk_legendre_inv_x3_ex(c.data_ptr(), img.data_ptr(), xf.data_ptr(), bc, nlat, lmax, mloc,
                                                     m_off, mg, int(bool(kmajor)), _stream()), "mk_legendre_inv_x3")
    else:
        _lib.check(_lib.load().mk_legendre_inv(c.data_ptr(), table.data_ptr(), xf.data_ptr(), bc, nlat, lmax, mloc,
                                               m_off, mg, _stream()), "mk_legendre_inv")
    return xf


def _latdft_check(a, table, nlat, lmax):
    _need_cuda(a, table)
    assert a.dim() == 3 and a.is_contiguous() and a.dtype == torch.complex64
    assert table.dtype == torch.float32 and table.is_contiguous()
    assert table.numel() == _lib.load().mk_latdft_table_len(int(nlat), int(lmax)), "latitude DFT table does not match the operand"


def lat_dft_raw(xf, table, lmax):
    """Latitude-major Fourier rows xf ``[nlat, M, BC]`` -> private spectrum ``[lmax, M, BC]`` of the planar transform."""
    nlat, m, bc = xf.shape
    _latdft_check(xf, table, nlat, lmax)
    c = torch.empty(lmax, m, bc, dtype=torch.complex64, device=xf.device)
    _lib.check(_lib.load().mk_latdft_fwd(xf.data_ptr(), table.data_ptr(), c.data_ptr(), nlat, lmax, m * bc, _stream()),
               "mk_latdft_fwd")
    return c


def lat_idft_raw(c, table, nlat):
    """Private spectrum ``[lmax, M, BC]`` -> latitude-major Fourier rows ``[nlat, M, BC]`` (the adjoint of ``lat_dft_raw``)."""
    lmax, m, bc = c.shape
    _latdft_check(c, table, nlat, lmax)
    xf = torch.empty(nlat, m, bc, dtype=torch.complex64, device=c.device)
    _lib.check(_lib.load().mk_latdft_inv(c.data_ptr(), table.data_ptr(), xf.data_ptr(), nlat, lmax, m * bc, _stream()),
               "mk_latdft_inv")
    return xf


def spec_pack_raw(c_std):
    """[BC, L, M] complex64 -> [L, M, BC]."""
    _need_cuda(c_std)
    assert c_std.dim() == 3 and c_std.is_contiguous() and c_std.dtype == torch.complex64
    bc, l, m = c_std.shape
    out = torch.empty(l, m, bc, dtype=torch.complex64, device=c_std.device)
    _lib.check(_lib.load().mk_spec_pack(c_std.data_ptr(), out.data_ptr(), bc, l, m, _stream()), "mk_spec_pack")
    return out


def spec_unpack_raw(c_prv, l_off=0, m_off=0):
    """[L, M, BC] complex64 -> [BC, L, M], exact zeros where l_off + l < m_off + m."""
    _need_cuda(c_prv)
    assert c_prv.dim() == 3 and c_prv.is_contiguous() and c_prv.dtype == torch.complex64
    l, m, bc = c_prv.shape
    out = torch.empty(bc, l, m, dtype=torch.complex64, device=c_prv.device)
    _lib.check(_lib.load().mk_spec_unpack(c_prv.data_ptr(), out.data_ptr(), bc, l, m, l_off, m_off, _stream()),
               "mk_spec_unpack")
    return out


def _w_phys(w):
    """Physical [L, I, O] contiguous view/copy of a dhconv weight of logical shape [I, O, L]."""
    wp = w.permute(2, 0, 1)
    return wp if wp.is_contiguous() else wp.contiguous()


def _dh_fn(name, mode, cin, cout):
    """bf16x3 kernels need even channel counts; odd ones take the fp32 MFMA kernels."""
    if _gemm_mode(mode) == "bf16x3" and cin % 2 == 0 and cout % 2 == 0:
        name += "_x3"
    return getattr(_lib.load(), name), name


def dhconv_fwd_raw(x, w_phys, batch, l_off=0, m_off=0, mode=None):
    _need_cuda(x, w_phys)
    assert x.is_contiguous() and x.dtype == torch.complex64 and w_phys.is_contiguous() and w_phys.dtype == torch.complex64
    lloc, mloc, bc = x.shape
    l2, cin, cout = w_phys.shape
    assert l2 == lloc and bc == batch * cin, "dhconv operand shapes do not match"
    y = torch.empty(lloc, mloc, batch * cout, dtype=torch.complex64, device=x.device)
    fn, name = _dh_fn("mk_dhconv_fwd", mode, cin, cout)
    _lib.check(fn(x.data_ptr(), w_phys.data_ptr(), y.data_ptr(), lloc, mloc, batch, cin, cout, l_off, m_off, _stream()), name)
    return y


def dhconv_dgrad_raw(gy, w_phys, batch, l_off=0, m_off=0, mode=None):
    _need_cuda(gy, w_phys)
    assert gy.is_contiguous() and gy.dtype == torch.complex64 and w_phys.is_contiguous()
    lloc, mloc, bo = gy.shape
    l2, cin, cout = w_phys.shape
    assert l2 == lloc and bo == batch * cout
    gx = torch.empty(lloc, mloc, batch * cin, dtype=torch.complex64, device=gy.device)
    fn, name = _dh_fn("mk_dhconv_dgrad", mode, cin, cout)
    _lib.check(fn(gy.data_ptr(), w_phys.data_ptr(), gx.data_ptr(), lloc, mloc, batch, cin, cout, l_off, m_off, _stream()), name)
    return gx


def dhconv_wgrad_raw(x, gy, batch, l_off=0, m_off=0, mode=None):
    _need_cuda(x, gy)
    assert x.is_contiguous() and gy.is_contiguous() and x.dtype == torch.complex64 and gy.dtype == torch.complex64
    lloc, mloc, bi = x.shape
    cin, cout = bi // batch, gy.shape[2] // batch
    gw = torch.empty(lloc, cin, cout, dtype=torch.complex64, device=x.device)
    fn, name = _dh_fn("mk_dhconv_wgrad", mode, cin, cout)
    _lib.check(fn(x.data_ptr(), gy.data_ptr(), gw.data_ptr(), lloc, mloc, batch, cin, cout, l_off, m_off, _stream()), name)
    return gw


def _diag_launch(name, a, b, out, batch, cin, cout, p):
    _lib.check(getattr(_lib.load(), name)(a.data_ptr(), b.data_ptr(), out.data_ptr(), batch, cin, cout, p, _stream()), name)
    return out


class _DiagContract(torch.autograd.Function):
    """y[b,o,l,m] = sum_i x[b,i,l,m] w[i,o,l,m] on the public layout (mk_diag_*)."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        b, i, l, m = x.shape
        o = w.shape[1]
        y = torch.empty(b, o, l, m, dtype=torch.complex64, device=x.device)
        return _diag_launch("mk_diag_fwd", x, w, y, b, i, o, l * m)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        b, i, l, m = x.shape
        o = w.shape[1]
        gy = gy.contiguous()
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = _diag_launch("mk_diag_dgrad", gy, w, torch.empty_like(x), b, i, o, l * m)
        if ctx.needs_input_grad[1]:
            gw = _diag_launch("mk_diag_wgrad", x, gy, torch.empty_like(w), b, i, o, l * m)
        return gx, gw


def diag_contract(x, w):
    """``einsum("bixy,ioxy->boxy")`` for complex64 x [B,I,L,M], w [I,O,L,M] on the HIP streaming kernels."""
    _need_cuda(x, w)
    if x.dtype != torch.complex64 or w.dtype != torch.complex64:
        raise TypeError("diag_contract expects complex64 operands")
    if x.dim() != 4 or w.dim() != 4 or x.shape[1] != w.shape[0] or tuple(x.shape[2:]) != tuple(w.shape[2:]):
        raise ValueError(f"diag_contract: incompatible shapes {tuple(x.shape)} and {tuple(w.shape)}")
    return _DiagContract.apply(x.contiguous(), w.contiguous())


# ----------------------------------------------------------------------------
# the diagonal filter on the private spectrum (mk_spec_diag_*): no layout round trip, the weight as the parameter stores it
# ----------------------------------------------------------------------------
# Opt-in: the default is flipped under the rule of DESIGN section 19 (no measured row of tools/specdiag_bench.py slower) in a
# change of its own.
SPEC_DIAG_DEFAULT = "public"


def spec_diag_fused():
    """``MK_SPEC_DIAG=fused|public`` (read at call time): the diagonal filter of ``SpectralConv`` on the private spectrum
    (``mk_spec_diag_*`` between ``forward_packed`` and ``inverse_packed``), or through the public layout (``mk_diag_*``)."""
    return _knob("MK_SPEC_DIAG", SPEC_DIAG_DEFAULT) == "fused"


def spec_diag_supported(c, w):
    """The ``mk_spec_diag_*`` kernels take these operands: contiguous complex64 tensors on a HIP device."""
    return all(t.is_cuda and t.dtype == torch.complex64 and t.is_contiguous() for t in (c, w))


def _spec_diag_args(s, batch, w_shape):
    """(lloc, mloc, cin, cout) of a private spectrum ``[L, M, batch * C]`` next to a weight of shape ``[I, O, L, M]``."""
    assert s.dim() == 3 and s.is_contiguous() and s.dtype == torch.complex64 and len(w_shape) == 4
    cin, cout, lloc, mloc = (int(v) for v in w_shape)
    assert (s.shape[0], s.shape[1]) == (lloc, mloc) and s.shape[2] % batch == 0, "spec_diag operand shapes do not match"
    return lloc, mloc, cin, cout


def _spec_diag_launch(name, a, b, out, lloc, mloc, batch, cin, cout, l_off, m_off, dense):
    _lib.check(getattr(_lib.load(), name)(a.data_ptr(), b.data_ptr(), out.data_ptr(), lloc, mloc, batch, cin, cout, int(l_off),
                                          int(m_off), int(bool(dense)), _stream()), name)
    return out


def spec_diag_fwd_raw(x, w, batch, l_off=0, m_off=0, dense=False, out=None):
    """y[l, m, b, o] = sum_i x[l, m, b, i] w[i, o, l, m]; entries with global l < m (``dense`` False) are left unwritten."""
    _need_cuda(x, w)
    assert w.is_contiguous() and w.dtype == torch.complex64
    lloc, mloc, cin, cout = _spec_diag_args(x, batch, w.shape)
    assert x.shape[2] == batch * cin, "spec_diag operand shapes do not match"
    y = torch.empty(lloc, mloc, batch * cout, dtype=torch.complex64, device=x.device) if out is None else out
    return _spec_diag_launch("mk_spec_diag_fwd", x, w, y, lloc, mloc, batch, cin, cout, l_off, m_off, dense)


def spec_diag_dgrad_raw(gy, w, batch, l_off=0, m_off=0, dense=False, out=None):
    """gx[l, m, b, i] = sum_o gy[l, m, b, o] conj(w[i, o, l, m]); entries with global l < m are left unwritten."""
    _need_cuda(gy, w)
    assert w.is_contiguous() and w.dtype == torch.complex64
    lloc, mloc, cin, cout = _spec_diag_args(gy, batch, w.shape)
    assert gy.shape[2] == batch * cout, "spec_diag operand shapes do not match"
    gx = torch.empty(lloc, mloc, batch * cin, dtype=torch.complex64, device=gy.device) if out is None else out
    return _spec_diag_launch("mk_spec_diag_dgrad", gy, w, gx, lloc, mloc, batch, cin, cout, l_off, m_off, dense)


def spec_diag_wgrad_raw(x, gy, batch, l_off=0, m_off=0, dense=False, out=None):
    """gw[i, o, l, m] = sum_b conj(x[l, m, b, i]) gy[l, m, b, o] in the parameter's layout; exact zeros where global l < m."""
    _need_cuda(x, gy)
    cin, cout = x.shape[2] // batch, gy.shape[2] // batch
    lloc, mloc, _, _ = _spec_diag_args(x, batch, (cin, cout, x.shape[0], x.shape[1]))
    _spec_diag_args(gy, batch, (cin, cout, lloc, mloc))
    assert x.shape[2] == batch * cin and gy.shape[2] == batch * cout, "spec_diag operand shapes do not match"
    gw = torch.empty(cin, cout, lloc, mloc, dtype=torch.complex64, device=x.device) if out is None else out
    return _spec_diag_launch("mk_spec_diag_wgrad", x, gy, gw, lloc, mloc, batch, cin, cout, l_off, m_off, dense)


class _SpecDiag(torch.autograd.Function):
    """y[l, m, b, o] = sum_i x[l, m, b, i] w[i, o, l, m] on the private layout (mk_spec_diag_*)."""

    @staticmethod
    def forward(ctx, x, w, batch, l_off, m_off, dense):
        ctx.save_for_backward(x, w)
        ctx.args = (batch, l_off, m_off, dense)
        return spec_diag_fwd_raw(x, w, batch, l_off, m_off, dense)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = gy.contiguous()
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = spec_diag_dgrad_raw(gy, w, *ctx.args)
        if ctx.needs_input_grad[1]:
            gw = spec_diag_wgrad_raw(x, gy, *ctx.args)
        return gx, gw, None, None, None, None


def spec_diag(c, w, batch, l_off=0, m_off=0, dense=False):
    """The diagonal filter ``einsum("bixy,ioxy->boxy")`` on the private spectrum ``c`` ``[L, M, batch * I]`` with the parameter
    ``w`` ``[I, O, L, M]`` as stored -> ``[L, M, batch * O]``.  The weight gradient comes back in the parameter's layout, the
    spectrum gradient in the private layout.  ``l_off`` / ``m_off``: the global indices of a shard's first degree / order;
    ``dense``: every entry is data (the planar pair), otherwise entries with global l < m are neither read nor written."""
    _need_cuda(c, w)
    if not spec_diag_supported(c, w):
        raise TypeError("spec_diag expects contiguous complex64 operands (spec_diag_supported)")
    return _SpecDiag.apply(c, w, batch, l_off, m_off, dense)


# ----------------------------------------------------------------------------
# 1x1 convolutions on fp32 fields: the bf16x3 engine of the spectral GEMMs (fp32-accurate, no vendor GEMM)
# ----------------------------------------------------------------------------
def _pad4(w):
    """[M, K] fp32 -> contiguous [M, K4] with K4 = K rounded up to 4 (zero columns): 16-byte aligned rows for the row stager."""
    k4 = (w.shape[1] + 3) // 4 * 4
    if k4 == w.shape[1] and w.is_contiguous():
        return w
    out = w.new_zeros(w.shape[0], k4)
    out[:, :w.shape[1]].copy_(w)
    return out


def conv1x1_x3_supported(x3):
    """fp32 ``[B, K, P]`` contiguous field on the GPU with an even pixel count."""
    return x3.is_cuda and x3.dtype == torch.float32 and x3.dim() == 3 and x3.is_contiguous() and x3.shape[2] % 2 == 0


def conv1x1_x3(w, x3, out=None, bias=None, gelu=False):
    """y[b] = w @ x3[b] (``out`` given: ``out[b] += w @ x3[b]`` in place): w fp32 ``[M, K]``, x3 fp32 ``[B, K, P]`` (``mk_conv1x1_x3``).
    ``bias`` / ``gelu`` (not with ``out``): ``y = act(w @ x3 + bias)`` in the kernel's epilogue (``mk_conv1x1_x3_bias_act``)."""
    _need_cuda(w, x3)
    assert w.dtype == torch.float32 and w.dim() == 2 and conv1x1_x3_supported(x3) and w.shape[1] == x3.shape[1]
    b, k, p = x3.shape
    m = w.shape[0]
    a = _pad4(w)
    if bias is not None or gelu:
        assert out is None
        bf = None if bias is None else bias.detach().float().contiguous()
        assert bf is None or bf.numel() == m
        y = torch.empty(b, m, p, dtype=torch.float32, device=x3.device)
        _lib.check(_lib.load().mk_conv1x1_x3_bias_act(a.data_ptr(), a.stride(0), x3.data_ptr(), p, y.data_ptr(), p, m, k, p, b, k * p,
                                                      m * p, _ptr(bf), int(bool(gelu)), _stream()),
                   "mk_conv1x1_x3_bias_act")
        return y
    if out is not None:
        assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (b, m, p)
    y = out if out is not None else torch.empty(b, m, p, dtype=torch.float32, device=x3.device)
    _lib.check(_lib.load().mk_conv1x1_x3(a.data_ptr(), a.stride(0), x3.data_ptr(), p, y.data_ptr(), p, m, k, p, b, 0, k * p,
                                         m * p, 1 if out is not None else 0, _stream()), "mk_conv1x1_x3")
    return y


def conv1x1_x3_wgrad(gy, x3):
    """gW[o][i] = sum_{b,p} gy[b][o][p] x3[b][i][p] for fp32 fields (P a multiple of 4): fp32 ``[O, I]``."""
    _need_cuda(gy, x3)
    assert gy.dtype == torch.float32 and x3.dtype == torch.float32 and gy.is_contiguous() and x3.is_contiguous()
    b, o, p = gy.shape
    i = x3.shape[1]
    assert p % 4 == 0 and x3.shape[0] == b and x3.shape[2] == p
    gw = torch.zeros(o, i, dtype=torch.float32, device=gy.device)
    _lib.check(_lib.load().mk_conv1x1_x3(gy.data_ptr(), p, x3.data_ptr(), p, gw.data_ptr(), i, o, p, i, b, o * p, i * p, 0, 2,
                                         _stream()), "mk_conv1x1_x3")
    return gw


# ----------------------------------------------------------------------------
# per-step arena of the pointwise stack: every packed weight image in ONE launch, every weight-gradient buffer in ONE fill
# ----------------------------------------------------------------------------
_ACTIVE_ARENA = None


class EngineArena:
    """What the 1x1 convolutions of one net need per step besides their GEMMs, batched: the MFMA fragment images of every
    weight in both orientations (``mk_pce_pack_batch``: one launch instead of one ``mk_pce_pack`` per GEMM) and the zeroed
    fp32 buffers the weight-gradient kernels accumulate into (one fill instead of one per layer).

    ``with arena.scope():`` around a forward pass refreshes the images from the CURRENT weights (always: no invalidation
    protocol to get wrong) and makes ``pce_pack`` / ``conv1x1_wgrad_raw`` find them; the autograd nodes take what their
    backward pass needs (transposed image, gradient buffer) while the scope is open.  Outside a scope -- a layer called on its
    own, a checkpoint recomputation -- every call packs / allocates for itself as before."""

    def __init__(self, weights):
        # detached: only addresses and shapes are kept.  (A `weight.view(out, in)` of a parameter carries a grad_fn that holds
        # the parameter's AccumulateGrad node; keeping it across steps pins that node to the stream of the first step and a
        # later capture on another stream dies in capture_end -- the round-1 crash)
        self.weights = [w.detach() for w in weights if w.is_cuda and w.dim() == 2 and w.stride(1) == 1
                        and w.dtype in _LOWP]
        lib = _lib.load()
        rows, self.slots, off, goff = [], {}, 0, 0
        self.gslots = {}
        self.n_fwd = self.total_fwd = 0
        for transpose in (False, True):            # the forward images first: inference (grad mode off) packs only those
            for w in self.weights:
                m, k = (w.shape[1], w.shape[0]) if transpose else (w.shape[0], w.shape[1])
                nbytes = lib.mk_pce_image_bytes(m, k)
                if nbytes <= 0:
                    continue
                lay = (ctypes.c_longlong * 3)()
                _lib.check(lib.mk_pce_pack_layout(m, k, lay), "mk_pce_pack_layout")
                rows.append([w.data_ptr(), 0 if w.dtype == torch.float32 else 1, int(transpose), m, k, w.stride(0), lay[0], lay[1],
                             lay[2], off])
                self.slots[self._key(w, transpose)] = (off * 2, nbytes)
                off += nbytes // 2
            if not transpose:
                self.n_fwd, self.total_fwd = len(rows), off
        for w in self.weights:
            self.gslots[self._key(w, False)] = (goff, w.shape[0], w.shape[1])
            goff += (w.numel() + 3) // 4 * 4           # 16-byte aligned buffers
        self.total, self.gtotal = off, goff
        self.n = len(rows)
        dev = self.weights[0].device if self.weights else None
        self.desc = torch.tensor(rows + [[0] * 9 + [off]], dtype=torch.int64).to(dev) if rows else None
        self.images = torch.empty(2 * off, dtype=torch.uint8, device=dev) if rows else None
        self.gbuf = None
        self._prev = None

    @staticmethod
    def _key(w, transpose):
        return (w.data_ptr(), tuple(w.shape), w.stride(0), w.dtype, bool(transpose))

    def refresh(self, with_grad_buffers):
        n, total = (self.n, self.total) if with_grad_buffers else (self.n_fwd, self.total_fwd)
        self._packed_all = bool(with_grad_buffers)
        if n:
            _lib.check(_lib.load().mk_pce_pack_batch(self.desc.data_ptr(), n, self.images.data_ptr(), total, _stream()),
                       "mk_pce_pack_batch")
        # a fresh buffer per step: the views handed out become the parameters' gradients and live as long as those do
        self.gbuf = torch.zeros(self.gtotal, dtype=torch.float32, device=self.images.device) if (with_grad_buffers and self.gtotal) else None

    def image(self, w, transpose):
        if transpose and not self._packed_all:       # grad mode was off at scope entry: the transposed images are stale
            return None
        slot = self.slots.get(self._key(w, transpose))
        return None if slot is None else self.images[slot[0]:slot[0] + slot[1]]

    def grad_buffer(self, w):
        """Zeroed fp32 ``[out, in]`` buffer for the gradient of ``w`` -- once per step (a second request gets None: the
        caller then allocates, e.g. a weight used twice in one forward pass)."""
        slot = self.gslots.get(self._key(w, False))
        if slot is None or self.gbuf is None or slot[0] in self._taken:
            return None
        self._taken.add(slot[0])
        return self.gbuf[slot[0]:slot[0] + slot[1] * slot[2]].view(slot[1], slot[2])

    def scope(self):
        return _ArenaScope(self)


class _ArenaScope:
    def __init__(self, arena):
        self.arena = arena

    def __enter__(self):
        global _ACTIVE_ARENA
        self.arena._prev, _ACTIVE_ARENA = _ACTIVE_ARENA, self.arena
        self.arena._taken = set()
        self.arena.refresh(torch.is_grad_enabled())
        return self.arena

    def __exit__(self, *exc):
        global _ACTIVE_ARENA
        _ACTIVE_ARENA = self.arena._prev
        return False


def arena_image(w, transpose=False):
    """The packed image of ``w`` from the open arena scope, or None."""
    return None if _ACTIVE_ARENA is None else _ACTIVE_ARENA.image(w, transpose)


def arena_grad_buffer(w):
    return None if _ACTIVE_ARENA is None else _ACTIVE_ARENA.grad_buffer(w)


def conv1x1_wgrad_raw(gy, x3, x_gelu=False, out=None):
    """gW[o][i] = sum_{b,p} gy[b][o][p] act(x3[b][i][p]): bf16 [B,O,P], [B,I,P] -> fp32 [O,I] (HIP bf16 MFMA kernel);
    ``x_gelu``: act = exact GELU rounded to bf16, applied while x3 is staged (x3 is then the kept pre-activation of an MLP;
    O <= 384).  ``out``: accumulate into this zeroed buffer instead of a fresh one."""
    _need_cuda(gy, x3)
    assert gy.is_contiguous() and x3.is_contiguous() and gy.dtype == torch.bfloat16 and x3.dtype == torch.bfloat16
    b, o, p = gy.shape
    i = x3.shape[1]
    if out is not None:      # a zeroed fp32 [O, I] buffer (EngineArena.grad_buffer)
        assert out.dtype == torch.float32 and tuple(out.shape) == (o, i) and out.is_contiguous()
    gw = out if out is not None else torch.zeros(o, i, dtype=torch.float32, device=x3.device)
    _lib.check(_lib.load().mk_conv1x1_wgrad_act(gy.data_ptr(), x3.data_ptr(), gw.data_ptr(), b, o, i, p, int(bool(x_gelu)),
                                                _stream()), "mk_conv1x1_wgrad_act")
    return gw


# ----------------------------------------------------------------------------
# pixel-column engine (csrc/pce.hip): 1x1 convolutions with fused epilogues
# ----------------------------------------------------------------------------
def pce_supported(m, k):
    """One GEMM ``[m, k] @ [k, P]`` the engine is built for: K <= 768, M <= 1536."""
    return _lib.load().mk_pce_image_bytes(int(m), int(k)) > 0


def pce_supported_train(out_channels, in_channels):
    """A 1x1 convolution the engine can run in BOTH directions: forward ``[out, in]`` and the data gradient, the
    transposed GEMM ``[in, out]`` (K' = out <= 768, M' = in <= 1536).  Layers that pass only the forward check
    (e.g. 768 -> 1536, the fc1 of ``sfno_dhealy_73ch_edim768``) must take the fallback path as a whole: the
    autograd node packs the transposed image in backward."""
    return pce_supported(out_channels, in_channels) and pce_supported(in_channels, out_channels)


def pce_pack(w, transpose=False):
    """MFMA fragment image of A = w (``[M, K]``) or A = w^T (``w`` is ``[K, M]``); fp32 or bf16 weights.  Inside an
    ``EngineArena`` scope that holds ``w`` the image comes from the arena's batched launch."""
    _need_cuda(w)
    img = arena_image(w, transpose)
    if img is not None:
        return img
    assert w.dim() == 2 and w.stride(1) == 1 and w.dtype in _LOWP
    m, k = (w.shape[1], w.shape[0]) if transpose else (w.shape[0], w.shape[1])
    lib = _lib.load()
    nbytes = lib.mk_pce_image_bytes(m, k)
    if nbytes <= 0:
        raise ValueError(f"pce_pack: unsupported GEMM shape M={m}, K={k}")
    img = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    _lib.check(lib.mk_pce_pack(w.data_ptr(), 0 if w.dtype == torch.float32 else 1, int(bool(transpose)), m, k, w.stride(0),
                               img.data_ptr(), _stream()), "mk_pce_pack")
    return img


def pce_mlp_supported(m, hd, k1):
    """Shapes of the fused conv -> GELU -> conv node (csrc/pce_mlp.hip): K1 <= 384, Hd <= 768, M <= 384."""
    return _lib.load().mk_pce_mlp_image_bytes(int(m), int(hd), int(k1)) > 0


def pce_mlp_pack(a1, a1_transposed, a2, a2_transposed):
    """Weight stream image of the fused node: ``A1 [Hd, K1]`` = ``a1`` (or ``a1^T`` when ``a1_transposed``: ``a1`` is
    ``[K1, Hd]``), ``A2 [M, Hd]`` = ``a2`` (or ``a2^T``: ``a2`` is ``[Hd, M]``).  Returns ``(image, M, Hd, K1)``."""
    _need_cuda(a1, a2)
    assert a1.dim() == 2 and a2.dim() == 2 and a1.stride(1) == 1 and a2.stride(1) == 1 and a1.dtype == a2.dtype
    assert a1.dtype in _LOWP
    hd, k1 = (a1.shape[1], a1.shape[0]) if a1_transposed else (a1.shape[0], a1.shape[1])
    m, hd2 = (a2.shape[1], a2.shape[0]) if a2_transposed else (a2.shape[0], a2.shape[1])
    assert hd == hd2, "the two matrices do not share the hidden dimension"
    lib = _lib.load()
    nbytes = lib.mk_pce_mlp_image_bytes(m, hd, k1)
    if nbytes <= 0:
        raise ValueError(f"pce_mlp_pack: unsupported shape M={m}, Hd={hd}, K1={k1}")
    img = torch.empty(nbytes, dtype=torch.uint8, device=a1.device)
    _lib.check(lib.mk_pce_mlp_pack(a1.data_ptr(), int(bool(a1_transposed)), a1.stride(0), a2.data_ptr(), int(bool(a2_transposed)),
                                   a2.stride(0), 0 if a1.dtype == torch.float32 else 1, m, hd, k1, img.data_ptr(), _stream()),
               "mk_pce_mlp_pack")
    return img, m, hd, k1


def pce_mlp(x3, packed, mode, b1=None, b2=None, pre=None, want_row_sums=False, want_mid_sums=False):
    """The fused node on bf16 ``[B, K1, P]`` fields (``mk_pce_mlp``).  ``mode`` 0: returns ``(y, pre[, sums])`` with
    ``pre = A1 x + b1`` and ``y = A2 gelu(pre) + b2``; ``mode`` 1 (``x3`` = output gradient, ``pre`` = the kept pre-activation):
    returns ``(gx, gpre[, gpre_sums])`` with ``gpre = (A1 x) * gelu'(pre)``, ``gx = A2 gpre`` and the fp64 ``[B * Hd]`` pixel sums
    of ``gpre``."""
    img, m, hd, k1 = packed
    _need_cuda(x3, img)
    assert x3.dim() == 3 and x3.is_contiguous() and x3.dtype == torch.bfloat16 and x3.shape[1] == k1
    b, _, p = x3.shape
    if mode == 1:
        assert pre is not None and pre.is_contiguous() and pre.dtype == torch.bfloat16 and tuple(pre.shape) == (b, hd, p)
    bf1 = None if b1 is None else b1.detach().float().contiguous()
    bf2 = None if b2 is None else b2.detach().float().contiguous()
    assert (bf1 is None or bf1.numel() == hd) and (bf2 is None or bf2.numel() == m)
    y = torch.empty(b, m, p, dtype=torch.bfloat16, device=x3.device)
    mid = torch.empty(b, hd, p, dtype=torch.bfloat16, device=x3.device)
    sums = torch.empty(b * m, 2, dtype=torch.float64, device=x3.device) if want_row_sums else None
    msum = torch.empty(b * hd, dtype=torch.float64, device=x3.device) if want_mid_sums else None
    _lib.check(_lib.load().mk_pce_mlp(x3.data_ptr(), img.data_ptr(), y.data_ptr(), mid.data_ptr(),
                                      _ptr(pre), _ptr(bf1), _ptr(bf2), _ptr(sums), _ptr(msum), int(mode), b, m, hd, k1, p, _stream()),
               "mk_pce_mlp")
    return (y, mid) + ((sums,) if want_row_sums else ()) + ((msum,) if want_mid_sums else ())


_ZERO_BIAS = {}


def _zero_bias(device):
    z = _ZERO_BIAS.get(device)
    if z is None:
        z = _ZERO_BIAS[device] = torch.zeros(1024, dtype=torch.float32, device=device)
    return z


def pce_gemm(x3, wimg, m, bias=None, addend=None, aux_in=None, want_pre=False, gelu=False, want_row_sums=False,
             addend_affine=None):
    """y[b] = epi(A @ x3[b]) on bf16 ``[B, K, P]`` fields (see ``mk_pce_gemm_ex``).  Returns ``y``, followed by ``pre``
    (the bf16 pre-activation ``A x + bias``) when ``want_pre`` and by the fp64 ``[B * M, 2]`` row sums (sum, sum of squares
    over the pixels of ``y``) when ``want_row_sums``.  ``addend_affine`` (fp32 ``[B * M, 2]``) lets the addend enter as
    ``a * addend + b`` per row (``instance_norm_coeffs``)."""
    _need_cuda(x3, wimg)
    assert x3.dim() == 3 and x3.is_contiguous() and x3.dtype == torch.bfloat16
    b, k, p = x3.shape
    for t in (addend, aux_in):
        if t is not None:
            assert t.is_contiguous() and t.dtype == torch.bfloat16 and tuple(t.shape) == (b, m, p)
    bf = _zero_bias(x3.device)   # the epilogue loads a bias unconditionally: zeros for layers without one
    if bias is not None:      # fp32 [m]
        bf = bias.detach().float().contiguous()
        assert bf.numel() == m
    y = torch.empty(b, m, p, dtype=torch.bfloat16, device=x3.device)
    pre = torch.empty_like(y) if want_pre else None
    sums = torch.empty(b * m, 2, dtype=torch.float64, device=x3.device) if want_row_sums else None
    if addend_affine is not None:
        assert (addend is not None and addend_affine.dtype == torch.float32 and addend_affine.is_contiguous()
                and addend_affine.numel() == 2 * b * m)
    _lib.check(_lib.load().mk_pce_gemm_ex(x3.data_ptr(), wimg.data_ptr(), y.data_ptr(), bf.data_ptr(),
                                          _ptr(addend), _ptr(addend_affine), _ptr(aux_in), _ptr(pre), int(bool(gelu)),
                                          _ptr(sums), b, m, k, p, _stream()),
               "mk_pce_gemm_ex")
    out = (y,) + ((pre,) if want_pre else ()) + ((sums,) if want_row_sums else ())
    return out if len(out) > 1 else y


# ----------------------------------------------------------------------------
# differentiable operators (all linear in the data: backward = adjoint launch)
# ----------------------------------------------------------------------------
class _RFFT(torch.autograd.Function):
    """x [BC, K, N] -> 2 pi rfft(x, norm="forward")[..., :mmax] (K1) as Fourier rows [mmax, K, BC], [K, mmax, BC] (``kmajor``) or,
    with ``pm`` = (chans, cpp), peer-major; the adjoint is the inverse launch from the same layout.  ``scale`` replaces the
    factor 2 pi / N on every mode (the planar transform passes 1 / sqrt(N))."""

    @staticmethod
    def forward(ctx, x, twiddles, mmax, kmajor=False, pm=None, scale=None):
        ctx.save_for_backward(twiddles)
        ctx.cfg = (x.shape[-1], x.dtype, kmajor, pm, scale)
        s = 2.0 * math.pi / x.shape[-1] if scale is None else float(scale)
        if pm:
            return rfft_pm_raw(x, twiddles, mmax, s, s, s, *pm)
        return rfft_raw(x, twiddles, mmax, s, s, s, kmajor)

    @staticmethod
    def backward(ctx, gxf):
        (tw,) = ctx.saved_tensors
        n, dt, kmajor, pm, scale = ctx.cfg
        if scale is None:
            s = (2.0 * math.pi / n, math.pi / n, 2.0 * math.pi / n)
        else:           # the adjoint of mk_rfft(s, s, s) is mk_irfft(s, s / 2, s)
            s = (float(scale), 0.5 * float(scale), float(scale))
        if pm:
            gx = irfft_pm_raw(gxf.contiguous(), tw, n, *s, *pm, dt)
        else:
            gx = irfft_raw(gxf.contiguous(), tw, n, *s, dt, kmajor)
        return gx, None, None, None, None, None


class _IRFFT(torch.autograd.Function):
    """Fourier rows (layouts as for ``_RFFT``) -> x [BC, K, nlon] = irfft(xf, n=nlon, norm="forward") (K4), times ``scale``
    where one is given (the planar transform passes 1 / sqrt(nlon))."""

    @staticmethod
    def forward(ctx, xf, twiddles, nlon, out_dtype, kmajor=False, want_sums=False, pm=None, scale=None, exact_sums=False):
        ctx.save_for_backward(twiddles)
        chans, cpp = pm or (0, 0)
        s = 1.0 if scale is None else float(scale)
        ctx.cfg = (_xf_dims(xf, kmajor, chans, cpp)[0], kmajor, pm, s)
        if want_sums:            # (x, row statistics): the sums are data for the norm's kernel, not a differentiable output
            x, sums = irfft_sums_raw(xf, twiddles, nlon, out_dtype, kmajor, chans, cpp, scale=s, exact=bool(exact_sums))
            ctx.mark_non_differentiable(sums)
            return x, sums
        if pm:
            return irfft_pm_raw(xf, twiddles, nlon, s, s, s, chans, cpp, out_dtype)
        return irfft_raw(xf, twiddles, nlon, s, s, s, out_dtype, kmajor)

    @staticmethod
    def backward(ctx, gx, *_):
        (tw,) = ctx.saved_tensors
        mmax, kmajor, pm, s = ctx.cfg         # the adjoint of mk_irfft(s, s, s) is mk_rfft(s, 2 s, s)
        gx = _lowp(gx)
        if pm:
            gxf = rfft_pm_raw(gx.contiguous(), tw, mmax, s, 2.0 * s, s, *pm)
        else:
            gxf = rfft_raw(gx.contiguous(), tw, mmax, s, 2.0 * s, s, kmajor)
        return gxf, None, None, None, None, None, None, None, None


class _LegendreFwd(torch.autograd.Function):
    """xf [Mloc, K, BC] -> c [L, Mloc, BC] with table[m_off + m] (K2)."""

    @staticmethod
    def forward(ctx, xf, table, lmax, m_off, kmajor=False):
        ctx.table = table   # constant buffer; the python object carries the cached bf16x3 images
        ctx.nlat, ctx.m_off, ctx.kmajor = xf.shape[0] if kmajor else xf.shape[1], m_off, kmajor
        return legendre_fwd_raw(xf, table, lmax, m_off, kmajor=kmajor)

    @staticmethod
    def backward(ctx, gc):
        return legendre_inv_raw(gc.contiguous(), ctx.table, ctx.nlat, ctx.m_off, kmajor=ctx.kmajor), None, None, None, None


class _LegendreInv(torch.autograd.Function):
    """c [L, Mloc, BC] -> xf [Mloc, K, BC] with table[m_off + m] (K3)."""

    @staticmethod
    def forward(ctx, c, table, nlat, m_off, kmajor=False):
        ctx.table = table
        ctx.lmax, ctx.m_off, ctx.kmajor = c.shape[0], m_off, kmajor
        return legendre_inv_raw(c, table, nlat, m_off, kmajor=kmajor)

    @staticmethod
    def backward(ctx, gxf):
        return legendre_fwd_raw(gxf.contiguous(), ctx.table, ctx.lmax, ctx.m_off, kmajor=ctx.kmajor), None, None, None, None


class _LatDft(torch.autograd.Function):
    """xf [nlat, M, BC] -> c [lmax, M, BC]: the truncated latitude DFT of the planar transform; backward = ``mk_latdft_inv``."""

    @staticmethod
    def forward(ctx, xf, table, lmax):
        ctx.table, ctx.nlat = table, xf.shape[0]
        return lat_dft_raw(xf, table, lmax)

    @staticmethod
    def backward(ctx, gc):
        return lat_idft_raw(gc.contiguous(), ctx.table, ctx.nlat), None, None


class _LatIdft(torch.autograd.Function):
    """c [lmax, M, BC] -> xf [nlat, M, BC]: the adjoint of ``_LatDft`` (the zero-padded inverse DFT); backward = ``mk_latdft_fwd``."""

    @staticmethod
    def forward(ctx, c, table, nlat):
        ctx.table, ctx.lmax = table, c.shape[0]
        return lat_idft_raw(c, table, nlat)

    @staticmethod
    def backward(ctx, gxf):
        return lat_dft_raw(gxf.contiguous(), ctx.table, ctx.lmax), None, None


class _SpecPack(torch.autograd.Function):
    @staticmethod
    def forward(ctx, c_std, l_off, m_off):
        ctx.offs = (l_off, m_off)
        return spec_pack_raw(c_std)

    @staticmethod
    def backward(ctx, g):
        return spec_unpack_raw(g.contiguous(), *ctx.offs), None, None


class _SpecUnpack(torch.autograd.Function):
    @staticmethod
    def forward(ctx, c_prv, l_off, m_off):
        return spec_unpack_raw(c_prv, l_off, m_off)

    @staticmethod
    def backward(ctx, g):
        return spec_pack_raw(g.contiguous()), None, None


class _Dhconv(torch.autograd.Function):
    """y[l, m, b, o] = sum_i x[l, m, b, i] w[i, o, l] on the private layout (K5)."""

    @staticmethod
    def forward(ctx, x, w, batch, l_off, m_off):
        wp = _w_phys(w)
        ctx.save_for_backward(x, wp)
        ctx.args = (batch, l_off, m_off)
        return dhconv_fwd_raw(x, wp, batch, l_off, m_off)

    @staticmethod
    def backward(ctx, gy):
        x, wp = ctx.saved_tensors
        batch, l_off, m_off = ctx.args
        gy = gy.contiguous()
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = dhconv_dgrad_raw(gy, wp, batch, l_off, m_off)
        if ctx.needs_input_grad[1]:
            # physical [L, I, O] -> logical [I, O, L] view with the parameter's own strides
            gw = dhconv_wgrad_raw(x, gy, batch, l_off, m_off).permute(1, 2, 0)
        return gx, gw, None, None, None


def spec_mix_supported(cin, cout):
    """The spectral channel mix runs on the bf16x3 engine only (even channel counts); ``MK_SPEC_MIX=0`` switches its call
    sites back to the convolutions on the grid."""
    return (_knob("MK_SPEC_MIX", "1") != "0" and _gemm_mode(None) == "bf16x3" and cin % 2 == 0 and cout % 2 == 0)


def _spec_mix_args(x, batch):
    _need_cuda(x)
    assert x.dim() == 3 and x.is_contiguous() and x.dtype == torch.complex64 and x.shape[2] % batch == 0
    return x.shape[0], x.shape[1], x.shape[2] // batch


def spec_mix_fwd_raw(x, w, batch, l_off=0, m_off=0):
    """y[l, m, b, o] = sum_i w[o, i] x[l, m, b, i] on the private spectrum ``[L, M, B * I]``; ``w`` fp32 ``[O, I]``."""
    lloc, mloc, cin = _spec_mix_args(x, batch)
    assert w.dtype == torch.float32 and w.is_contiguous() and w.dim() == 2 and w.shape[1] == cin
    cout = w.shape[0]
    y = torch.empty(lloc, mloc, batch * cout, dtype=torch.complex64, device=x.device)
    _lib.check(_lib.load().mk_spec_mix_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), lloc, mloc, batch, cin, cout, l_off, m_off,
                                           _stream()), "mk_spec_mix_fwd")
    return y


def spec_mix_dgrad_raw(gy, w, batch, l_off=0, m_off=0):
    """gx[l, m, b, i] = sum_o w[o, i] gy[l, m, b, o]."""
    lloc, mloc, cout = _spec_mix_args(gy, batch)
    assert w.dtype == torch.float32 and w.is_contiguous() and w.dim() == 2 and w.shape[0] == cout
    cin = w.shape[1]
    gx = torch.empty(lloc, mloc, batch * cin, dtype=torch.complex64, device=gy.device)
    _lib.check(_lib.load().mk_spec_mix_dgrad(gy.data_ptr(), w.data_ptr(), gx.data_ptr(), lloc, mloc, batch, cin, cout, l_off,
                                             m_off, _stream()), "mk_spec_mix_dgrad")
    return gx


def spec_mix_wgrad_raw(x, gy, batch, l_off=0, m_off=0):
    """gw[o, i] = sum over the valid (l, m, b) of re(gy[l, m, b, o] conj(x[l, m, b, i])) -> fp32 ``[O, I]``."""
    lloc, mloc, cin = _spec_mix_args(x, batch)
    l2, m2, cout = _spec_mix_args(gy, batch)
    assert (l2, m2) == (lloc, mloc)
    gw = torch.zeros(cout, cin, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().mk_spec_mix_wgrad(x.data_ptr(), gy.data_ptr(), gw.data_ptr(), lloc, mloc, batch, cin, cout, l_off,
                                             m_off, _stream()), "mk_spec_mix_wgrad")
    return gw


class _SpecMix(torch.autograd.Function):
    """A bias-free 1x1 convolution moved across a spherical harmonic transform: the real ``[O, I]`` weight mixes the
    channels of every coefficient of the private spectrum (``mk_spec_mix_*``).  Saves the input spectrum and the weight."""

    @staticmethod
    def forward(ctx, x, w, batch, l_off, m_off):
        wf = w.detach().float().contiguous()
        ctx.save_for_backward(x, wf)
        ctx.args = (batch, l_off, m_off, w.dtype, tuple(w.shape))
        return spec_mix_fwd_raw(x, wf.view(wf.shape[0], -1), batch, l_off, m_off)

    @staticmethod
    def backward(ctx, gy):
        x, wf = ctx.saved_tensors
        batch, l_off, m_off, wdt, wshape = ctx.args
        gy = gy.contiguous()
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = spec_mix_dgrad_raw(gy, wf.view(wf.shape[0], -1), batch, l_off, m_off)
        if ctx.needs_input_grad[1]:
            gw = spec_mix_wgrad_raw(x, gy, batch, l_off, m_off).view(wshape).to(wdt)
        return gx, gw, None, None, None


def spec_mix(x, w, batch, l_off=0, m_off=0):
    """``w``: the convolution's weight, ``[O, I]`` or ``[O, I, 1, 1]`` (the fp32 master, used as it is)."""
    return _SpecMix.apply(x, w, batch, l_off, m_off)


# ----------------------------------------------------------------------------
# complex channel MLP on the private spectrum (the non-linear filter, mk_spec_cmlp_*)
# ----------------------------------------------------------------------------
# The fused path is the default by the rule of DESIGN section 19: no row of tools/specattn_bench.py is slower than the torch
# formulation.
SPEC_ATTN_DEFAULT = "hip"
CMLP_ACT = {None: 0, "none": 0, "real": 1, "cartesian": 2}


def spec_attn_hip():
    """``MK_SPEC_ATTN=hip|torch`` (read at call time): the channel MLP of ``SpectralAttention`` on the ``mk_spec_cmlp_*`` kernels,
    or the torch einsums on the public spectrum."""
    return _hip_or_torch("MK_SPEC_ATTN", SPEC_ATTN_DEFAULT)


def _cmlp_weight(w, lloc):
    assert w.dtype == torch.complex64 and w.is_contiguous() and w.dim() in (2, 3), "complex64 [I, O] or [L, I, O] weight"
    assert w.dim() == 2 or w.shape[0] == lloc, "a per-degree weight needs one panel per local degree"
    return int(w.dim() == 3), w.shape[-2], w.shape[-1]


def _cmlp_out(out, shape, like):
    if out is None:
        return torch.empty(shape, dtype=torch.complex64, device=like.device)
    assert tuple(out.shape) == tuple(shape) and out.dtype == torch.complex64 and out.is_contiguous() and out.device == like.device
    return out


def spec_cmlp_fwd_raw(x, w, bias, batch, act=0, l_off=0, m_off=0, out=None):
    """y[l, m, b, o] = act(sum_i x[l, m, b, i] w[(l,) i, o] + bias[o]) on the private spectrum ``[L, M, B * I]``; ``w`` complex64
    ``[I, O]`` (all degrees) or ``[L, I, O]`` (per degree), ``bias`` complex64 with O elements or None, ``act`` 0 | 1 | 2
    (none | ``real`` | ``cartesian``).  ``out``: the result's buffer (its entries with l < m stay as they are)."""
    lloc, mloc, cin = _spec_mix_args(x, batch)
    _need_cuda(w)
    per_degree, wi, cout = _cmlp_weight(w, lloc)
    assert wi == cin, "channel MLP operand shapes do not match"
    bp = 0
    if bias is not None:
        _need_cuda(bias)
        assert bias.dtype == torch.complex64 and bias.is_contiguous() and bias.numel() == cout
        bp = bias.data_ptr()
    y = _cmlp_out(out, (lloc, mloc, batch * cout), x)
    _lib.check(_lib.load().mk_spec_cmlp_fwd(x.data_ptr(), w.data_ptr(), bp, y.data_ptr(), lloc, mloc, batch, cin, cout, l_off, m_off,
                                            per_degree, int(act), _stream()), "mk_spec_cmlp_fwd")
    return y


def spec_cmlp_dgrad_raw(gy, w, a, batch, act=0, l_off=0, m_off=0, out=None):
    """gx = (gy conj(w)^T) * relu'(a): ``a`` the saved activation output ``[L, M, B * I]`` of the layer in front (mode ``act``), or
    None for no mask."""
    lloc, mloc, cout = _spec_mix_args(gy, batch)
    _need_cuda(w)
    per_degree, cin, wo = _cmlp_weight(w, lloc)
    assert wo == cout, "channel MLP operand shapes do not match"
    ap = 0
    if a is not None:
        assert _spec_mix_args(a, batch) == (lloc, mloc, cin)
        ap = a.data_ptr()
    gx = _cmlp_out(out, (lloc, mloc, batch * cin), gy)
    _lib.check(_lib.load().mk_spec_cmlp_dgrad(gy.data_ptr(), w.data_ptr(), ap, gx.data_ptr(), lloc, mloc, batch, cin, cout, l_off,
                                              m_off, per_degree, int(act) if a is not None else 0, _stream()), "mk_spec_cmlp_dgrad")
    return gx


def spec_cmlp_wgrad_raw(x, gy, batch, per_degree, l_off=0, m_off=0):
    """gw[(l,) i, o] = sum over the valid (m, b) (and, without ``per_degree``, l) of conj(x[l, m, b, i]) gy[l, m, b, o]."""
    lloc, mloc, cin = _spec_mix_args(x, batch)
    l2, m2, cout = _spec_mix_args(gy, batch)
    assert (l2, m2) == (lloc, mloc)
    lib = _lib.load()
    gw = torch.empty((lloc, cin, cout) if per_degree else (cin, cout), dtype=torch.complex64, device=x.device)
    nbytes = lib.mk_spec_cmlp_wgrad_workspace(lloc, cin, cout, int(bool(per_degree)))
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device) if nbytes else None
    _lib.check(lib.mk_spec_cmlp_wgrad(x.data_ptr(), gy.data_ptr(), gw.data_ptr(), ws.data_ptr() if nbytes else 0, lloc, mloc, batch,
                                      cin, cout, l_off, m_off, int(bool(per_degree)), _stream()), "mk_spec_cmlp_wgrad")
    return gw


def spec_cmlp_bgrad_raw(g, batch, l_off=0, m_off=0):
    """gb[o] = sum over the valid (l, m, b) of g[l, m, b, o] -> complex64 ``[O]`` (float64 sums in a fixed order)."""
    lloc, mloc, cout = _spec_mix_args(g, batch)
    lib = _lib.load()
    gb = torch.empty(cout, dtype=torch.complex64, device=g.device)
    ws = torch.empty(lib.mk_spec_cmlp_bgrad_workspace(lloc, cout) // 8, dtype=torch.float64, device=g.device)
    _lib.check(lib.mk_spec_cmlp_bgrad(g.data_ptr(), gb.data_ptr(), ws.data_ptr(), lloc, mloc, batch, cout, l_off, m_off, _stream()),
               "mk_spec_cmlp_bgrad")
    return gb


class _SpecChannelMLP(torch.autograd.Function):
    """The channel MLP of the non-linear filter on the private spectrum: ``n`` activated products, then ``wout``.  Saves the input
    spectrum and every layer's activation output (the next product's input and, by its signs, relu' of its own layer)."""

    @staticmethod
    def forward(ctx, c, batch, act, per_degree, l_off, m_off, n, has_bias, *params):
        weights, biases, wout = params[:n], params[n:2 * n] if has_bias else (None,) * n, params[-1]
        fields = [c]
        for w, b in zip(weights, biases):
            fields.append(spec_cmlp_fwd_raw(fields[-1], w.detach(), None if b is None else b.detach().reshape(-1), batch, act,
                                            l_off, m_off))
        y = spec_cmlp_fwd_raw(fields[-1], wout.detach(), None, batch, 0, l_off, m_off)
        ctx.save_for_backward(*fields, *weights, wout)
        ctx.args = (batch, act, per_degree, l_off, m_off, n, has_bias, [None if b is None else b.shape for b in biases])
        return y

    @staticmethod
    def backward(ctx, gy):
        batch, act, per_degree, l_off, m_off, n, has_bias, bshapes = ctx.args
        fields, ws = ctx.saved_tensors[:n + 1], ctx.saved_tensors[n + 1:]
        need = ctx.needs_input_grad
        g = gy.contiguous()
        gws, gbs = [None] * (n + 1), [None] * n
        for k in range(n, -1, -1):      # layer k reads fields[k]; k == n is wout
            if need[8 + k if k < n else len(need) - 1]:
                gws[k] = spec_cmlp_wgrad_raw(fields[k], g, batch, per_degree, l_off, m_off)
            if k < n and has_bias and need[8 + n + k]:
                gbs[k] = spec_cmlp_bgrad_raw(g, batch, l_off, m_off).view(bshapes[k])
            if k > 0:
                g = spec_cmlp_dgrad_raw(g, ws[k], fields[k] if act else None, batch, act, l_off, m_off)     # act 0: no mask
            elif need[0]:
                g = spec_cmlp_dgrad_raw(g, ws[0], None, batch, 0, l_off, m_off)
            else:
                g = None
        return (g, None, None, None, None, None, None, None, *gws[:n], *(gbs if has_bias else ()), gws[n])


def spec_channel_mlp(c, weights, biases, wout, batch, act, per_degree, l_off=0, m_off=0):
    """``SpectralAttention.forward_mlp`` on the private spectrum ``c`` ``[L, M, B * C]``: for every layer
    ``c = ComplexReLU(c w + b)``, then ``c wout``.  ``weights`` / ``wout``: complex64 ``[I, O]`` (``per_degree`` False) or
    ``[L, I, O]``; ``biases``: one complex64 tensor of O elements per layer, or None; ``act``: ``"real"`` | ``"cartesian"`` (or
    None: plain products, no mask in the backward).
    Gradients come back in every parameter's own shape."""
    weights = list(weights)
    biases = list(biases) if biases is not None else []
    assert not biases or len(biases) == len(weights)
    return _SpecChannelMLP.apply(c, batch, CMLP_ACT[act], bool(per_degree), l_off, m_off, len(weights), bool(biases),
                                 *weights, *biases, wout)


# ----------------------------------------------------------------------------
# block-diagonal complex MLP on the dense planar spectrum (AFNO2D, mk_spec_bdmlp_*)
# ----------------------------------------------------------------------------
# The fused path is the default by the rule of DESIGN section 19: no row of tools/afno_bench.py is slower than the torch
# formulation.  It still needs the HIP planar transforms (MK_PLANAR_FFT=hip).
AFNO_DEFAULT = "hip"


def afno_hip():
    """``MK_AFNO=hip|torch`` (read at call time): ``AFNO2D`` on the HIP planar transforms with the ``mk_spec_bdmlp_*`` block MLP
    in between, or the reference's formulation in torch ops."""
    return _hip_or_torch("MK_AFNO", AFNO_DEFAULT)


def _bdmlp_args(x, w, cols):
    """``x``: contiguous complex64 field whose last axis is a whole number of ``nb * cols`` channel groups; ``w``: complex64
    ``[nb, ib, ob]``; ``cols``: which of the panel's axes the field's channels are (1: ib, 2: ob).  -> rows, nb, ib, ob."""
    _need_cuda(x, w)
    assert x.dtype == torch.complex64 and x.is_contiguous() and x.dim() >= 1, "contiguous complex64 field"
    assert w.dtype == torch.complex64 and w.is_contiguous() and w.dim() == 3, "contiguous complex64 [nb, ib, ob] weight"
    nb, ib, ob = w.shape
    chans = nb * w.shape[cols]
    assert x.shape[-1] % chans == 0, "block MLP operand shapes do not match"
    return x.numel() // chans, nb, ib, ob


def _bdmlp_out(out, x, chans_in, chans_out):
    shape = tuple(x.shape[:-1]) + (x.shape[-1] // chans_in * chans_out,)
    if out is None:
        return torch.empty(shape, dtype=torch.complex64, device=x.device)
    assert tuple(out.shape) == shape and out.dtype == torch.complex64 and out.is_contiguous() and out.device == x.device
    return out


def spec_bdmlp_mask_raw(gy, s, out=None):
    """``gy`` where the same component (real / imaginary) of ``s`` is non-zero, else 0: the gradient through a soft-shrink whose
    saved output is ``s``.  ``out`` may be ``gy`` itself."""
    _need_cuda(gy, s)
    assert gy.dtype == s.dtype == torch.complex64 and gy.is_contiguous() and s.is_contiguous() and gy.shape == s.shape
    out = torch.empty_like(gy) if out is None else out
    assert out.dtype == torch.complex64 and out.is_contiguous() and out.shape == gy.shape and out.device == gy.device
    _lib.check(_lib.load().mk_spec_bdmlp_mask(gy.data_ptr(), s.data_ptr(), out.data_ptr(), 2 * gy.numel(), _stream()),
               "mk_spec_bdmlp_mask")
    return out


def spec_bdmlp_fwd_raw(x, w, act=0, lam=0.0, out=None, bias=None):
    """y[r, k * ob + o] = act(sum_i x[r, k * ib + i] w[k, i, o] + bias[k * ob + o]) on the rows of the dense spectrum
    ``[L, M, B * nb * ib]``; ``w`` complex64 ``[nb, ib, ob]``; ``bias`` complex64 of ``nb * ob`` elements or None (then
    ``mk_spec_bdmlp_fwd``, as ever); ``act`` 0 | 2 | 3 (none | ReLU on both components | soft-shrink with threshold ``lam`` on
    both)."""
    rows, nb, ib, ob = _bdmlp_args(x, w, 1)
    y = _bdmlp_out(out, x, nb * ib, nb * ob)
    if bias is None:
        _lib.check(_lib.load().mk_spec_bdmlp_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), rows, nb, ib, ob, int(act), float(lam),
                                                 _stream()), "mk_spec_bdmlp_fwd")
        return y
    _need_cuda(bias)
    assert bias.dtype == torch.complex64 and bias.is_contiguous() and bias.numel() == nb * ob, "contiguous complex64 bias of nb * ob"
    _lib.check(_lib.load().mk_spec_bdmlp_fwd_bias(x.data_ptr(), w.data_ptr(), bias.data_ptr(), y.data_ptr(), rows, nb, ib, ob, int(act),
                                                  float(lam), _stream()), "mk_spec_bdmlp_fwd_bias")
    return y


def spec_bdmlp_dgrad_raw(gy, w, a=None, s=None, out=None):
    """gx = (gy' conj(w)^T) * relu'(a): ``a`` the saved ReLU output ``[L, M, B * nb * ib]`` of the layer in front or None; ``s``
    the saved soft-shrink output of this layer or None -- with it gy' is ``spec_bdmlp_mask_raw(gy, s)`` (one more pass)."""
    rows, nb, ib, ob = _bdmlp_args(gy, w, 2)
    if s is not None:
        gy = spec_bdmlp_mask_raw(gy, s)
    ap = 0
    if a is not None:
        assert _bdmlp_args(a, w, 1) == (rows, nb, ib, ob)
        ap = a.data_ptr()
    gx = _bdmlp_out(out, gy, nb * ob, nb * ib)
    _lib.check(_lib.load().mk_spec_bdmlp_dgrad(gy.data_ptr(), w.data_ptr(), ap, gx.data_ptr(), rows, nb, ib, ob, 2 if ap else 0,
                                               _stream()), "mk_spec_bdmlp_dgrad")
    return gx


def spec_bdmlp_wgrad_raw(x, gy, batch, num_blocks, s=None):
    """gw[k, i, o] = sum_r conj(x[r, k * ib + i]) gy'[r, k * ob + o] -> complex64 ``[nb, ib, ob]`` for fields ``[L, M, B * nb * ib]``
    and ``[L, M, B * nb * ob]``; ``s`` as for the data gradient.  Partial panels are added in a fixed order: the same bits on
    every run."""
    _need_cuda(x, gy)
    assert x.dtype == gy.dtype == torch.complex64 and x.is_contiguous() and gy.is_contiguous() and x.shape[:-1] == gy.shape[:-1]
    nb, per = int(num_blocks), int(batch) * int(num_blocks)
    assert x.shape[-1] % per == 0 and gy.shape[-1] % per == 0, "block MLP operand shapes do not match"
    ib, ob = x.shape[-1] // per, gy.shape[-1] // per
    rows = x.numel() // (nb * ib)
    if s is not None:
        gy = spec_bdmlp_mask_raw(gy, s)
    lib = _lib.load()
    gw = torch.empty((nb, ib, ob), dtype=torch.complex64, device=x.device)
    nbytes = lib.mk_spec_bdmlp_wgrad_workspace(rows, nb, ib, ob)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device) if nbytes else None
    _lib.check(lib.mk_spec_bdmlp_wgrad(x.data_ptr(), gy.data_ptr(), gw.data_ptr(), ws.data_ptr() if nbytes else 0, rows, nb, ib, ob,
                                       _stream()), "mk_spec_bdmlp_wgrad")
    return gw


def _block_weight(w):
    """The reference's real ``[nb, ib, ob, 2]`` parameter as the kernels' complex64 ``[nb, ib, ob]``, taken as it is."""
    assert w.dim() == 4 and w.shape[-1] == 2 and w.dtype == torch.float32, "fp32 [nb, ib, ob, 2] block weight"
    return torch.view_as_complex(w.detach().contiguous())


def _block_bias(b):
    """A real ``[n, 2]`` (re, im) bias as the kernels' contiguous complex64 ``[n]``, or None."""
    if b is None:
        return None
    assert b.dim() == 2 and b.shape[1] == 2 and b.dtype == torch.float32, "fp32 [nb * ob, 2] block bias"
    return torch.view_as_complex(b.detach().contiguous())


def _block_bias_grad(g, batch):
    """Sum of the dense ``[L, M, B * n]`` gradient over all rows and samples -> real ``[n, 2]``: ``mk_spec_cmlp_bgrad`` with the
    degree offset at ``M`` (no triangle), float64 sums in a fixed order."""
    return torch.view_as_real(spec_cmlp_bgrad_raw(g, batch, g.shape[1], 0))


class _SpecBlockMLP(torch.autograd.Function):
    """``softshrink(relu_c(c w1) w2)`` per channel block on the dense spectrum.  Saves the input spectrum, the hidden activation
    (the second product's input and, by its signs, relu') and the output (by its zeros, softshrink')."""

    @staticmethod
    def forward(ctx, c, w1, w2, batch, nb, lam, b1, b2):
        h = spec_bdmlp_fwd_raw(c, _block_weight(w1), 2, bias=_block_bias(b1))
        y = spec_bdmlp_fwd_raw(h, _block_weight(w2), 3, lam, bias=_block_bias(b2))
        ctx.save_for_backward(c, h, y, w1, w2)
        ctx.args = (batch, nb)
        return y

    @staticmethod
    def backward(ctx, gy):
        batch, nb = ctx.args
        c, h, y, w1, w2 = ctx.saved_tensors
        need = ctx.needs_input_grad
        g = spec_bdmlp_mask_raw(gy.contiguous(), y)         # one masked copy serves both gradients of the second layer
        gw2 = torch.view_as_real(spec_bdmlp_wgrad_raw(h, g, batch, nb)) if need[2] else None
        need_b1, need_b2 = need[6], need[7]
        gb2 = _block_bias_grad(g, batch) if need_b2 else None
        gc = gw1 = gb1 = None
        if need[0] or need[1] or need_b1:
            gh = spec_bdmlp_dgrad_raw(g, _block_weight(w2), a=h)
            if need[1]:
                gw1 = torch.view_as_real(spec_bdmlp_wgrad_raw(c, gh, batch, nb))
            if need_b1:
                gb1 = _block_bias_grad(gh, batch)
            if need[0]:
                gc = spec_bdmlp_dgrad_raw(gh, _block_weight(w1))
        return gc, gw1, gw2, None, None, None, gb1, gb2


def _spec_block_mlp_torch(c, w1, w2, batch, nb, lam, b1=None, b2=None):
    """The same function in torch ops (CPU tensors)."""
    L, M = c.shape[0], c.shape[1]
    x = c.reshape(L, M, batch, nb, -1)
    h = torch.einsum("lmbki,kio->lmbko", x, torch.view_as_complex(w1.contiguous()))
    if b1 is not None:
        h = h + torch.view_as_complex(b1.contiguous()).view(nb, -1)
    h = torch.complex(torch.relu(h.real), torch.relu(h.imag))
    y = torch.einsum("lmbki,kio->lmbko", h, torch.view_as_complex(w2.contiguous()))
    if b2 is not None:
        y = y + torch.view_as_complex(b2.contiguous()).view(nb, -1)
    y = torch.view_as_complex(torch.nn.functional.softshrink(torch.view_as_real(y), lambd=lam))
    return y.reshape(L, M, -1)


def spec_block_mlp(c, w1, w2, batch, num_blocks, lam, b1=None, b2=None):
    """AFNO's filter arithmetic on the dense private spectrum ``c`` ``[L, M, B * C]`` (complex64): per channel block k of
    ``C / num_blocks`` channels ``softshrink(relu_c(c_k w1[k] + b1[k]) w2[k] + b2[k], lam)``, ReLU and soft-shrink on both
    components.  ``w1`` ``[nb, bs, hb, 2]``, ``w2`` ``[nb, hb, bs, 2]``: the reference's real fp32 parameters of afnonet_v2.py; their
    gradients come back in that shape.  ``b1`` ``[nb * hb, 2]``, ``b2`` ``[nb * bs, 2]``: real fp32 (re, im) pairs per hidden / output
    channel (the channels-last AFNO's complex biases), or None -- without them the calls and the bits are what they were.  The
    bias gradients are float64 sums in a fixed order (``mk_spec_cmlp_bgrad``).
    CUDA tensors run on the ``mk_spec_bdmlp_*`` kernels (even ``bs`` and ``hb``), CPU tensors on torch ops."""
    nb = int(num_blocks)
    assert c.dim() == 3 and c.shape[2] % (batch * nb) == 0 and w1.dim() == 4 and w2.dim() == 4
    bs = c.shape[2] // (batch * nb)
    assert w1.shape[0] == w2.shape[0] == nb and w1.shape[1] == w2.shape[2] == bs and w1.shape[2] == w2.shape[1], "block weight shapes"
    assert b1 is None or tuple(b1.shape) == (nb * w1.shape[2], 2), "b1: [nb * hb, 2]"
    assert b2 is None or tuple(b2.shape) == (nb * bs, 2), "b2: [nb * bs, 2]"
    if not c.is_cuda:
        return _spec_block_mlp_torch(c, w1, w2, batch, nb, lam, b1, b2)
    return _SpecBlockMLP.apply(c.contiguous(), w1, w2, int(batch), nb, float(lam), b1, b2)


# ----------------------------------------------------------------------------
# tokens [B, N, C] <-> fields [B, C, N] (the channels-last AFNO on the planar transforms, mk_tokens_to_fields / mk_fields_to_tokens)
# ----------------------------------------------------------------------------
# The fused path is the default by the rule of DESIGN section 19: no row of tools/afnov1_bench.py is slower than the torch
# formulation.  It still needs the HIP planar transforms (MK_PLANAR_FFT=hip).
AFNOV1_DEFAULT = "hip"


def afnov1_hip():
    """``MK_AFNOV1=hip|torch`` (read at call time): the channels-last ``AFNO2D`` of ``afnonet_v1`` on the layout passes, the HIP
    planar transforms and the block MLP with biases, or the reference's formulation in torch ops."""
    return _hip_or_torch("MK_AFNOV1", AFNOV1_DEFAULT)


def _layout_args(x, other=None):
    assert x.dim() == 3 and x.numel() > 0 and x.dtype in _LOWP, "[B, N, C] / [B, C, N] fp32 or bf16"
    assert other is None or (other.dtype == x.dtype and other.device == x.device)


def tokens_to_fields_raw(x, out=None):
    """``x`` ``[B, N, C]`` contiguous -> ``[B, C, N]`` (``mk_tokens_to_fields``)."""
    _need_cuda(x)
    _layout_args(x)
    assert x.is_contiguous()
    B, N, C = x.shape
    out = torch.empty((B, C, N), dtype=x.dtype, device=x.device) if out is None else out
    assert tuple(out.shape) == (B, C, N) and out.is_contiguous() and out.dtype == x.dtype and out.device == x.device
    _lib.check(_lib.load().mk_tokens_to_fields(x.data_ptr(), out.data_ptr(), _pw_dtype(x), B, N, C, _stream()), "mk_tokens_to_fields")
    return out


def fields_to_tokens_raw(r, addend=None, out=None):
    """``r`` ``[B, C, N]`` contiguous (+ ``addend`` ``[B, N, C]`` contiguous) -> ``[B, N, C]`` (``mk_fields_to_tokens``)."""
    _need_cuda(r)
    _layout_args(r, addend)
    assert r.is_contiguous()
    B, C, N = r.shape
    assert addend is None or (tuple(addend.shape) == (B, N, C) and addend.is_contiguous())
    out = torch.empty((B, N, C), dtype=r.dtype, device=r.device) if out is None else out
    assert tuple(out.shape) == (B, N, C) and out.is_contiguous() and out.dtype == r.dtype and out.device == r.device
    _lib.check(_lib.load().mk_fields_to_tokens(r.data_ptr(), _ptr(addend), out.data_ptr(),
                                               _pw_dtype(r), B, N, C, _stream()), "mk_fields_to_tokens")
    return out


class _TokensToFields(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return tokens_to_fields_raw(x.contiguous())

    @staticmethod
    def backward(ctx, g):
        return fields_to_tokens_raw(g.contiguous())


class _FieldsToTokens(torch.autograd.Function):
    @staticmethod
    def forward(ctx, r, addend):
        return fields_to_tokens_raw(r.contiguous(), None if addend is None else addend.contiguous())

    @staticmethod
    def backward(ctx, g):
        need = ctx.needs_input_grad
        return tokens_to_fields_raw(g.contiguous()) if need[0] else None, g if need[1] else None


def tokens_to_fields(x):
    """``[B, N, C]`` tokens -> ``[B, C, N]`` fields (fp32 / bf16): one ``mk_tokens_to_fields`` pass on the device, its backward one
    ``mk_fields_to_tokens`` pass; CPU tensors take ``x.transpose(1, 2).contiguous()``."""
    _layout_args(x)
    if not x.is_cuda:
        return x.transpose(1, 2).contiguous()
    return _TokensToFields.apply(x)


def fields_to_tokens(r, addend=None):
    """``[B, C, N]`` fields -> ``[B, N, C]`` tokens, ``+ addend`` (``[B, N, C]``, same dtype; the add in fp32, rounded once) in the
    same pass.  The backward is one ``mk_tokens_to_fields`` pass; the addend's gradient is the incoming gradient.  CPU tensors take
    ``r.transpose(1, 2) + addend``."""
    _layout_args(r, addend)
    if not r.is_cuda:
        t = r.transpose(1, 2)
        return (t if addend is None else t + addend).contiguous()
    return _FieldsToTokens.apply(r, addend)


def rfft(x, twiddles, mmax, kmajor=False, scale=None):
    """``scale``: the factor on every mode; None = the SHT's 2 pi / nlon."""
    return _RFFT.apply(x, twiddles, mmax, kmajor, None, scale)


def irfft(xf, twiddles, nlon, out_dtype=torch.float32, kmajor=False, want_sums=False, scale=None, exact_sums=False):
    """``want_sums``: returns (x, fp64 ``[BC, 2]`` row sums / sums of squares of x) -- see ``mk_irfft_sums``; ``exact_sums``: through
    ``mk_irfft_sums_ws`` (float64 from the first add, fixed order; one more launch).
    ``scale``: the factor on every mode; None = 1 (``norm="forward"``)."""
    return _IRFFT.apply(xf, twiddles, nlon, out_dtype, kmajor, want_sums, None, scale, exact_sums)


def lat_dft(xf, table, lmax):
    return _LatDft.apply(xf, table, lmax)


def lat_idft(c, table, nlat):
    return _LatIdft.apply(c, table, nlat)


def rfft_pm(x, twiddles, mmax, chans, cpp):
    return _RFFT.apply(x, twiddles, mmax, True, (chans, cpp))


def irfft_pm(xf, twiddles, nlon, out_dtype, chans, cpp, want_sums=False):
    return _IRFFT.apply(xf, twiddles, nlon, out_dtype, True, want_sums, (chans, cpp))


def legendre_fwd(xf, table, lmax, m_off=0, kmajor=False):
    return _LegendreFwd.apply(xf, table, lmax, m_off, kmajor)


def legendre_inv(c, table, nlat, m_off=0, kmajor=False):
    return _LegendreInv.apply(c, table, nlat, m_off, kmajor)


def spec_pack(c_std, l_off=0, m_off=0):
    return _SpecPack.apply(c_std, l_off, m_off)


def spec_unpack(c_prv, l_off=0, m_off=0):
    return _SpecUnpack.apply(c_prv, l_off, m_off)


def dhconv(x, w, batch, l_off=0, m_off=0):
    return _Dhconv.apply(x, w, batch, l_off, m_off)


# ----------------------------------------------------------------------------
# fused pointwise ops of the FNO block (bias + GELU, instance norm [+ GELU])
# ----------------------------------------------------------------------------
def _pw_dtype(t):
    if t.dtype in _DTYPE_CODE:
        return _DTYPE_CODE[t.dtype]
    raise TypeError(f"makani_amd pointwise ops: unsupported dtype {t.dtype}")


def pointwise_supported(x):
    """NCHW, contiguous, on the GPU, fp32/bf16, H*W a multiple of 8, B*C <= 65535."""
    return (x.is_cuda and x.dim() == 4 and x.is_contiguous() and x.dtype in _LOWP
            and (x.shape[2] * x.shape[3]) % 8 == 0 and x.shape[0] * x.shape[1] <= 65535)


class _BiasGelu(torch.autograd.Function):
    """y = gelu(x + bias[c]) on [B, C, H, W] (bias may be None)."""

    @staticmethod
    def forward(ctx, x, bias):
        _need_cuda(x)
        B, C, H, W = x.shape
        y = torch.empty_like(x)
        bf = None if bias is None else bias.detach().float().contiguous()
        _lib.check(_lib.load().mk_bias_gelu_fwd(x.data_ptr(), _ptr(bf), y.data_ptr(),
                                                _pw_dtype(x), B * C, C, H * W, _stream()), "mk_bias_gelu_fwd")
        ctx.save_for_backward(x, bf if bf is not None else x.new_empty(0))
        ctx.has_bias = bias is not None
        ctx.bias_dtype = None if bias is None else bias.dtype
        return y

    @staticmethod
    def backward(ctx, gy):
        x, bf = ctx.saved_tensors
        B, C, H, W = x.shape
        gy = gy.contiguous()
        gx = torch.empty_like(x)
        gb = torch.zeros(C, dtype=torch.float32, device=x.device) if ctx.has_bias else None
        _lib.check(_lib.load().mk_bias_gelu_bwd(x.data_ptr(), bf.data_ptr() if ctx.has_bias else 0, gy.data_ptr(),
                                                gx.data_ptr(), _ptr(gb), _pw_dtype(x),
                                                B * C, C, H * W, _stream()), "mk_bias_gelu_bwd")
        return gx, (gb.to(ctx.bias_dtype) if gb is not None else None)


class _InstanceNorm(torch.autograd.Function):
    """Affine instance norm over (H, W) with optional fused GELU; statistics in fp32/fp64.

    ``group`` / ``count``: the rows are sharded over the ranks of ``group`` (spatial model parallelism) -- the local
    row sums are all-reduced between the two kernel phases and ``count`` is the global number of elements per row.
    The weight / bias gradients returned are the LOCAL contributions (shared-weight reduction sums them later).
    """

    @staticmethod
    def forward(ctx, x, weight, bias, eps, fuse_gelu, group, count, sums=None):
        _need_cuda(x)
        B, C, H, W = x.shape
        y = torch.empty_like(x)
        wf = None if weight is None else weight.detach().float().contiguous()
        bf = None if bias is None else bias.detach().float().contiguous()
        stats = torch.empty(B * C, 2, dtype=torch.float32, device=x.device)
        if sums is not None:     # the producer of x delivered the local row sums (engine epilogue): statistics pass done
            assert sums.dtype == torch.float64 and sums.is_contiguous() and sums.numel() == 2 * B * C
        ws = sums if sums is not None else torch.empty(B * C, 2, dtype=torch.float64, device=x.device)
        lib = _lib.load()
        cnt = H * W if group is None else int(count)

        def run(phase):
            _lib.check(lib.mk_instnorm_fwd_ex(x.data_ptr(), _ptr(wf),
                                              _ptr(bf), y.data_ptr(), stats.data_ptr(),
                                              ws.data_ptr(), _pw_dtype(x), B * C, C, H * W, cnt, float(eps),
                                              int(fuse_gelu), phase, _stream()), "mk_instnorm_fwd_ex")
        if group is None:
            run(0 if sums is None else 2)
        else:
            if sums is None:
                run(1)
            torch.distributed.all_reduce(ws, group=group)
            run(2)
        empty = x.new_empty(0, dtype=torch.float32)
        ctx.save_for_backward(x, stats, wf if wf is not None else empty, bf if bf is not None else empty)
        ctx.cfg = (weight is not None, bias is not None, bool(fuse_gelu),
                   None if weight is None else weight.dtype, None if bias is None else bias.dtype, group, cnt)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, stats, wf, bf = ctx.saved_tensors
        has_w, has_b, fuse, wdt, bdt, group, cnt = ctx.cfg
        gx, gw, gb = instance_norm_backward(x, gy, stats, wf if has_w else None, bf if has_b else None, fuse, group, cnt,
                                            grad_dtype=wdt if (has_w and has_b and wdt == bdt) else None)
        return gx, gw.to(wdt) if has_w else None, gb.to(bdt) if has_b else None, None, None, None, None, None


def instance_norm_backward(x, gy, stats, wf, bf, fuse_gelu=False, group=None, count=None, grad_dtype=None):
    """Backward of the (optionally GELU-fused) instance norm from its saved ``stats`` [B * C, 2] = (mean, rstd):
    returns (gx, local weight-gradient sums [C], local bias-gradient sums [C]) -- the sums in fp64, or, with ``grad_dtype``,
    cast to it by ONE copy into a ``[2, C]`` buffer whose rows are the two (contiguous) results."""
    B, C, H, W = x.shape
    gy = gy.contiguous()
    gx = torch.empty_like(x)
    ws = torch.empty(B * C, 2, dtype=torch.float64, device=x.device)
    lib = _lib.load()
    cnt = H * W if group is None else int(count)

    def run(phase):
        _lib.check(lib.mk_instnorm_bwd_ex(x.data_ptr(), gy.data_ptr(), stats.data_ptr(), _ptr(wf), _ptr(bf),
                                          gx.data_ptr(), ws.data_ptr(), _pw_dtype(x), B * C, C, H * W, cnt, int(fuse_gelu),
                                          phase, _stream()), "mk_instnorm_bwd_ex")
    if group is None and B == 1 and grad_dtype == torch.float32 and wf is not None and bf is not None:
        # one sample: the kernel writes the affine parameters' gradients itself (no copy / cast launch behind it)
        out = torch.empty(2, C, dtype=torch.float32, device=x.device)
        _lib.check(lib.mk_instnorm_bwd_wb(x.data_ptr(), gy.data_ptr(), stats.data_ptr(), wf.data_ptr(), bf.data_ptr(),
                                          gx.data_ptr(), ws.data_ptr(), out.data_ptr(), _pw_dtype(x), C, H * W, int(fuse_gelu),
                                          _stream()), "mk_instnorm_bwd_wb")
        return gx, out[0], out[1]
    if group is None:
        run(0)
        local = ws
    else:
        run(1)
        local = ws.clone()
        torch.distributed.all_reduce(ws, group=group)
        run(2)
    sums = local.view(B, C, 2)
    sums = sums[0] if B == 1 else sums.sum(0)
    if grad_dtype is not None:
        out = torch.empty(2, C, dtype=grad_dtype, device=x.device)
        out.copy_(sums.t())
        return gx, out[1], out[0]
    return gx, sums[:, 1], sums[:, 0]


def instance_norm_coeffs(sums, weight, bias, rows, channels, count, eps):
    """Row sums fp64 [rows, 2] (global when sharded) -> (stats, affine), both fp32 [rows, 2]: (mean, rstd) and the affine
    map (a, b) with norm(x) = a * x + b (``mk_instnorm_coeffs``)."""
    _need_cuda(sums)
    assert sums.dtype == torch.float64 and sums.is_contiguous() and sums.numel() == 2 * rows
    stats = torch.empty(rows, 2, dtype=torch.float32, device=sums.device)
    affine = torch.empty(rows, 2, dtype=torch.float32, device=sums.device)
    _lib.check(_lib.load().mk_instnorm_coeffs(sums.data_ptr(), _ptr(weight),
                                              _ptr(bias), stats.data_ptr(), affine.data_ptr(),
                                              rows, channels, int(count), float(eps), _stream()), "mk_instnorm_coeffs")
    return stats, affine


class _WeightedMSE(torch.autograd.Function):
    """scale * sum wrow[h] (pred - tar)^2 over [B, C, H, W]; one streaming pass each way (mk_wmse_*)."""

    @staticmethod
    def forward(ctx, pred, tar, wrow, scale):
        _need_cuda(pred, tar, wrow)
        B, C, H, W = pred.shape
        loss = torch.empty(1, dtype=torch.float64, device=pred.device)
        _lib.check(_lib.load().mk_wmse_fwd(pred.data_ptr(), _pw_dtype(pred), tar.data_ptr(), wrow.data_ptr(), loss.data_ptr(),
                                           B * C * H, H, W, float(scale), _stream()), "mk_wmse_fwd")
        ctx.save_for_backward(pred, tar, wrow)
        ctx.scale = float(scale)
        return loss.float().squeeze(0)

    @staticmethod
    def backward(ctx, g):
        pred, tar, wrow = ctx.saved_tensors
        B, C, H, W = pred.shape
        gp = torch.empty_like(pred)
        g32 = g.detach().float().reshape(1).contiguous()
        _lib.check(_lib.load().mk_wmse_bwd(pred.data_ptr(), _pw_dtype(pred), tar.data_ptr(), wrow.data_ptr(), g32.data_ptr(),
                                           gp.data_ptr(), B * C * H, H, W, ctx.scale, _stream()), "mk_wmse_bwd")
        return gp, None, None, None


def weighted_mse(pred, tar, wrow, scale=1.0):
    """``scale * (((pred - tar) ** 2) * wrow[None, None, :, None]).sum()`` for pred [B, C, H, W] (fp32 / bf16, contiguous),
    tar fp32 of the same shape, wrow fp32 [H]; gradient w.r.t. pred only."""
    if not (pred.is_cuda and pred.is_contiguous() and tar.is_contiguous() and tar.dtype == torch.float32
            and pred.dtype in _LOWP and pred.shape[-1] % 8 == 0):
        w = wrow.view(1, 1, -1, 1)
        return scale * (((pred.float() - tar) ** 2) * w).sum()
    return _WeightedMSE.apply(pred, tar, wrow.float().contiguous(), scale)


def row_sums(t3):
    """Sum over the last axis of a contiguous [B, C, P] fp32 / bf16 field -> fp32 [B * C] (mk_instnorm_fwd_ex, phase 1)."""
    _need_cuda(t3)
    assert t3.dim() == 3 and t3.is_contiguous()
    b, c, p = t3.shape
    if not _hip_or_torch("MK_ROWSUM", "hip"):
        return torch.sum(t3, dim=-1, dtype=torch.float32).view(-1)
    ws = torch.empty(b * c, 2, dtype=torch.float64, device=t3.device)
    _lib.check(_lib.load().mk_instnorm_fwd_ex(t3.data_ptr(), 0, 0, 0, 0, ws.data_ptr(), _pw_dtype(t3), b * c, c, p, p, 0.0, 0,
                                              1, _stream()), "mk_instnorm_fwd_ex")
    return ws[:, 0].float()


def bias_gelu(x, bias):
    return _BiasGelu.apply(x, bias)


def gelu_backward(pre, gy, want_row_sums=False):
    """``gy * gelu'(pre)`` on contiguous ``[B, C, P]`` fp32 / bf16 fields (``pre`` holds the bias already), and, with
    ``want_row_sums``, its sum over (batch, pixels) as fp32 ``[C]`` -- the bias gradient (``mk_bias_gelu_bwd``)."""
    _need_cuda(pre, gy)
    assert pre.dim() == 3 and pre.is_contiguous() and gy.is_contiguous() and gy.shape == pre.shape and gy.dtype == pre.dtype
    b, c, p = pre.shape
    gx = torch.empty_like(pre)
    gsum = torch.zeros(c, dtype=torch.float32, device=pre.device) if want_row_sums else None
    _lib.check(_lib.load().mk_bias_gelu_bwd(pre.data_ptr(), 0, gy.data_ptr(), gx.data_ptr(), _ptr(gsum),
                                            _pw_dtype(pre), b * c, c, p, _stream()), "mk_bias_gelu_bwd")
    return gx, gsum


def affine_add(r, z, affine):
    """``r + a * z + b`` per row of two contiguous ``[B, C, H, W]`` fields of one dtype (fp32 / bf16), ``affine`` fp32
    ``[B * C, 2]`` = (a, b) from ``instance_norm_coeffs`` (``mk_affine_add``)."""
    _need_cuda(r, z, affine)
    assert r.is_contiguous() and z.is_contiguous() and r.shape == z.shape and r.dtype == z.dtype and z.dim() == 4
    B, C, H, W = z.shape
    assert affine.dtype == torch.float32 and affine.is_contiguous() and affine.numel() == 2 * B * C
    y = torch.empty_like(z)
    _lib.check(_lib.load().mk_affine_add(r.data_ptr(), z.data_ptr(), affine.data_ptr(), y.data_ptr(), _pw_dtype(z), B * C, H * W,
                                         _stream()), "mk_affine_add")
    return y


def instance_norm(x, weight, bias, eps=1e-5, fuse_gelu=False, group=None, count=None, row_sums=None):
    """``row_sums``: fp64 ``[B * C, 2]`` LOCAL (sum, sum of squares) of every row of ``x`` when its producer already has
    them (``pce_gemm(..., want_row_sums=True)``); the statistics pass over ``x`` is then skipped."""
    return _InstanceNorm.apply(x, weight, bias, eps, fuse_gelu, group, count, row_sums)


# ----------------------------------------------------------------------------
# layer norm over the channel axis of an NCHW field (csrc/chnorm.hip)
# ----------------------------------------------------------------------------
def channel_layer_norm_supported(x):
    """NCHW on the GPU in fp32 / bf16; any H * W, any C (``channel_layer_norm`` makes the field contiguous itself)."""
    return x.is_cuda and x.dim() == 4 and x.dtype in _LOWP and x.numel() > 0


class _ChannelLayerNorm(torch.autograd.Function):
    """Layer norm over C per (b, h, w) with optional fused GELU, one HBM pass each way; statistics in fp32.

    Saves ``x`` and the per-pixel (mean, rstd); the GELU pre-activation is recomputed.  The weight / bias gradients
    returned are the LOCAL sums over this rank's pixels (shared-weight reduction sums them later).
    """

    @staticmethod
    def forward(ctx, x, weight, bias, eps, fuse_gelu, out_dtype):
        _need_cuda(x)
        x = x.contiguous()
        B, C, H, W = x.shape
        y = torch.empty(x.shape, dtype=x.dtype if out_dtype is None else out_dtype, device=x.device)
        wf = None if weight is None else weight.detach().float().contiguous()
        bf = None if bias is None else bias.detach().float().contiguous()
        stats = torch.empty(B, H * W, 2, dtype=torch.float32, device=x.device)
        _lib.check(_lib.load().mk_chan_layernorm_fwd(x.data_ptr(), _pw_dtype(x), _ptr(wf),
                                                     _ptr(bf), y.data_ptr(), _pw_dtype(y),
                                                     stats.data_ptr(), B, C, H * W, float(eps), int(fuse_gelu), _stream()),
                   "mk_chan_layernorm_fwd")
        empty = x.new_empty(0, dtype=torch.float32)
        ctx.save_for_backward(x, stats, wf if wf is not None else empty, bf if bf is not None else empty)
        ctx.cfg = (weight is not None, bias is not None, bool(fuse_gelu), None if weight is None else weight.dtype,
                   None if bias is None else bias.dtype)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, stats, wf, bf = ctx.saved_tensors
        has_w, has_b, fuse, wdt, bdt = ctx.cfg
        B, C, H, W = x.shape
        gy = _lowp(gy)
        gy = gy.contiguous()
        gx = torch.empty_like(x)
        lib = _lib.load()
        want = (has_w and ctx.needs_input_grad[1]) or (has_b and ctx.needs_input_grad[2])
        ws = gwb = None
        if want:
            ws = torch.empty(lib.mk_chan_layernorm_workspace(B, C, H * W), dtype=torch.float32, device=x.device)
            gwb = torch.empty(2, C, dtype=torch.float32, device=x.device)
        _lib.check(lib.mk_chan_layernorm_bwd(x.data_ptr(), _pw_dtype(x), gy.data_ptr(), _pw_dtype(gy), stats.data_ptr(),
                                             wf.data_ptr() if has_w else 0, bf.data_ptr() if has_b else 0, gx.data_ptr(),
                                             _ptr(ws), _ptr(gwb), B, C,
                                             H * W, int(fuse), _stream()), "mk_chan_layernorm_bwd")
        gw = gwb[0].to(wdt) if (has_w and ctx.needs_input_grad[1]) else None
        gb = gwb[1].to(bdt) if (has_b and ctx.needs_input_grad[2]) else None
        return gx, gw, gb, None, None, None


def channel_layer_norm(x, weight, bias, eps=1e-5, fuse_gelu=False, out_dtype=None):
    """``act(weight * (x - mean) * rstd + bias)`` with mean / biased variance over the CHANNELS of ``x [B, C, H, W]`` at every
    grid point (``nn.LayerNorm(C)`` on the channels-last view, without the transposes), ``act`` = exact GELU when
    ``fuse_gelu``.  ``weight`` / ``bias`` may be None; ``out_dtype`` (fp32 / bf16) defaults to ``x.dtype``."""
    if not channel_layer_norm_supported(x):
        raise RuntimeError("makani_amd: channel_layer_norm needs a 4-D fp32 / bf16 field on a HIP device; there is no fallback")
    if out_dtype not in (None, torch.float32, torch.bfloat16):
        raise TypeError(f"makani_amd channel_layer_norm: unsupported out_dtype {out_dtype}")
    return _ChannelLayerNorm.apply(x, weight, bias, eps, fuse_gelu, out_dtype)


# ----------------------------------------------------------------------------
# validation metrics (csrc/metrics.hip)
# ----------------------------------------------------------------------------
GEO_METRIC_SUMS = ("l1", "sq", "cov", "var_p", "var_t")     # order of the last axis of geo_metric_sums


def _geo_metric_sums_torch(prd, tar, clim, wrow):
    """The five sums in torch float64 on the tensors' device (the CPU path of ``geo_metric_sums`` and of ``rollout_tail``)."""
    B, C, H, W = prd.shape
    p, t = prd.double(), tar.double()
    w = wrow.double().reshape(1, 1, H, 1)
    c = clim.double().reshape(1, C, H, W) if clim is not None else torch.zeros((), dtype=torch.float64, device=prd.device)
    d, pa, ta = p - t, p - c, t - c
    return torch.stack([(w * d.abs()).sum((-2, -1)), (w * d * d).sum((-2, -1)), (w * pa * ta).sum((-2, -1)),
                        (w * pa * pa).sum((-2, -1)), (w * ta * ta).sum((-2, -1))], dim=-1)


@torch.no_grad()
def geo_metric_sums(prd, tar, clim, wrow):
    """Latitude-weighted integrals of the validation metrics, ``[B, C, 5]`` float64 in the order of ``GEO_METRIC_SUMS``:
    sum w |p - t|, sum w (p - t)^2, sum w (p - c)(t - c), sum w (p - c)^2, sum w (t - c)^2 over each ``[H, W]`` field,
    with w = ``wrow[h]`` and c = ``clim`` (``[C, H, W]``, shared by all samples; ``None``: c = 0).

    CUDA tensors: one streaming HIP pass plus a fixed-order finalize (``mk_geo_metric_sums``; bitwise repeatable,
    capturable).  The prediction is read as fp32 or bf16, everything else as fp32.  CPU tensors: the same sums in
    torch float64.  No gradient flows through this op."""
    if prd.dim() != 4 or tar.shape != prd.shape:
        raise ValueError(f"geo_metric_sums: prediction {tuple(prd.shape)} and target {tuple(tar.shape)} must be equal [B, C, H, W]")
    B, C, H, W = prd.shape
    if wrow.numel() != H:
        raise ValueError(f"geo_metric_sums: wrow has {wrow.numel()} weights for {H} latitude rows")
    if clim is not None and tuple(clim.shape[-3:]) != (C, H, W):
        raise ValueError(f"geo_metric_sums: climatology {tuple(clim.shape)} does not match [C, H, W] = {(C, H, W)}")
    if not prd.is_cuda:
        return _geo_metric_sums_torch(prd, tar, clim, wrow)
    _need_cuda(prd, tar, wrow, *([clim] if clim is not None else []))
    prd = _lowp(prd)
    prd = prd.contiguous()
    tar = tar.float().contiguous()
    wrow = wrow.float().contiguous()
    clim = clim.float().contiguous() if clim is not None else None
    lib = _lib.load()
    ws = torch.empty(lib.mk_geo_metric_workspace(B, C, H), dtype=torch.float64, device=prd.device)
    out = torch.empty(B, C, 5, dtype=torch.float64, device=prd.device)
    _lib.check(lib.mk_geo_metric_sums(prd.data_ptr(), _pw_dtype(prd), tar.data_ptr(), _ptr(clim),
                                      wrow.data_ptr(), ws.data_ptr(), out.data_ptr(), B, C, H, W, _stream()), "mk_geo_metric_sums")
    return out


# ----------------------------------------------------------------------------
# training losses of the Lp family (csrc/lploss.hip)
# ----------------------------------------------------------------------------
def _geo_lp_sums_torch(prd, tar, wrow, p):
    """The two sums in torch float64 on the tensors' device, differentiable in both fields by ordinary autograd."""
    w = wrow.double().reshape(1, 1, -1, 1)
    d, t = prd.double() - tar.double(), tar.double()
    if p == 2:
        return torch.stack([(w * d * d).sum((-2, -1)), (w * t * t).sum((-2, -1))], dim=-1)
    return torch.stack([(w * d.abs()).sum((-2, -1)), (w * t.abs()).sum((-2, -1))], dim=-1)


class _GeoLpSums(torch.autograd.Function):
    """[B, C, 2] float64 (sum w |prd - tar|^p, sum w |tar|^p); one streaming pass each way (mk_geo_lp_sums, mk_geo_lp_bwd)."""

    @staticmethod
    def forward(ctx, prd, tar, wrow, p):
        B, C, H, W = prd.shape
        lib = _lib.load()
        ws = torch.empty(lib.mk_geo_lp_workspace(B, C, H), dtype=torch.float64, device=prd.device)
        out = torch.empty(B, C, 2, dtype=torch.float64, device=prd.device)
        _lib.check(lib.mk_geo_lp_sums(prd.data_ptr(), _pw_dtype(prd), tar.data_ptr(), wrow.data_ptr(), ws.data_ptr(),
                                      out.data_ptr(), p, B, C, H, W, _stream()), "mk_geo_lp_sums")
        ctx.save_for_backward(prd, tar, wrow)
        ctx.p = p
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        prd, tar, wrow = ctx.saved_tensors
        B, C, H, W = prd.shape
        gp = torch.empty_like(prd)
        g0 = g[..., 0].float().contiguous()          # the upstream gradient of s0; s1 does not depend on the prediction
        _lib.check(_lib.load().mk_geo_lp_bwd(prd.data_ptr(), _pw_dtype(prd), tar.data_ptr(), wrow.data_ptr(), g0.data_ptr(),
                                             gp.data_ptr(), ctx.p, B, C, H, W, _stream()), "mk_geo_lp_bwd")
        return gp, None, None, None


def geo_lp_sums(prd, tar, wrow, p):
    """Latitude-weighted integrals of the Lp losses, ``[B, C, 2]`` float64: ``sum w |prd - tar| ** p`` and
    ``sum w |tar| ** p`` over each ``[H, W]`` field, with w = ``wrow[h]`` and ``p`` 1 or 2.

    CUDA tensors: one streaming HIP pass plus a fixed-order finalize (``mk_geo_lp_sums``; bitwise repeatable, capturable)
    and one streaming pass for the gradient of the prediction (``mk_geo_lp_bwd``).  The prediction is read as fp32 or
    bf16 and its gradient written in the same dtype; target and weights are read as fp32.  CPU tensors, or a target that
    requires a gradient: the same sums in torch float64, differentiated by ordinary autograd."""
    if p not in (1, 2):
        raise ValueError(f"geo_lp_sums: p must be 1 or 2, got {p}")
    if prd.dim() != 4 or tar.shape != prd.shape:
        raise ValueError(f"geo_lp_sums: prediction {tuple(prd.shape)} and target {tuple(tar.shape)} must be equal [B, C, H, W]")
    if wrow.numel() != prd.shape[-2]:
        raise ValueError(f"geo_lp_sums: wrow has {wrow.numel()} weights for {prd.shape[-2]} latitude rows")
    if not prd.is_cuda or tar.requires_grad:
        return _geo_lp_sums_torch(prd, tar, wrow, int(p))
    _need_cuda(prd, tar, wrow)
    prd = _lowp(prd)
    return _GeoLpSums.apply(prd.contiguous(), tar.float().contiguous(), wrow.detach().float().contiguous(), int(p))


# ----------------------------------------------------------------------------
# per-degree power of a packed spectrum (csrc/specnorm.hip)
# ----------------------------------------------------------------------------
def _stored_triangle(L, M, l_off, m_off, device):
    """Of an ``[L, M]`` shard of a packed spectrum from degree ``l_off`` and order ``m_off`` on: ``stored`` (bool), the entries
    with ``l_off + l >= m_off + m``, and ``w`` (float64), the order weights there (1 for ``m = 0``, 2 for ``m > 0``), zero elsewhere."""
    l = torch.arange(L, device=device).reshape(L, 1) + l_off
    m = torch.arange(M, device=device).reshape(1, M) + m_off
    stored = l >= m
    w = torch.where(m == 0, 1.0, 2.0).to(torch.float64).expand(L, M)
    return stored, torch.where(stored, w, torch.zeros_like(w))


def _degree_power_torch(c, l_off, m_off):
    """The degree sums in torch float64 on the tensor's device, differentiable by ordinary autograd; the rows with
    ``l_off + l < m_off + m`` are masked out before they are squared (they may hold anything, NaN included)."""
    L, M, _ = c.shape
    stored, w = _stored_triangle(L, M, l_off, m_off, c.device)
    ri = torch.view_as_real(c).to(torch.float64)
    ri = torch.where(stored.reshape(L, M, 1, 1), ri, torch.zeros_like(ri))
    return (w.unsqueeze(-1) * (ri[..., 0] ** 2 + ri[..., 1] ** 2)).sum(dim=1).t()


class _DegreePower(torch.autograd.Function):
    """[BC, L] float64 degree sums of a packed spectrum [L, M, BC]; one streaming pass each way (mk_degree_power,
    mk_degree_power_bwd)."""

    @staticmethod
    def forward(ctx, c, l_off, m_off):
        L, M, BC = c.shape
        lib = _lib.load()
        ws = torch.empty(lib.mk_degree_power_workspace(L, M, BC), dtype=torch.float64, device=c.device)
        out = torch.empty(L, BC, dtype=torch.float64, device=c.device)
        _lib.check(lib.mk_degree_power(c.data_ptr(), ws.data_ptr(), out.data_ptr(), L, M, BC, l_off, m_off, _stream()),
                   "mk_degree_power")
        ctx.save_for_backward(c)
        ctx.offs = (l_off, m_off)
        return out.t()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        c, = ctx.saved_tensors
        L, M, BC = c.shape
        gp = g.t().to(torch.float64).contiguous()        # [L, BC], as the kernel wrote P
        gc = torch.empty_like(c)
        _lib.check(_lib.load().mk_degree_power_bwd(c.data_ptr(), gp.data_ptr(), gc.data_ptr(), L, M, BC, *ctx.offs, _stream()),
                   "mk_degree_power_bwd")
        return gc, None, None


def degree_power(c_packed, l_off=0, m_off=0):
    """Per-degree power of a packed spectrum ``[L_loc, M_loc, BC]`` complex64 (``forward_packed`` of the transforms),
    ``[BC, L_loc]`` float64: ``P[bc, l] = sum_m w(m_off + m) |c[l, m, bc]| ** 2`` with ``w(0) = 1`` and ``w(m > 0) = 2``
    (a real field's orders ``-m`` counted with ``m``).  ``l_off`` / ``m_off`` are the shard's global offsets; the rows with
    ``l_off + l < m_off + m``, which the Legendre kernels leave unwritten, are never read.  The sums add up over ``m`` shards
    and concatenate over ``l`` shards.

    CUDA tensors: one streaming HIP pass plus a fixed-order finalize (``mk_degree_power``; bitwise repeatable, capturable)
    and one streaming pass for the gradient (``mk_degree_power_bwd``: ``2 w gP c``, exact zeros in the empty triangle,
    handed to the transform's backward as it is).  CPU tensors: the same sums in torch float64, differentiated by ordinary
    autograd."""
    if c_packed.dim() != 3 or c_packed.dtype != torch.complex64:
        raise ValueError(f"degree_power: expected a complex64 spectrum [L, M, BC], got {c_packed.dtype} {tuple(c_packed.shape)}")
    if min(c_packed.shape) < 1:
        raise ValueError(f"degree_power: empty spectrum {tuple(c_packed.shape)}")
    l_off, m_off = int(l_off), int(m_off)
    if l_off < 0 or m_off < 0:
        raise ValueError(f"degree_power: offsets must not be negative, got l_off={l_off}, m_off={m_off}")
    if not c_packed.is_cuda:
        return _degree_power_torch(c_packed, l_off, m_off)
    return _DegreePower.apply(c_packed.contiguous(), l_off, m_off)


# ----------------------------------------------------------------------------
# input assembly of the step wrappers (csrc/preproc.hip)
# ----------------------------------------------------------------------------
def _history_sums_torch(xa, wt):
    """``[B, Cn, 2]`` float64 from the concatenated history ``xa`` ``[B, T, Cn, H, W]``, differentiable by autograd."""
    w = wt.double().reshape(1, -1, 1, 1, 1)
    v = xa.double()
    return torch.stack([(v * w).sum((1, 3, 4)), (v * v * w).sum((1, 3, 4))], dim=-1)


@torch.no_grad()
def history_sums(x, u, wt):
    """Weighted raw sums of the history statistics, ``[B, C + Cu, 2]`` float64: ``sum_t wt[t] sum_hw v`` and
    ``sum_t wt[t] sum_hw v ** 2`` over the channels of ``x`` ``[B, T, C, H, W]`` (fp32 or bf16) followed by those of ``u``
    ``[B, T, Cu, H, W]`` (fp32, or ``None``).

    CUDA tensors: one streaming HIP pass in fp64 plus a fixed-order finalize (``mk_history_sums``; bitwise repeatable,
    capturable).  CPU tensors: the same sums in torch float64.  No gradient flows through this op; a caller that needs
    one forms the sums with ordinary torch ops."""
    if x.dim() != 5 or (u is not None and (u.dim() != 5 or u.shape[:2] != x.shape[:2] or u.shape[3:] != x.shape[3:])):
        raise ValueError(f"history_sums: x {tuple(x.shape)} must be [B, T, C, H, W] and u, if given, [B, T, Cu, H, W]")
    B, T, C, H, W = x.shape
    if wt.numel() != T:
        raise ValueError(f"history_sums: {wt.numel()} weights for {T} history steps")
    if not x.is_cuda:
        return _history_sums_torch(x if u is None else torch.cat([x.float(), u], dim=2), wt.reshape(-1))
    _need_cuda(x, wt, *([u] if u is not None else []))
    x = _lowp(x)
    x = x.contiguous()
    u = u.float().contiguous() if u is not None else None
    wt = wt.float().reshape(-1).contiguous()
    Cu = u.shape[2] if u is not None else 0
    lib = _lib.load()
    ws = torch.empty(lib.mk_history_workspace(B, C + Cu, H), dtype=torch.float64, device=x.device)
    out = torch.empty(B, C + Cu, 2, dtype=torch.float64, device=x.device)
    _lib.check(lib.mk_history_sums(x.data_ptr(), _pw_dtype(x), _ptr(u), wt.data_ptr(), ws.data_ptr(), out.data_ptr(),
                                   B, T, C, Cu, H, W, _stream()), "mk_history_sums")
    return out


class _InputAssemble(torch.autograd.Function):
    """One pass each way (mk_input_assemble, mk_input_assemble_bwd); the gradient is that of ``x`` alone, with the
    statistics taken as constants."""

    @staticmethod
    def forward(ctx, x, u, stat, mean, std, mask_chans, mask_src, out_dtype):
        B, T, C, H, W = x.shape
        Cu = u.shape[2] if u is not None else 0
        Cs = stat.shape[0] if stat is not None else 0
        n_mask = mask_chans.numel() if mask_chans is not None else 0
        out = torch.empty(B, T * (C + Cu) + Cs, H, W, dtype=out_dtype, device=x.device)
        _lib.check(_lib.load().mk_input_assemble(x.data_ptr(), _pw_dtype(x), _ptr(u), _ptr(stat), _ptr(mean), _ptr(std),
                                                 _ptr(mask_chans), n_mask, mask_src, out.data_ptr(), _pw_dtype(out),
                                                 B, T, C, Cu, Cs, H, W, _stream()), "mk_input_assemble")
        ctx.save_for_backward(stat, std, mask_chans)
        ctx.meta = (x.dtype, mask_src, B, T, C, Cu, Cs, H, W)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        stat, std, mask_chans = ctx.saved_tensors
        x_dtype, mask_src, B, T, C, Cu, Cs, H, W = ctx.meta
        g = _lowp(g)
        g = g.contiguous()
        gx = torch.empty(B, T, C, H, W, dtype=x_dtype, device=g.device)
        n_mask = mask_chans.numel() if mask_chans is not None else 0
        _lib.check(_lib.load().mk_input_assemble_bwd(g.data_ptr(), _pw_dtype(g), _ptr(stat), _ptr(std), _ptr(mask_chans),
                                                     n_mask, mask_src, gx.data_ptr(), _pw_dtype(gx), B, T, C, Cu, Cs, H, W,
                                                     _stream()), "mk_input_assemble_bwd")
        return gx, None, None, None, None, None, None, None


def input_assemble(x, u=None, stat=None, mean=None, std=None, mask_chans=None, mask_src=-1, out_dtype=torch.float32):
    """The model input of the step wrappers in one HIP pass: ``[B, T (C + Cu) + Cs, H, W]`` in ``out_dtype`` (fp32 or
    bf16) from the predicted channels ``x`` ``[B, T, C, H, W]`` (fp32 or bf16), the unpredicted channels ``u``
    ``[B, T, Cu, H, W]``, the static features ``stat`` ``[Cs, H, W]`` shared by all samples, the statistics ``mean`` /
    ``std`` ``[B, C + Cu]`` (``(v - mean) / std``, both or neither) and ``mask_chans``, an int32 device tensor of output
    channels that are multiplied by ``stat[mask_src]``.  Everything but ``x`` is read as fp32.

    Differentiable in ``x`` only (``mk_input_assemble_bwd``): the statistics are constants to this op.  A gradient
    through the statistics is the business of the torch formulation (``Preprocessor2D._assemble_torch``).  CUDA only."""
    _need_cuda(x, *[t for t in (u, stat, mean, std, mask_chans) if t is not None])
    if x.dim() != 5:
        raise ValueError(f"input_assemble: x {tuple(x.shape)} must be [B, T, C, H, W]")
    B, T, C, H, W = x.shape
    if u is not None and (u.dim() != 5 or tuple(u.shape[:2]) != (B, T) or tuple(u.shape[3:]) != (H, W)):
        raise ValueError(f"input_assemble: u {tuple(u.shape)} does not match x {tuple(x.shape)}")
    if stat is not None and (stat.dim() != 3 or tuple(stat.shape[1:]) != (H, W)):
        raise ValueError(f"input_assemble: static features {tuple(stat.shape)} must be [Cs, {H}, {W}]")
    Cn = C + (u.shape[2] if u is not None else 0)
    if (mean is None) != (std is None) or (mean is not None and (mean.numel() != B * Cn or std.numel() != B * Cn)):
        raise ValueError(f"input_assemble: mean and std must both be [B, C + Cu] = {(B, Cn)}")
    if out_dtype not in _LOWP:
        raise ValueError(f"input_assemble: output dtype {out_dtype} is neither fp32 nor bf16")
    if mask_chans is not None and mask_chans.numel() == 0:
        mask_chans = None
    if mask_chans is not None and mask_chans.dtype != torch.int32:
        raise ValueError("input_assemble: mask_chans must be int32")
    x = _lowp(x)

    return _InputAssemble.apply(x.contiguous(), _f32(u), _f32(stat), _f32(mean), _f32(std),
                                mask_chans.contiguous() if mask_chans is not None else None, int(mask_src), out_dtype)


# ----------------------------------------------------------------------------
# the tail of an autoregressive rollout step (csrc/rollout.hip)
# ----------------------------------------------------------------------------
ROLLOUT_DEFAULT = "hip"         # MK_ROLLOUT: hip | torch.  No row of tools/rollout_bench.py is slower than torch
ROLLOUT_SUMS = GEO_METRIC_SUMS + ("sq_unweighted",)     # order of the last axis of rollout_tail's sums


def _chan_list(name, chans, C, device, allow_repeat=False, who="rollout_tail"):
    """A channel list as an int32 tensor on ``device`` (None when empty).  A python list is range-checked here; a tensor is
    taken as it is (the caller built it once: nothing is uploaded or read back, so the call stays capturable)."""
    if chans is None:
        return None
    if torch.is_tensor(chans):
        if chans.dtype != torch.int32 or chans.dim() != 1:
            raise ValueError(f"{who}: {name} must be a 1-D int32 tensor, got {chans.dtype} {tuple(chans.shape)}")
        if chans.device != device:
            raise ValueError(f"{who}: {name} on {chans.device}, the model output on {device}")
        return chans.contiguous() if chans.numel() else None
    chans = [int(c) for c in chans]
    if not chans:
        return None
    if min(chans) < 0 or max(chans) >= C:
        raise ValueError(f"{who}: {name} {chans} out of range for {C} channels")
    if not allow_repeat and len(set(chans)) != len(chans):
        raise ValueError(f"{who}: {name} {chans} repeats a channel")
    return torch.tensor(chans, dtype=torch.int32, device=device)


def _rollout_tail_torch(yn, mean, std, mask, mask_chans, x_last, residual, scale, hold_chans, tar, clim, wrow, err_map,
                        emit_chans, emit_scale, emit_shift):
    """The steps of ``rollout_tail`` as torch ops on the tensors' device, one rounding per operation; the sums in torch
    float64 (the sixth from ``d`` rounded to fp32).  Arguments as ``rollout_tail`` has normalised them."""
    B, C, H, W = yn.shape
    v = yn.float()
    if mean is not None:
        v = v * std.reshape(B, C, 1, 1)
        v = v + mean.reshape(B, C, 1, 1)

    def hit(chans):
        h = torch.zeros(C, dtype=torch.bool, device=yn.device)
        h[chans.long()] = True
        return h.reshape(1, C, 1, 1)

    if mask_chans is not None:
        v = v * torch.where(hit(mask_chans), mask.reshape(1, 1, H, W), torch.ones((), dtype=torch.float32, device=yn.device))
    if residual:
        if scale is not None:
            v = v * scale.reshape(1, C, 1, 1)
        v = x_last + v
    if hold_chans is not None:
        v = torch.where(hit(hold_chans), x_last, v)
    pred = v.contiguous() if v.data_ptr() != yn.data_ptr() else v.clone()
    sums = emit = None
    if tar is not None:
        d = pred - tar
        sums = torch.cat([_geo_metric_sums_torch(pred, tar, clim, wrow), d.double().square().sum((-2, -1)).unsqueeze(-1)], dim=-1)
        if err_map is not None:
            for b in range(B):
                err_map += d[b] * d[b]
    if emit_chans is not None:
        emit = pred[:, emit_chans.long()]
        if emit_scale is not None:
            emit = emit * emit_scale.reshape(1, -1, 1, 1)
        if emit_shift is not None:
            emit = emit + emit_shift.reshape(1, -1, 1, 1)
        emit = emit.contiguous()
    return pred, sums, emit


@torch.no_grad()
def rollout_tail(yn, mean=None, std=None, mask=None, mask_chans=None, x_last=None, residual=False, scale=None, hold_chans=None,
                 tar=None, clim=None, wrow=None, err_map=None, emit_chans=None, emit_scale=None, emit_shift=None):
    """Everything a rollout step does behind the model call, in one pass over the model output ``yn`` ``[B, C, H, W]`` (fp32
    or bf16): returns ``(pred, sums, emit)`` and updates ``err_map`` in place.  Per point, in this order, every product
    and sum an fp32 rounding of its own:

    * ``v = yn * std + mean`` with ``mean`` / ``std`` of ``B * C`` elements, both or neither (``history_denormalize``);
    * ``v = v * mask`` for the channels ``mask_chans`` with ``mask`` ``[H, W]`` (``mask_output``);
    * ``v = x_last + v * scale`` when ``residual`` (``scale`` ``[C]`` optional), ``x_last`` ``[B, C, H, W]`` fp32, which may
      be the last history step of the step's input, a strided view read in place (``add_residual``);
    * ``v = x_last`` for the channels ``hold_chans``;
    * ``pred = v``, fp32 ``[B, C, H, W]``;
    * with ``tar`` ``[B, C, H, W]`` and ``wrow`` ``[H]``: ``d = pred - tar`` and ``sums`` ``[B, C, 6]`` float64 in the order of
      ``ROLLOUT_SUMS`` -- the five of ``geo_metric_sums`` (``clim`` ``[C, H, W]`` or None) and the unweighted sum of
      ``d * d``; ``err_map`` ``[C, H, W]`` fp32 (contiguous) gets ``+= d[b] * d[b]`` for b = 0, 1, ... in that order;
    * ``emit = pred[:, emit_chans] * emit_scale + emit_shift`` ``[B, K, H, W]`` fp32 (scale and shift ``[K]``, each optional).

    Channel lists are python lists (checked against C) or 1-D int32 tensors on the device (taken as they are; an entry
    outside ``[0, C)`` matches nothing in the kernel).  ``sums`` / ``emit`` are None without ``tar`` / ``emit_chans``.

    ``MK_ROLLOUT=hip`` (read on every call): CUDA tensors take one HIP pass plus a fixed-order finalize
    (``mk_rollout_tail``; bitwise repeatable, capturable).  CPU tensors, and ``MK_ROLLOUT=torch``, take
    ``_rollout_tail_torch``, the same steps as torch ops.  No gradient flows through this op."""
    hip = _hip_or_torch("MK_ROLLOUT", ROLLOUT_DEFAULT)
    if yn.dim() != 4:
        raise ValueError(f"rollout_tail: model output {tuple(yn.shape)} must be [B, C, H, W]")
    B, C, H, W = yn.shape
    dev = yn.device
    if (mean is None) != (std is None) or (mean is not None and (mean.numel() != B * C or std.numel() != B * C)):
        raise ValueError(f"rollout_tail: mean and std must both have B * C = {B * C} elements, got "
                         f"{None if mean is None else tuple(mean.shape)} and {None if std is None else tuple(std.shape)}")
    mask_chans = _chan_list("mask_chans", mask_chans, C, dev)
    hold_chans = _chan_list("hold_chans", hold_chans, C, dev)
    emit_chans = _chan_list("emit_chans", emit_chans, C, dev, allow_repeat=True)
    if mask_chans is not None and (mask is None or tuple(mask.shape[-2:]) != (H, W) or mask.numel() != H * W):
        raise ValueError(f"rollout_tail: masked channels need a mask [H, W] = {(H, W)}, got {None if mask is None else tuple(mask.shape)}")
    if (residual or hold_chans is not None) and (x_last is None or tuple(x_last.shape) != (B, C, H, W)):
        raise ValueError(f"rollout_tail: the residual and the held channels need x_last {(B, C, H, W)}, got "
                         f"{None if x_last is None else tuple(x_last.shape)}")
    if scale is not None and (not residual or scale.numel() != C):
        raise ValueError(f"rollout_tail: scale {tuple(scale.shape)} needs residual=True and C = {C} elements")
    if tar is None and (clim is not None or err_map is not None):
        raise ValueError("rollout_tail: clim and err_map need a target")
    if tar is not None:
        if tuple(tar.shape) != (B, C, H, W):
            raise ValueError(f"rollout_tail: target {tuple(tar.shape)} does not match the model output {(B, C, H, W)}")
        if wrow is None or wrow.numel() != H:
            raise ValueError(f"rollout_tail: wrow has {0 if wrow is None else wrow.numel()} weights for {H} latitude rows")
        if clim is not None and tuple(clim.shape[-3:]) != (C, H, W):
            raise ValueError(f"rollout_tail: climatology {tuple(clim.shape)} does not match [C, H, W] = {(C, H, W)}")
        if err_map is not None and (tuple(err_map.shape) != (C, H, W) or err_map.dtype != torch.float32
                                    or not err_map.is_contiguous() or err_map.device != dev):
            raise ValueError(f"rollout_tail: err_map must be a contiguous fp32 [C, H, W] = {(C, H, W)} on {dev}, got "
                             f"{err_map.dtype} {tuple(err_map.shape)} on {err_map.device}")
    K = emit_chans.numel() if emit_chans is not None else 0
    for name, t in (("emit_scale", emit_scale), ("emit_shift", emit_shift)):
        if t is not None and (K == 0 or t.numel() != K):
            raise ValueError(f"rollout_tail: {name} {tuple(t.shape)} needs K = {K} emitted channels")

    yn = _lowp(yn)
    yn = yn.detach()
    mean, std, mask, scale, tar, clim, wrow = (_f32(t) for t in (mean, std, mask, scale, tar, clim, wrow))
    emit_scale, emit_shift = _f32(emit_scale), _f32(emit_shift)
    if not (residual or hold_chans is not None):
        x_last = None
    if x_last is not None:
        x_last = x_last.detach().float()
    if not (hip and yn.is_cuda):
        return _rollout_tail_torch(yn, mean, std, mask, mask_chans, x_last, bool(residual), scale, hold_chans, tar, clim, wrow,
                                   err_map, emit_chans, emit_scale, emit_shift)
    _need_cuda(*[t for t in (mean, std, mask, x_last, scale, tar, clim, wrow, emit_scale, emit_shift) if t is not None])
    yn = yn.contiguous()
    x_bstride = 0
    if x_last is not None:
        # read in place when every sample is a contiguous [C, H, W] block (the last history step of the input is)
        if tuple(x_last.stride()[1:]) != (H * W, W, 1) or (B > 1 and x_last.stride(0) < C * H * W):
            x_last = x_last.contiguous()
        x_bstride = x_last.stride(0) if B > 1 else C * H * W
    lib = _lib.load()
    pred = torch.empty(B, C, H, W, dtype=torch.float32, device=dev)
    ws = sums = emit = None
    if tar is not None:
        ws = torch.empty(lib.mk_rollout_tail_workspace(B, C, H), dtype=torch.float64, device=dev)
        sums = torch.empty(B, C, 6, dtype=torch.float64, device=dev)
    if K:
        emit = torch.empty(B, K, H, W, dtype=torch.float32, device=dev)
    _lib.check(lib.mk_rollout_tail(yn.data_ptr(), _pw_dtype(yn), _ptr(mean), _ptr(std), _ptr(mask), _ptr(mask_chans),
                                   mask_chans.numel() if mask_chans is not None else 0, _ptr(x_last), x_bstride, int(bool(residual)),
                                   _ptr(scale), _ptr(hold_chans), hold_chans.numel() if hold_chans is not None else 0,
                                   pred.data_ptr(), _ptr(tar), _ptr(clim), _ptr(wrow), _ptr(ws), _ptr(sums), _ptr(err_map),
                                   _ptr(emit), _ptr(emit_chans), _ptr(emit_scale), _ptr(emit_shift), K, B, C, H, W, _stream()),
               "mk_rollout_tail")
    return pred, sums, emit


# ----------------------------------------------------------------------------
# dataset statistics (csrc/stats.hip)
# ----------------------------------------------------------------------------
STATS_DEFAULT = "hip"           # MK_STATS: hip | torch.  No row of tools/stats_bench.py is slower than torch
FIELD_STATS_SUMS = ("d", "d_sq", "diff", "diff_sq")     # order of the last axis of field_stats' sums


def _field_stats_torch(x, prev, pivot, wrow, tsum, wind_u, wind_v):
    """The sums of ``field_stats`` as float64 torch ops on the tensors' device; ``tsum`` is added to sample by sample."""
    T, C, H, W = x.shape
    xd = x.double()
    w = wrow.double().reshape(1, 1, H, 1)
    d = xd - pivot.double().reshape(1, C, 1, 1) if pivot is not None else xd
    if prev is not None:
        e = xd - torch.cat([prev.double().reshape(1, C, H, W), xd[:-1]], dim=0)
    else:
        e = xd[1:] - xd[:-1]                     # empty for T = 1: the sums over it are exact zeros
    sums = torch.stack([(w * d).sum((0, 2, 3)), (w * d * d).sum((0, 2, 3)), (w * e).sum((0, 2, 3)), (w * e * e).sum((0, 2, 3))], dim=-1)
    minmax = torch.stack([x.amin((0, 2, 3)), x.amax((0, 2, 3))], dim=-1)        # amin / amax keep a NaN, as np.min does
    sums = torch.where(torch.isnan(minmax[:, :1]), float("nan"), sums)
    for t in range(T):
        tsum += xd[t]
    wsums = None
    if wind_u is not None:
        u, v = x[:, wind_u.long()], x[:, wind_v.long()]
        # fp32, one rounding per operation, then widened.  The root is taken in float64 and rounded to fp32, which is the
        # correctly rounded fp32 root (53 >= 2 * 24 + 2 bits); torch's own fp32 sqrt is not correctly rounded everywhere
        m = torch.sqrt((u * u + v * v).double()).float().double()
        wsums = torch.stack([m.sum((0, 2, 3)), (m * m).sum((0, 2, 3))], dim=-1)
    return sums, minmax, wsums


@torch.no_grad()
def field_stats(x, wrow, tsum, prev=None, pivot=None, wind_u=None, wind_v=None):
    """One pass over a batch ``x`` ``[T, C, H, W]`` (fp32, consecutive in time) for the dataset statistics: returns
    ``(sums, minmax, wsums)`` and adds the samples to ``tsum`` in place.

    * ``sums`` ``[C, 4]`` float64 in the order of ``FIELD_STATS_SUMS``: ``sum w d``, ``sum w d^2``, ``sum w e``, ``sum w e^2``
      with ``d = x - pivot[c]`` (``pivot`` ``[C]`` fp32 or None: 0), ``e = x[t] - x[t - 1]``, both formed in float64, and
      ``w = wrow[h]``.  ``e`` runs over ``t = 1 ... T - 1``, and over ``t = 0`` too when ``prev`` ``[C, H, W]`` (the sample
      before the first) is given;
    * ``minmax`` ``[C, 2]`` fp32; a NaN in a channel makes its min, max and sums NaN;
    * ``tsum`` ``[C, H, W]`` float64 (contiguous): ``tsum += x[0]``, ``+= x[1]``, ... in that order;
    * ``wsums`` ``[n_wind, 2]`` float64 (None without pairs): the unweighted ``sum m``, ``sum m^2`` of
      ``m = sqrt(u * u + v * v)`` (fp32, one rounding per operation) for the channel pairs ``(wind_u[k], wind_v[k])``;
      python lists (checked against C, the u channels distinct) or 1-D int32 tensors on the device (taken as they are).

    ``MK_STATS=hip`` (read on every call): CUDA tensors take one HIP pass plus a fixed-order finish (``mk_field_stats``;
    bitwise repeatable, capturable).  CPU tensors, and ``MK_STATS=torch``, take ``_field_stats_torch``, the same sums as
    float64 torch ops.  No gradient flows through this op."""
    hip = _hip_or_torch("MK_STATS", STATS_DEFAULT)
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError(f"field_stats: the batch must be fp32 [T, C, H, W], got {x.dtype} {tuple(x.shape)}")
    T, C, H, W = x.shape
    dev = x.device
    if T < 1 or C < 1 or H < 1 or W < 1:
        raise ValueError(f"field_stats: empty batch {tuple(x.shape)}")
    if wrow.numel() != H:
        raise ValueError(f"field_stats: wrow has {wrow.numel()} weights for {H} latitude rows")
    if tuple(tsum.shape) != (C, H, W) or tsum.dtype != torch.float64 or not tsum.is_contiguous() or tsum.device != dev:
        raise ValueError(f"field_stats: tsum must be a contiguous float64 [C, H, W] = {(C, H, W)} on {dev}, got "
                         f"{tsum.dtype} {tuple(tsum.shape)} on {tsum.device}")
    if prev is not None and (tuple(prev.shape[-3:]) != (C, H, W) or prev.numel() != C * H * W):
        raise ValueError(f"field_stats: prev {tuple(prev.shape)} does not match [C, H, W] = {(C, H, W)}")
    if pivot is not None and pivot.numel() != C:
        raise ValueError(f"field_stats: pivot has {pivot.numel()} elements for {C} channels")
    if (wind_u is None) != (wind_v is None):
        raise ValueError("field_stats: wind_u and wind_v come together")
    wind_u = _chan_list("wind_u", wind_u, C, dev, who="field_stats")
    wind_v = _chan_list("wind_v", wind_v, C, dev, allow_repeat=True, who="field_stats")
    if (wind_u is None) != (wind_v is None) or (wind_u is not None and wind_u.numel() != wind_v.numel()):
        raise ValueError("field_stats: wind_u and wind_v must name the same number of channels")

    x = x.detach()
    prev, pivot, wrow = _f32(prev), _f32(pivot), _f32(wrow)
    if not (hip and x.is_cuda):
        return _field_stats_torch(x, prev, pivot, wrow, tsum, wind_u, wind_v)
    _need_cuda(*[t for t in (prev, pivot, wrow) if t is not None])
    x = x.contiguous()
    n_wind = wind_u.numel() if wind_u is not None else 0
    lib = _lib.load()
    ws = torch.empty(lib.mk_field_stats_workspace(C, H, n_wind), dtype=torch.float64, device=dev)
    sums = torch.empty(C, 4, dtype=torch.float64, device=dev)
    minmax = torch.empty(C, 2, dtype=torch.float32, device=dev)
    wsums = torch.empty(n_wind, 2, dtype=torch.float64, device=dev) if n_wind else None
    _lib.check(lib.mk_field_stats(x.data_ptr(), _ptr(prev), _ptr(pivot), wrow.data_ptr(), ws.data_ptr(), sums.data_ptr(),
                                  minmax.data_ptr(), tsum.data_ptr(), _ptr(wind_u), _ptr(wind_v), n_wind, _ptr(wsums), T, C, H, W,
                                  _stream()), "mk_field_stats")
    return sums, minmax, wsums


# ----------------------------------------------------------------------------
# dataset histograms (csrc/hist.hip)
# ----------------------------------------------------------------------------
HIST_DEFAULT = "hip"            # MK_HIST: hip | torch.  No row of tools/hist_bench.py is slower than torch
HIST_MAX_BINS = 4096            # what mk_field_hist takes: the edge table and one bin array in 32,776 bytes of LDS
FIELD_HIST_OUTSIDE = ("below", "above", "nan")          # order of the last axis of field_hist's outside


def hist_edges(lo, hi, nbins, dtype=np.float32):
    """The bin edges ``[C, nbins + 1]`` that ``np.histogram(a, bins=nbins, range=(lo[c], hi[c]))`` returns for data ``a`` of
    ``dtype`` and Python-float bounds, bit for bit: ``np.linspace`` over the range in ``dtype`` (numpy computes it in float64
    and rounds once).  ``lo`` and ``hi`` are scalars or ``[C]``; ``lo == hi`` widens the range by 0.5 each way, as numpy
    does.  Raises ``ValueError`` for non-finite bounds, ``lo > hi``, ``nbins < 1`` and for a table that is not strictly
    increasing in ``dtype`` ("Too many bins for data range", numpy's words)."""
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError(f"hist_edges: the edge dtype must be float32 or float64, got {dtype}")
    if int(nbins) != nbins or nbins < 1:
        raise ValueError(f"hist_edges: nbins must be a positive integer, got {nbins!r}")
    nbins = int(nbins)
    lo, hi = np.atleast_1d(np.asarray(lo, dtype=np.float64)), np.atleast_1d(np.asarray(hi, dtype=np.float64))
    if lo.ndim != 1 or lo.shape != hi.shape or lo.size < 1:
        raise ValueError(f"hist_edges: lo {lo.shape} and hi {hi.shape} must be scalars or [C]")
    out = np.empty((lo.size, nbins + 1), dtype=dtype)
    for c, (first, last) in enumerate(zip(lo.tolist(), hi.tolist())):
        if not (np.isfinite(first) and np.isfinite(last)):
            raise ValueError(f"hist_edges: channel {c}: the range [{first}, {last}] is not finite")
        if first > last:
            raise ValueError(f"hist_edges: channel {c}: max must be larger than min in the range [{first}, {last}]")
        if first == last:
            first, last = first - 0.5, last + 0.5
        out[c] = np.linspace(first, last, nbins + 1, endpoint=True, dtype=dtype)
        if np.any(out[c, :-1] >= out[c, 1:]):
            raise ValueError(f"hist_edges: channel {c}: Too many bins for data range. Cannot create {nbins} finite-sized bins "
                             f"in [{first}, {last}] in {dtype}.")
    return out


def _field_hist_torch(x, edges, counts, outside):
    """``field_hist`` as torch ops on the tensors' device, exact by the same definition: ``bucketize`` of the float64 points
    against the channel's table, the last edge sent to the last bin, ``bincount``."""
    nbins = counts.shape[1]
    for c in range(x.shape[1]):
        v = x[:, c].reshape(-1).double()
        e = edges[c]
        nan, below, above = torch.isnan(v), v < e[0], v > e[-1]
        idx = (torch.bucketize(v[~(nan | below | above)], e, right=True) - 1).clamp_(max=nbins - 1)
        counts[c] += torch.bincount(idx, minlength=nbins)
        if outside is not None:
            outside[c] += torch.stack([below.sum(), above.sum(), nan.sum()])


@torch.no_grad()
def field_hist(x, edges, counts, outside=None):
    """Adds the per-channel histograms of a batch ``x`` ``[T, C, H, W]`` (fp32) to ``counts`` in place; returns ``counts``.

    * ``edges`` ``[C, nbins + 1]`` float64 (contiguous): per channel a strictly increasing table, as ``hist_edges`` builds
      (an fp32 table widened, which is exact).  That it increases is the caller's to see to: ``hist_edges`` checks it;
    * ``counts`` ``[C, nbins]`` int64 (contiguous), added to: bin ``i`` counts ``edges[i] <= x < edges[i + 1]``, the last bin
      is closed on the right -- the counts of ``np.histogram`` with these edges, exactly, whatever path runs;
    * ``outside`` ``[C, 3]`` int64 (contiguous) or None, added to, in the order of ``FIELD_HIST_OUTSIDE``: the points below
      the first edge, above the last, and the NaNs, which no bin counts.

    ``MK_HIST=hip`` (read on every call): CUDA tensors with up to ``HIST_MAX_BINS`` bins take one HIP pass
    (``mk_field_hist``: bins in LDS, 64-bit integer atomics to ``counts``; the same result every run, capturable).  CPU
    tensors, more bins, and ``MK_HIST=torch`` take ``_field_hist_torch``; the two are equal, not close.  No gradient flows
    through this op.

    Speed, not counts: the HIP pass guesses the bin as if the table were uniform and walks from the guess to the right bin
    one edge at a time, so it is fast for near-uniform tables (``hist_edges``).  A strongly non-uniform table, such as
    quantile edges, stays exact but can cost up to ``nbins`` dependent LDS reads per point; its time is not measured, and
    ``MK_HIST=torch`` (a binary search) is the path to try there."""
    hip = _hip_or_torch("MK_HIST", HIST_DEFAULT)
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError(f"field_hist: the batch must be fp32 [T, C, H, W], got {x.dtype} {tuple(x.shape)}")
    T, C, H, W = x.shape
    dev = x.device
    if T < 1 or C < 1 or H < 1 or W < 1:
        raise ValueError(f"field_hist: empty batch {tuple(x.shape)}")
    if edges.dim() != 2 or edges.shape[0] != C or edges.shape[1] < 2 or edges.dtype != torch.float64 or not edges.is_contiguous() \
            or edges.device != dev:
        raise ValueError(f"field_hist: edges must be a contiguous float64 [C, nbins + 1] with C = {C} on {dev}, got "
                         f"{edges.dtype} {tuple(edges.shape)} on {edges.device}")
    nbins = edges.shape[1] - 1
    if tuple(counts.shape) != (C, nbins) or counts.dtype != torch.int64 or not counts.is_contiguous() or counts.device != dev:
        raise ValueError(f"field_hist: counts must be a contiguous int64 [C, nbins] = {(C, nbins)} on {dev}, got "
                         f"{counts.dtype} {tuple(counts.shape)} on {counts.device}")
    if outside is not None and (tuple(outside.shape) != (C, 3) or outside.dtype != torch.int64 or not outside.is_contiguous()
                                or outside.device != dev):
        raise ValueError(f"field_hist: outside must be a contiguous int64 [C, 3] = {(C, 3)} on {dev}, got "
                         f"{outside.dtype} {tuple(outside.shape)} on {outside.device}")
    x = x.detach()
    if not (hip and x.is_cuda and nbins <= HIST_MAX_BINS):
        _field_hist_torch(x, edges, counts, outside)
        return counts
    x = x.contiguous()
    _lib.check(_lib.load().mk_field_hist(x.data_ptr(), edges.data_ptr(), counts.data_ptr(), _ptr(outside), nbins, T, C, H, W,
                                         _stream()), "mk_field_hist")
    return counts


# ----------------------------------------------------------------------------
# ensemble scores (csrc/ens.hip)
# ----------------------------------------------------------------------------
ENSEMBLE_DEFAULT = "hip"        # MK_ENSEMBLE: hip | torch.  The rule of DESIGN section 19 on tools/ens_bench.py
ENSEMBLE_MAX_MEMBERS = 64       # what mk_ens_sums takes: a thread sorts the members of its point in registers
ENSEMBLE_SUMS = ("abs_err", "pair_dist", "mean_sq_err", "variance")     # order of the last axis of ensemble_sums: a, g, q, v
_ENS_TORCH_CHUNK = 1 << 26      # ensemble elements per channel chunk of the torch formulation (its float64 temporaries)


def _ensemble_sums_torch(ens, tar, wrow, ranks=None, skipped=None):
    """``ensemble_sums`` as torch float64 ops on the tensors' device, by the same definition (``ens`` ``[B, E, C, H, W]``):
    a sort over the member axis for ``g``, the two-pass variance, NaN points counted and made NaN by hand.  The channels
    are walked in chunks so that a temporary holds at most ``_ENS_TORCH_CHUNK`` elements; no host synchronisation."""
    B, E, C, H, W = ens.shape
    dev = ens.device
    w = wrow.double().reshape(1, 1, H, 1)
    coef = (2.0 * torch.arange(1, E + 1, dtype=torch.float64, device=dev) - E - 1.0).reshape(1, E, 1, 1, 1)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    out = torch.empty(B, C, 4, dtype=torch.float64, device=dev)
    step = max(1, _ENS_TORCH_CHUNK // max(1, B * E * H * W))
    for c0 in range(0, C, step):
        x, y = ens[:, :, c0:c0 + step].double(), tar[:, c0:c0 + step].double()
        bad = torch.isnan(y) | torch.isnan(x).any(dim=1)
        a = (x - y.unsqueeze(1)).abs().sum(dim=1) / E
        g = (coef * torch.sort(x, dim=1).values).sum(dim=1) * (2.0 / (E * E))
        m = x.sum(dim=1) / E
        q = (m - y) ** 2
        v = ((x - m.unsqueeze(1)) ** 2).sum(dim=1) / (E - 1) if E > 1 else torch.full_like(m, float("nan"))
        for k, f in enumerate((a, g, q, v)):
            out[:, c0:c0 + step, k] = (w * torch.where(bad, nan, f)).sum(dim=(-2, -1))
        if ranks is not None:
            cc = y.shape[1]
            r = (x < y.unsqueeze(1)).sum(dim=1)                                  # [B, cc, H, W], 0 ... E
            idx = torch.where(bad, E + 1, r) + (E + 2) * torch.arange(cc, device=dev).reshape(1, cc, 1, 1)
            cnt = torch.zeros(cc * (E + 2), dtype=torch.int64, device=dev)
            cnt.scatter_add_(0, idx.reshape(-1), torch.ones(idx.numel(), dtype=torch.int64, device=dev))
            ranks[c0:c0 + step] += cnt.view(cc, E + 2)[:, :E + 1]
        if skipped is not None:
            skipped[c0:c0 + step] += bad.sum(dim=(0, 2, 3))
    return out


def _ensemble_operands(op, ens, tar, wrow):
    """The checks ``ensemble_sums`` and ``ensemble_crps_sums`` share on an ensemble, its target ``[B, C, H, W]`` and the row
    weights, under the name ``op``; returns the ensemble as ``[B, E, C, H, W]`` (a ``[B * E, C, H, W]`` one viewed, member fastest)."""
    if tar.dim() != 4:
        raise ValueError(f"{op}: the target must be [B, C, H, W], got {tuple(tar.shape)}")
    B, C, H, W = tar.shape
    if ens.dim() == 4 and B >= 1 and ens.shape[0] % B == 0 and tuple(ens.shape[1:]) == (C, H, W):
        ens = ens.view(B, ens.shape[0] // B, C, H, W) if ens.is_contiguous() else ens.reshape(B, ens.shape[0] // B, C, H, W)
    if ens.dim() != 5 or ens.shape[0] != B or tuple(ens.shape[2:]) != (C, H, W) or ens.shape[1] < 1 or min(B, C, H, W) < 1:
        raise ValueError(f"{op}: ensemble {tuple(ens.shape)} must be [B, E, C, H, W] or [B * E, C, H, W] for a target "
                         f"{tuple(tar.shape)}")
    if tar.device != ens.device or wrow.device != ens.device:
        raise ValueError(f"{op}: ensemble on {ens.device}, target on {tar.device}, wrow on {wrow.device}")
    if wrow.numel() != H:
        raise ValueError(f"{op}: wrow has {wrow.numel()} weights for {H} latitude rows")
    return ens


def _ens_sums_launch(ens, tar, wrow, ranks=None, skipped=None):
    """One ``mk_ens_sums`` pass over fp32 / bf16 members ``[B, E, C, H, W]``, ``tar`` and ``wrow`` fp32 and contiguous: the
    ``[B, C, 4]`` float64 sums, and the members and the batch stride the kernel read them with (``mk_ens_crps_bwd`` reads them
    the same way).  Every member's ``[C, H, W]`` block must be contiguous -- else the ensemble is copied --; the batch and member
    strides are free."""
    B, E, C, H, W = ens.shape
    if ens.stride()[2:] != (H * W, W, 1) or min(ens.stride(0), ens.stride(1)) < C * H * W:
        ens = ens.contiguous()
    lib = _lib.load()
    ws = torch.empty(lib.mk_ens_workspace(B, C, H), dtype=torch.float64, device=ens.device)
    out = torch.empty(B, C, 4, dtype=torch.float64, device=ens.device)
    bstride = ens.stride(0) if B > 1 else E * ens.stride(1)      # a stride of a size-1 axis means nothing
    _lib.check(lib.mk_ens_sums(ens.data_ptr(), _pw_dtype(ens), bstride, ens.stride(1), tar.data_ptr(), wrow.data_ptr(),
                               ws.data_ptr(), out.data_ptr(), _ptr(ranks), _ptr(skipped), B, E, C, H, W, _stream()), "mk_ens_sums")
    return out, ens, bstride


@torch.no_grad()
def ensemble_sums(ens, tar, wrow, ranks=None, skipped=None):
    """Latitude-weighted integrals of the ensemble scores, ``[B, C, 4]`` float64 in the order of ``ENSEMBLE_SUMS``, of an
    ensemble ``ens`` ``[B, E, C, H, W]`` (a ``[B * E, C, H, W]`` model output is viewed, member fastest) against a target
    ``tar`` ``[B, C, H, W]``.  Per point, members ``x_e`` and target ``y`` widened to float64:

    * ``a = mean_e |x_e - y|``, ``g = mean_ef |x_e - x_f|`` (over all E^2 pairs; computed from the sorted members),
    * ``m = mean_e x_e``, ``q = (m - y)^2``, ``v = sum_e (x_e - m)^2 / (E - 1)`` (NaN for ``E = 1``),

    each summed over the field with ``w = wrow[h]``.  CRPS is ``a - g / 2``, the fair CRPS ``a - g E / (2 (E - 1))``.

    * ``ranks`` ``[C, E + 1]`` int64 (contiguous) or None, added to: the histogram of ``r = #{e : x_e < y}`` (a member
      equal to the target is not below it);
    * ``skipped`` ``[C]`` int64 (contiguous) or None, added to: the points whose target or one of whose members is NaN.
      Such a point is not ranked and makes the four sums of its ``(b, c)`` NaN.  Infinite values are out of contract.

    ``MK_ENSEMBLE=hip`` (read on every call): CUDA tensors with 2 to ``ENSEMBLE_MAX_MEMBERS`` members take one HIP pass
    (``mk_ens_sums``: fp32 or bf16 members read in place through their batch and member strides, no floating-point atomics,
    the same bits every run, capturable).  CPU tensors, ``E = 1``, more members and ``MK_ENSEMBLE=torch`` take
    ``_ensemble_sums_torch``.  No gradient flows through this op."""
    hip = _hip_or_torch("MK_ENSEMBLE", ENSEMBLE_DEFAULT)
    ens = _ensemble_operands("ensemble_sums", ens, tar, wrow)
    E, C, dev = ens.shape[1], ens.shape[2], ens.device
    for name, t, shape in (("ranks", ranks, (C, E + 1)), ("skipped", skipped, (C,))):
        if t is not None and (tuple(t.shape) != shape or t.dtype != torch.int64 or not t.is_contiguous() or t.device != dev):
            raise ValueError(f"ensemble_sums: {name} must be a contiguous int64 {list(shape)} on {dev}, got {t.dtype} "
                             f"{tuple(t.shape)} on {t.device}")
    ens, tar = ens.detach(), tar.detach()
    if not (hip and ens.is_cuda and 2 <= E <= ENSEMBLE_MAX_MEMBERS):
        return _ensemble_sums_torch(ens, tar, wrow, ranks, skipped)
    return _ens_sums_launch(_lowp(ens), tar.float().contiguous(), wrow.float().contiguous(), ranks, skipped)[0]


# ----------------------------------------------------------------------------
# ensemble forecast products (csrc/ens.hip: mk_ens_products)
# ----------------------------------------------------------------------------
ENS_PRODUCTS_DEFAULT = "hip"    # MK_ENS_PRODUCTS: hip | torch.  No row of tools/ens_products_bench.py is slower than torch
ENS_PRODUCTS_MAX = 16           # products per launch of mk_ens_products (its [K][TP] LDS region)
ENS_PRODUCT_KINDS = ("mean", "std", "order", "above", "below")          # the kind codes of mk_ens_products, by position


def quantile_position(q, E):
    """``(k, t)`` of the quantile ``q`` in [0, 1] of ``E`` members by numpy's ``linear`` method: float64 ``h = q (E - 1)``,
    ``k = floor(h)``, ``t = h - k``; the quantile is ``x_(k) + t (x_(k+1) - x_(k))`` over the members sorted ascending, ranks from 0.
    ``q = 1`` is ``(E - 1, 0.0)``: the maximum itself, nothing is read behind it."""
    q, E = float(q), int(E)
    if not 0.0 <= q <= 1.0 or E < 1:
        raise ValueError(f"quantile_position: q = {q} must lie in [0, 1] and E = {E} be at least 1")
    if q == 1.0:
        return E - 1, 0.0
    h = q * (E - 1)
    k = int(math.floor(h))
    return k, h - k


def _ens_product_table(kinds, orders, fracs, E):
    """The product table as ``mk_ens_products`` takes it (int32 kinds and ranks, float64 fractions, numpy), checked as it checks it."""
    kinds = [ENS_PRODUCT_KINDS.index(k) if isinstance(k, str) and k in ENS_PRODUCT_KINDS else k for k in kinds]
    K = len(kinds)
    if K < 1 or len(orders) != K or len(fracs) != K:
        raise ValueError(f"ensemble_products: {K} kinds, {len(orders)} orders, {len(fracs)} fracs; need one of each per product")
    for i, kind in enumerate(kinds):
        if kind not in range(len(ENS_PRODUCT_KINDS)):
            raise ValueError(f"ensemble_products: unknown kind {kind!r} of product {i} ({', '.join(ENS_PRODUCT_KINDS)} or 0 ... 4)")
        if kind == 2:
            k, t = int(orders[i]), float(fracs[i])
            if not 0.0 <= t < 1.0 or not 0 <= k <= (E - 1 if t == 0.0 else E - 2):
                raise ValueError(f"ensemble_products: product {i} has rank {k} and fraction {t} for {E} members: need t in [0, 1) "
                                 "and k in 0 ... E - 1 (E - 2 with a fraction)")
    return (np.asarray(kinds, dtype=np.int32), np.asarray([int(k) for k in orders], dtype=np.int32),
            np.asarray([float(t) for t in fracs], dtype=np.float64))


def _ensemble_products_torch(ens, kinds, orders, fracs, idx, thr, scale, shift, out):
    """``ensemble_products`` as torch ops on the tensors' device by the same definitions: the members widened to float64, the sum
    in member order, the two-pass deviation, a ``sort`` over the member axis and its planes for the order statistics, counts
    compared in fp32, every value rounded once to fp32, then ``* scale + shift`` as two fp32 operations.  ``idx``: the selected
    channels (int64 tensor) or None; ``out`` ``[B, K, Cs, H, W]`` is written in place, chunk of channels by chunk so that a
    temporary holds at most ``_ENS_TORCH_CHUNK`` elements."""
    B, E, C, H, W = ens.shape
    Cs = out.shape[2]
    nan = torch.full((), float("nan"), dtype=torch.float32, device=ens.device)
    # divisors as tensors: torch divides by a python scalar on the device as a multiplication by its reciprocal, which is not
    # the division of the definition (E equal members must give m = x, a count over E the IEEE quotient)
    n64, nm1, n32 = (torch.full((), v, dtype=t, device=ens.device) for v, t in ((E, torch.float64), (E - 1, torch.float64), (E, torch.float32)))
    need_std, need_sort = bool((kinds == 1).any()), bool((kinds == 2).any())
    step = max(1, _ENS_TORCH_CHUNK // max(1, B * E * H * W))
    for c0 in range(0, Cs, step):
        sel = slice(c0, min(Cs, c0 + step))
        x32 = (ens[:, :, sel] if idx is None else ens.index_select(2, idx[sel])).float()
        x = x32.double()
        bad = torch.isnan(x32).any(dim=1)
        sm = x[:, 0].clone()
        for e in range(1, E):
            sm += x[:, e]
        m = sm / n64
        if need_std:
            sv = torch.zeros_like(m)
            for e in range(E):
                d = x[:, e] - m
                sv += d * d
            sd = torch.sqrt(sv / nm1) if E > 1 else torch.full_like(m, float("nan"))
        if need_sort:
            xs = torch.sort(x32, dim=1).values
        for i, kind in enumerate(kinds.tolist()):
            if kind == 0:
                v = m.float()
            elif kind == 1:
                v = sd.float()
            elif kind == 2:
                k, t = int(orders[i]), float(fracs[i])
                v = xs[:, k]
                if t != 0.0:
                    a, b = xs[:, k].double(), xs[:, k + 1].double()
                    v = (a + t * (b - a)).float()
            else:
                th = thr[i, sel].reshape(1, -1, 1, 1)
                cnt = ((x32 > th.unsqueeze(1)) if kind == 3 else (x32 < th.unsqueeze(1))).sum(dim=1)
                v = torch.where(torch.isnan(th), nan, cnt.float() / n32)
            if scale is not None and kind <= 2:
                v = v * scale[sel].reshape(1, -1, 1, 1)
                if kind != 1:
                    v = v + shift[sel].reshape(1, -1, 1, 1)
            out[:, i, sel] = torch.where(bad, nan, v)
    return out


def _ens_products_launch(ens, kinds, orders, fracs, chans, thr, scale, shift, out):
    """One ``mk_ens_products`` launch: fp32 / bf16 members ``[B, E, C, H, W]`` read in place where every member's ``[C, H, W]``
    block is contiguous (else the ensemble is copied), ``out`` ``[B, K, Cs, H, W]`` fp32 / bf16 written through its strides."""
    B, E, C, H, W = ens.shape
    K, Cs = out.shape[1], out.shape[2]
    if ens.stride()[2:] != (H * W, W, 1) or min(ens.stride(0), ens.stride(1)) < C * H * W:
        ens = ens.contiguous()
    bstride = ens.stride(0) if B > 1 else E * ens.stride(1)      # a stride of a size-1 axis means nothing
    okstride = out.stride(1) if K > 1 else Cs * H * W
    obstride = out.stride(0) if B > 1 else K * okstride
    _lib.check(_lib.load().mk_ens_products(ens.data_ptr(), _pw_dtype(ens), bstride, ens.stride(1), out.data_ptr(), _pw_dtype(out),
                                           obstride, okstride, _ptr(chans), kinds.ctypes.data, orders.ctypes.data, fracs.ctypes.data,
                                           _ptr(thr), _ptr(scale), _ptr(shift), B, E, C, Cs, K, H, W, _stream()), "mk_ens_products")
    return out


@torch.no_grad()
def ensemble_products(ens, kinds, orders, fracs, chans=None, thr=None, scale=None, shift=None, out=None, out_dtype=torch.float32):
    """Forecast products of an ensemble ``ens`` ``[B, E, C, H, W]``: ``[B, K, Cs, H, W]`` of ``out_dtype``, one plane per product
    and selected channel.  A ``[B * E, C, H, W]`` model output is passed pre-viewed, ``x.view(B, E, C, H, W)`` (member fastest);
    there is no ``members=`` argument.

    ``kinds`` (names of ``ENS_PRODUCT_KINDS`` or their positions), ``orders`` and ``fracs`` are sequences of length K, at most
    ``ENS_PRODUCTS_MAX`` on the HIP pass.  Per point, with the members ``x_e`` widened to float64:

    * ``mean``: ``m = (sum_e x_e) / E``, summed in member order;
    * ``std``: ``sqrt(sum_e (x_e - m)^2 / (E - 1))``, two-pass about ``m`` (NaN for ``E = 1``);
    * ``order``: ``x_(k) + t (x_(k+1) - x_(k))`` over the members sorted ascending, ``k = orders[i]`` from 0, ``t = fracs[i]`` in
      [0, 1); with ``t == 0`` the member of rank k itself (``k = E - 1`` is legal only then).  ``quantile_position`` gives the
      pair of a quantile; min is ``(0, 0.0)``, max ``(E - 1, 0.0)``;
    * ``above`` / ``below``: ``#{e : x_e > thr[i, j]} / E`` and ``#{e : x_e < thr[i, j]} / E``, compared in fp32, a tie counts
      for neither; ``thr`` is an fp32 ``[K, Cs]`` tensor read for these kinds only, a NaN threshold gives a NaN plane.

    ``chans`` selects and orders the channels (a list, checked against C, or a 1-D integer tensor on the device, taken as it
    is: on the HIP pass an entry outside ``[0, C)`` gives NaN planes); repeats are allowed, None is all C.  The first three
    kinds are rounded once to fp32; ``scale`` and ``shift`` ``[Cs]`` (both or neither) then give ``v * scale[j] + shift[j]`` in
    fp32 as ``rollout_tail`` applies its emit statistics -- ``std`` is multiplied only, the counts are never scaled.  A bf16
    result is the fp32 one rounded to nearest even.  A point with a NaN member is NaN in all K planes; infinite members are out
    of contract.  ``out``, where given, is written and returned: any ``[B, K, Cs, H, W]`` view whose ``[Cs, H, W]`` blocks are
    contiguous and do not overlap, such as a slice of a larger buffer; what lies between the blocks keeps its bytes.

    ``MK_ENS_PRODUCTS=hip`` (read on every call): CUDA fp32 / bf16 members with 2 to ``ENSEMBLE_MAX_MEMBERS`` members, at most
    ``ENS_PRODUCTS_MAX`` products and an fp32 / bf16 result take one ``mk_ens_products`` launch (members read in place through
    their strides, no atomics, no workspace, the same bits every run, capturable).  CPU tensors, ``E = 1``, more members or
    products, other dtypes and ``MK_ENS_PRODUCTS=torch`` take ``_ensemble_products_torch``.  No gradient flows through this op."""
    hip = _hip_or_torch("MK_ENS_PRODUCTS", ENS_PRODUCTS_DEFAULT)
    if ens.dim() != 5 or min(ens.shape) < 1:
        raise ValueError(f"ensemble_products: the ensemble must be [B, E, C, H, W], got {tuple(ens.shape)}")
    B, E, C, H, W = ens.shape
    dev = ens.device
    kinds, orders, fracs = _ens_product_table(kinds, orders, fracs, E)
    K = len(kinds)
    idx = None
    if chans is not None:
        if not torch.is_tensor(chans):
            chans = [int(c) for c in chans]
            if not chans or min(chans) < 0 or max(chans) >= C:
                raise ValueError(f"ensemble_products: chans {chans} out of range for {C} channels")
            chans = torch.tensor(chans, dtype=torch.int32, device=dev)
        if chans.dim() != 1 or chans.numel() < 1 or chans.device != dev or chans.dtype.is_floating_point:
            raise ValueError(f"ensemble_products: chans must be a 1-D integer tensor on {dev}, got {chans.dtype} {tuple(chans.shape)} "
                             f"on {chans.device}")
    Cs = C if chans is None else chans.numel()
    if bool(((kinds == 3) | (kinds == 4)).any()):
        if thr is None or tuple(thr.shape) != (K, Cs) or thr.device != dev:
            raise ValueError(f"ensemble_products: a count product needs thr [K, Cs] = [{K}, {Cs}] on {dev}")
    if (scale is None) != (shift is None):
        raise ValueError("ensemble_products: scale and shift come together or not at all")
    for name, t in (("scale", scale), ("shift", shift)):
        if t is not None and (t.numel() != Cs or t.device != dev):
            raise ValueError(f"ensemble_products: {name} {tuple(t.shape)} on {t.device} needs Cs = {Cs} elements on {dev}")
    thr, scale, shift = _f32(thr), _f32(None if scale is None else scale.reshape(-1)), _f32(None if shift is None else shift.reshape(-1))
    if out is None:
        out = torch.empty(B, K, Cs, H, W, dtype=out_dtype, device=dev)
    elif tuple(out.shape) != (B, K, Cs, H, W) or out.device != dev:
        raise ValueError(f"ensemble_products: out {tuple(out.shape)} on {out.device} must be {[B, K, Cs, H, W]} on {dev}")
    ens = ens.detach()
    if not (hip and ens.is_cuda and 2 <= E <= ENSEMBLE_MAX_MEMBERS and K <= ENS_PRODUCTS_MAX and ens.dtype in _LOWP
            and out.dtype in _LOWP):
        return _ensemble_products_torch(ens, kinds, orders, fracs, None if chans is None else chans.long(), thr, scale, shift, out)
    chw = Cs * H * W
    so = out.stride()
    if (so[2:] != (H * W, W, 1) or (K > 1 and so[1] < chw) or (B > 1 and so[0] < chw)
            or (B > 1 and K > 1 and so[0] < K * so[1] and so[1] < B * so[0])):
        raise ValueError(f"ensemble_products: out with strides {tuple(so)} is not [B, K] separate contiguous [Cs, H, W] blocks")
    if chans is not None:
        chans = chans.to(torch.int32).contiguous()
    return _ens_products_launch(ens, kinds, orders, fracs, chans, thr, scale, shift, out)


# ----------------------------------------------------------------------------
# the ensemble CRPS as a training loss (csrc/ens.hip: mk_ens_sums forward, mk_ens_crps_bwd backward)
# ----------------------------------------------------------------------------
ENS_LOSS_DEFAULT = "hip"        # MK_ENS_LOSS: hip | torch.  No row of tools/ens_loss_bench.py is slower than torch
ENS_LOSS_MAX_MEMBERS = 16       # what mk_ens_crps_bwd takes: a thread compares all pairs of its point's members in registers


def _walk_chunks(fn, pieces, n, step, needs_grad, dim):
    """``fn(*pieces(s))`` for the slices ``s`` of ``step`` out of ``n``, concatenated along ``dim``.  Under autograd, with more than
    one slice, a slice is recomputed in the backward instead of kept (``torch.utils.checkpoint``)."""
    keep = torch.is_grad_enabled() and needs_grad
    out = []
    for i0 in range(0, n, step):
        args = pieces(slice(i0, i0 + step))
        if keep and step < n:
            from torch.utils.checkpoint import checkpoint
            out.append(checkpoint(fn, *args, use_reentrant=False))
        else:
            out.append(fn(*args))
    return torch.cat(out, dim=dim)


def _ens_crps_chunk(x, y, w):
    """``[B, c, 4]`` float64 of a channel chunk, ``x`` ``[B, E, c, H, W]``: a and g from ALL PAIRS, differentiable; q and v
    detached, NaN where the point is.

    ``sum_ef |x_e - x_f|`` is written as ``2 sum_e (x_e - y) r_e`` with ``r_e = sum_f sgn(x_e - x_f) = L_e - G_e`` summed as integers
    and detached (``sum_e r_e = 0``, so the target drops out; it only keeps the terms small).  The value and the gradient are those
    of ``abs`` under autograd, ``abs'(0) = 0`` included, but the backward multiplies the upstream gradient u by ``r_e`` ONCE: it is
    exactly zero where ``L_e = G_e``.  The backward of the plain ``abs`` adds E terms ``+-u`` per member, and those sums round
    (3 u is not a float64 number), which leaves 1e-17 where the definition has zero from E = 5 on."""
    E = x.shape[1]
    x, y = x.double(), y.double()
    d = x - y.unsqueeze(1)
    a = d.abs().sum(dim=1) / E
    with torch.no_grad():
        r = torch.sign(x.unsqueeze(1) - x.unsqueeze(2)).sum(dim=1)          # [b, f, e] = x_e - x_f, summed over f
    g = ((x - y.detach().unsqueeze(1)) * r).sum(dim=1) * (2.0 / (E * E))
    with torch.no_grad():
        m = x.sum(dim=1) / E
        q = (m - y) ** 2
        v = ((x - m.unsqueeze(1)) ** 2).sum(dim=1) / (E - 1) if E > 1 else torch.full_like(m, float("nan"))
        # 1 at a good point, NaN where the target or a member is NaN.  As a factor it makes all four values of such a point NaN
        # and, in the backward, the gradient of EVERY member of the point (torch's abs' is sgn, and sgn(NaN) is 0: without the
        # factor a NaN point would hand its members zeros and finite values)
        mark = 1.0 + 0.0 * (y + x.sum(dim=1))
        q, v = q * mark, v * mark
    a, g = a * mark, g * mark
    return torch.stack([(w * f).sum(dim=(-2, -1)) for f in (a, g, q, v)], dim=-1)


def _ensemble_crps_sums_torch(ens, tar, wrow):
    """``[B, C, 4]`` float64 in the order of ``ENSEMBLE_SUMS`` on the tensors' device (``ens`` ``[B, E, C, H, W]``); the first two,
    ``a`` and ``g``, are the all-pairs expression under ordinary autograd (``abs'(0) = 0``: tied members get equal gradients; see
    ``_ens_crps_chunk`` for how the pairs are written), the other two are detached.  The channels are walked in chunks so that an ``E^2`` temporary holds at most ``_ENS_TORCH_CHUNK``
    elements; under autograd a chunk is recomputed in the backward instead of kept (``torch.utils.checkpoint``)."""
    B, E, C, H, W = ens.shape
    w = wrow.detach().double().reshape(1, 1, H, 1)
    step = max(1, _ENS_TORCH_CHUNK // max(1, B * E * E * H * W))
    return _walk_chunks(_ens_crps_chunk, lambda s: (ens[:, :, s], tar[:, s], w), C, step, ens.requires_grad or tar.requires_grad, 1)


class _EnsCrpsSums(torch.autograd.Function):
    """([B, C, 2] float64 (sum w a, sum w g), the detached [B, C, 4] of the same pass); mk_ens_sums forward, mk_ens_crps_bwd backward."""

    @staticmethod
    def forward(ctx, ens, tar, wrow):
        out, ens, ctx.bstride = _ens_sums_launch(ens, tar, wrow)
        # ``ens`` is what the kernel read: the argument, or its contiguous copy where the strides did not fit (made in here, not
        # by the caller; the gradient is contiguous with the argument's shape either way)
        ctx.save_for_backward(ens, tar, wrow)
        ctx.mark_non_differentiable(out)
        return out[..., :2].contiguous(), out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _):
        ens, tar, wrow = ctx.saved_tensors
        B, E, C, H, W = ens.shape
        gens = torch.empty(ens.shape, dtype=ens.dtype, device=ens.device)
        g = g.double().contiguous()
        _lib.check(_lib.load().mk_ens_crps_bwd(ens.data_ptr(), _pw_dtype(ens), ctx.bstride, ens.stride(1), tar.data_ptr(),
                                               wrow.data_ptr(), g.data_ptr(), gens.data_ptr(), E * C * H * W, C * H * W,
                                               B, E, C, H, W, _stream()), "mk_ens_crps_bwd")
        return gens, None, None


def ensemble_crps_sums(ens, tar, wrow, with_sums=False):
    """The two latitude-weighted integrals the ensemble CRPS losses are made of, ``[B, C, 2]`` float64, differentiable in the
    members: ``S[b, c] = (sum_hw w a, sum_hw w g)`` with ``a = mean_e |x_e - y|``, ``g = mean_ef |x_e - x_f|`` over all E^2 pairs
    and ``w = wrow[h]``, of an ensemble ``ens`` ``[B, E, C, H, W]`` (a ``[B * E, C, H, W]`` model output is viewed, member fastest)
    against a target ``tar`` ``[B, C, H, W]``.  The loss of a point is ``a - (kappa / 2) g``: ``kappa = 1`` the CRPS,
    ``kappa = E / (E - 1)`` the fair CRPS.  The gradient is that of the all-pairs expression,

        ``d/dx_e = w (gS0 sgn(x_e - y) / E + gS1 2 (L_e - G_e) / E^2)``,   ``L_e, G_e`` the members below and above ``x_e``,

    equal among tied members; a point whose target or one of whose members is NaN gives NaN to every member of that point and
    to the sums of its ``(b, c)``.  ``with_sums=True`` returns ``(S, sums)`` with the detached ``[B, C, 4]`` in the order of
    ``ENSEMBLE_SUMS`` from the same pass (spread and ensemble-mean error for a training log).

    ``MK_ENS_LOSS=hip`` (read on every call): CUDA fp32 / bf16 members, 2 to ``ENS_LOSS_MAX_MEMBERS`` of them, take
    ``mk_ens_sums`` forward and one ``mk_ens_crps_bwd`` launch backward, which writes a contiguous gradient in the members' dtype
    (the members are read in place through their batch and member strides; the same bits every run, capturable).  CPU tensors,
    ``E = 1``, more members, other dtypes, a target that requires a gradient and ``MK_ENS_LOSS=torch`` take
    ``_ensemble_crps_sums_torch``."""
    hip = _hip_or_torch("MK_ENS_LOSS", ENS_LOSS_DEFAULT)
    ens = _ensemble_operands("ensemble_crps_sums", ens, tar, wrow)
    if not (hip and ens.is_cuda and 2 <= ens.shape[1] <= ENS_LOSS_MAX_MEMBERS and ens.dtype in _LOWP and not tar.requires_grad):
        out = _ensemble_crps_sums_torch(ens, tar, wrow)
        s, sums = out[..., :2], out.detach()
    else:
        s, sums = _EnsCrpsSums.apply(ens, tar.detach().float().contiguous(), wrow.detach().float().contiguous())
    return (s, sums) if with_sums else s


# ----------------------------------------------------------------------------
# the spectral ensemble CRPS (csrc/spec_crps.hip: mk_spec_crps_sums forward, mk_spec_crps_bwd backward)
# ----------------------------------------------------------------------------
SPEC_CRPS_DEFAULT = "hip"       # MK_SPEC_CRPS: hip | torch.  No row of tools/spec_crps_bench.py is slower than torch
SPEC_CRPS_MAX_MEMBERS = 16      # what the kernels take: a thread holds the members of its coefficient in registers


def _spec_crps_chunk(x, y, w):
    """``[l, B, C, 2]`` float64 of a slice of degrees: ``x`` ``[l, M, B, E, C, 2]`` and ``y`` ``[l, M, B, C, 2]`` the (re, im)
    components with the unstored triangle already set to zero, ``w`` ``[l, M]`` float64 the order weights (zero there).

    As in ``_ens_crps_chunk``, ``sum_ef |x_e - x_f|`` is written as ``2 sum_e (x_e - c) r_e`` with ``r_e = L_e - G_e`` summed as
    integers and detached, so the backward multiplies the upstream gradient by ``r_e`` once: equal among tied members and
    exactly zero where ``L_e = G_e``.  ``sum_e r_e = 0``, so any constant ``c`` drops out; the detached member mean keeps
    ``sum_e |x_e - c| |r_e|`` below ``sum_ef |x_e - x_f|``."""
    E = x.shape[3]
    x, y = x.double(), y.double()
    a = (x - y.unsqueeze(3)).abs().sum(dim=3) / E
    with torch.no_grad():
        r = torch.sign(x.unsqueeze(3) - x.unsqueeze(4)).sum(dim=3)          # [l, M, B, f, e, C, 2] = x_e - x_f, summed over f
        c = x.sum(dim=3, keepdim=True) / E
        # 1 at a good coefficient, NaN where a component of the target or of a member is: both terms and, in the backward,
        # both components of every member's gradient become NaN there (sgn(NaN) is 0 in torch's abs')
        mark = (1.0 + 0.0 * (y.sum(dim=-1) + x.sum(dim=(3, -1)))).unsqueeze(-1)
    g = ((x - c) * r).sum(dim=3) * (2.0 / (E * E))
    w = w.reshape(w.shape + (1, 1))
    return torch.stack([(w * (f * mark).sum(dim=-1)).sum(dim=1) for f in (a, g)], dim=-1)


def _spectral_crps_sums_torch(cp, ct, members, l_off=0, m_off=0, batch=1):
    """``spectral_crps_sums`` in torch float64 on the tensors' device under ordinary autograd: the all-pairs expression (see
    ``_spec_crps_chunk`` for how the pairs are written), over the stored triangle only -- the rows with
    ``l_off + l < m_off + m`` are replaced by zeros before any arithmetic and get zero gradients.  The degrees are walked in
    slices so that an ``E^2`` temporary holds at most ``_ENS_TORCH_CHUNK`` elements; under autograd a slice is recomputed in the
    backward instead of kept (``torch.utils.checkpoint``)."""
    L, M, BC = ct.shape
    E, B = int(members), int(batch)
    C = BC // B
    stored, w = _stored_triangle(L, M, l_off, m_off, cp.device)
    x = torch.view_as_real(cp).reshape(L, M, B, E, C, 2)
    y = torch.view_as_real(ct).reshape(L, M, B, C, 2)
    x = torch.where(stored.reshape(L, M, 1, 1, 1, 1), x, torch.zeros_like(x))
    y = torch.where(stored.reshape(L, M, 1, 1, 1), y, torch.zeros_like(y))
    step = max(1, _ENS_TORCH_CHUNK // max(1, 2 * M * B * E * E * C))
    out = _walk_chunks(_spec_crps_chunk, lambda s: (x[s], y[s], w[s]), L, step, cp.requires_grad or ct.requires_grad, 0)
    return out.permute(1, 2, 0, 3).reshape(BC, L, 2)


class _SpecCrpsSums(torch.autograd.Function):
    """[BC, L, 2] float64 of packed spectra cp [L, M, B E C] and ct [L, M, BC]; mk_spec_crps_sums forward, mk_spec_crps_bwd backward."""

    @staticmethod
    def forward(ctx, cp, ct, B, E, C, l_off, m_off):
        L, M, BC = ct.shape
        lib = _lib.load()
        ws = torch.empty(lib.mk_spec_crps_workspace(L, M, BC), dtype=torch.float64, device=cp.device)
        out = torch.empty(L, BC, 2, dtype=torch.float64, device=cp.device)
        _lib.check(lib.mk_spec_crps_sums(cp.data_ptr(), ct.data_ptr(), ws.data_ptr(), out.data_ptr(), L, M, B, E, C, l_off, m_off,
                                         _stream()), "mk_spec_crps_sums")
        ctx.save_for_backward(cp, ct)
        ctx.dims = (B, E, C, l_off, m_off)
        return out.permute(1, 0, 2)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        cp, ct = ctx.saved_tensors
        L, M, _ = ct.shape
        gs = g.permute(1, 0, 2).to(torch.float64).contiguous()      # [L, BC, 2], as the kernel wrote S
        gcp = torch.empty_like(cp)
        _lib.check(_lib.load().mk_spec_crps_bwd(cp.data_ptr(), ct.data_ptr(), gs.data_ptr(), gcp.data_ptr(), L, M, *ctx.dims,
                                                _stream()), "mk_spec_crps_bwd")
        return gcp, None, None, None, None, None, None


def spectral_crps_sums(cp, ct, members, l_off=0, m_off=0, batch=1):
    """The per-degree sums the spectral ensemble CRPS is made of, ``[B C, L, 2]`` float64, differentiable in the members' spectra.
    ``cp`` is the packed spectrum ``[L, M, B E C]`` complex64 of the predictions (row ``(b E + e) C + c``: ``forward_packed`` of
    ``[B E, C, H, W]``, member fastest), ``ct`` ``[L, M, B C]`` that of the target, ``members`` = E and ``batch`` = B (the rows
    alone do not say how they split into samples and channels).  For every stored coefficient (``l_off + l >= m_off + m``), each
    component ``k`` of it taken as a real number, ``a_k = mean_e |x_e - y|`` and ``g_k = mean_ef |x_e - x_f|`` over all E^2 pairs,

        ``S[bc, l, 0] = sum_m w (a_re + a_im)``,   ``S[bc, l, 1] = sum_m w (g_re + g_im)``,   ``w(0) = 1``, ``w(m > 0) = 2``.

    The rows the Legendre kernels leave unwritten are never read.  The sums concatenate over ``l`` shards and add up over ``m``
    shards, as ``degree_power``'s do.  The gradient is that of the all-pairs expression, per component
    ``w (gS0 sgn(x_e - y) / E + gS1 2 (L_e - G_e) / E^2)`` in torch's complex convention: equal among tied members, exactly zero
    for the zero imaginary parts of ``m = 0`` and in the unstored triangle.  A NaN component of a member or the target makes the
    gradients of that coefficient's members and the sums of its ``(b, c, l)`` NaN.

    ``MK_SPEC_CRPS=hip`` (read on every call): CUDA tensors with 2 to ``SPEC_CRPS_MAX_MEMBERS`` members take ``mk_spec_crps_sums``
    (a streaming pass and a fixed-order finalize: the same bits every run, capturable) and one ``mk_spec_crps_bwd`` launch
    backward; no gradient flows to the target there.  CPU tensors, ``E = 1``, more members, a target that requires a gradient
    and ``MK_SPEC_CRPS=torch`` take ``_spectral_crps_sums_torch``."""
    hip = _hip_or_torch("MK_SPEC_CRPS", SPEC_CRPS_DEFAULT)
    E, B, l_off, m_off = int(members), int(batch), int(l_off), int(m_off)
    for name, t in (("cp", cp), ("ct", ct)):
        if t.dim() != 3 or t.dtype != torch.complex64 or min(t.shape) < 1:
            raise ValueError(f"spectral_crps_sums: {name} must be a non-empty complex64 spectrum [L, M, rows], got {t.dtype} {tuple(t.shape)}")
    if E < 1 or B < 1 or ct.shape[2] % B or tuple(cp.shape) != (ct.shape[0], ct.shape[1], E * ct.shape[2]):
        raise ValueError(f"spectral_crps_sums: {tuple(cp.shape)} is not the spectrum of {E} members of a target {tuple(ct.shape)} "
                         f"of {B} samples")
    if l_off < 0 or m_off < 0:
        raise ValueError(f"spectral_crps_sums: offsets must not be negative, got l_off={l_off}, m_off={m_off}")
    if cp.device != ct.device:
        raise ValueError(f"spectral_crps_sums: predictions on {cp.device}, target on {ct.device}")
    if not (hip and cp.is_cuda and 2 <= E <= SPEC_CRPS_MAX_MEMBERS and not ct.requires_grad):
        return _spectral_crps_sums_torch(cp, ct, E, l_off, m_off, B)
    return _SpecCrpsSums.apply(cp.contiguous(), ct.detach().contiguous(), B, E, ct.shape[2] // B, l_off, m_off)


# ----------------------------------------------------------------------------
# latitude interpolation (csrc/grid.hip: mk_lat_lerp_fwd forward, mk_lat_lerp_bwd backward): the arithmetic of grids.GridConverter
# ----------------------------------------------------------------------------
GRID_DEFAULT = "hip"            # MK_GRID: hip | torch.  No row of tools/grid_bench.py is slower than torch


class LatInterpTables:
    """What ``lat_interp`` reads, on one device: ``idx`` int32 ``[Hd]`` local source rows, ``wgt`` fp32 ``[Hd]``, the CSR transpose
    (``rowptr`` int32 ``[Hs + 1]``, ``term_row`` int32 and ``term_coef`` fp32 ``[2 Hd]``: per source row its terms by ascending
    destination row, ``1 - w`` for the a-term and ``w`` for the b-term, each rounded once from float64 to fp32), and for the torch formulation ``index``
    int64 ``[Hd]`` and ``weights`` float64 ``[Hd, 1]``.  ``n_src_rows`` = Hs, ``n_dst_rows`` = Hd."""

    def __init__(self, local, weights64, n_src_rows, device):
        hd = local.shape[0]
        w32 = weights64.astype(np.float32)
        rows = np.stack([local, local + 1], axis=1).reshape(-1)
        # 1 - w from the float64 weight, rounded once: fl(1 - fl(w)) carries the rounding of w as an ABSOLUTE error, which is
        # not small against 1 - w where w is close to 1 (the rows next to the equator)
        coef = np.stack([(1.0 - weights64).astype(np.float32), w32], axis=1).reshape(-1)
        order = np.argsort(rows, kind="stable")              # by source row; within one, ascending k (and a before b)
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n_src_rows))])
        dev = torch.device(device)
        self.n_src_rows, self.n_dst_rows, self.device = int(n_src_rows), int(hd), dev
        self.idx = torch.from_numpy(local.astype(np.int32)).to(dev)
        self.wgt = torch.from_numpy(w32).to(dev)
        self.rowptr = torch.from_numpy(rowptr.astype(np.int32)).to(dev)
        self.term_row = torch.from_numpy((np.repeat(np.arange(hd), 2)[order]).astype(np.int32)).to(dev)
        self.term_coef = torch.from_numpy(coef[order].astype(np.float32)).to(dev)
        self.index = torch.from_numpy(local.astype(np.int64)).to(dev)
        self.weights = torch.from_numpy(weights64.astype(np.float64).reshape(-1, 1)).to(dev)


def lat_interp_tables(indices, weights, n_src_rows, src_row0=0, device="cpu"):
    """The tables of ``lat_interp`` for the destination rows whose GLOBAL source rows are ``indices`` (integers) with ``weights``
    (float64; any finite value: outside [0, 1] extrapolates) -- a whole table or any slice of one -- on a slab of ``n_src_rows``
    source rows that starts at global row ``src_row0``.  Every pair must lie in the slab: ``src_row0 <= i`` and
    ``i + 1 < src_row0 + n_src_rows``, else ``ValueError``.  The contents are checked here, once, and not by the kernels."""
    i = np.asarray(indices.detach().cpu() if torch.is_tensor(indices) else indices).astype(np.int64).reshape(-1)
    w = np.asarray(weights.detach().cpu() if torch.is_tensor(weights) else weights, dtype=np.float64).reshape(-1)
    n_src_rows, src_row0 = int(n_src_rows), int(src_row0)
    if i.shape[0] < 1 or i.shape != w.shape:
        raise ValueError(f"lat_interp_tables: {i.shape[0]} indices and {w.shape[0]} weights (need as many, at least one)")
    if n_src_rows < 2:
        raise ValueError(f"lat_interp_tables: {n_src_rows} source rows (a destination row blends two)")
    if not np.isfinite(w).all():
        raise ValueError("lat_interp_tables: a weight is not finite")
    if (i < src_row0).any() or (i + 1 >= src_row0 + n_src_rows).any():
        raise ValueError(f"lat_interp_tables: source rows {int(i.min())} ... {int(i.max()) + 1} leave the slab "
                         f"[{src_row0}, {src_row0 + n_src_rows})")
    return LatInterpTables(i - src_row0, w, n_src_rows, device)


def _lat_interp_torch(x, tables, bias=None, scale=None):
    """The reference's expression (``makani/utils/grids.py``: ``GridConverter.forward`` after the loader's ``(x - bias) / scale``):
    ``torch.lerp(x[..., i, :], x[..., i + 1, :], w.to(x.dtype))``, ``bias`` / ``scale`` broadcast over the channel axis.  A bf16
    input is widened to fp32 and blended with the fp32 weights (the result is fp32; the caller rounds it once)."""
    if x.dtype == torch.bfloat16:
        x = x.float()
    if bias is not None:
        x = (x - bias.to(x.dtype).reshape(-1, 1, 1)) / scale.to(x.dtype).reshape(-1, 1, 1)
    i = tables.index
    return torch.lerp(x[..., i, :], x[..., i + 1, :], tables.weights.to(dtype=x.dtype))


def _row_contiguous(t):
    H, W = t.shape[-2:]
    return (W == 1 or t.stride(-1) == 1) and (H == 1 or t.stride(-2) >= W)


def _plane_groups(a, b):
    """``a`` ``[..., Ha, W]`` and ``b`` ``[..., Hb, W]`` with the same leading shape, as launches: the trailing leading axes that have ONE
    plane stride in both tensors form the planes of a launch (always at least the last, the channel axis), the axes in front
    are walked on the host.  Yields ``(address of a, address of b, P, plane stride of a, of b)``."""
    if a.dim() == 2:
        a, b = a.unsqueeze(0), b.unsqueeze(0)
    lead = tuple(a.shape[:-2])
    m = len(lead) - 1

    def planes(t, q):
        try:
            return t.view(*lead[:q], -1, *t.shape[-2:])
        except RuntimeError:
            return None

    for q in range(m + 1):
        va, vb = planes(a, q), planes(b, q)
        if va is not None and vb is not None:
            break
    P = va.shape[q]
    for outer in np.ndindex(*lead[:q]):
        oa = sum(int(o) * va.stride(d) for d, o in enumerate(outer))
        ob = sum(int(o) * vb.stride(d) for d, o in enumerate(outer))
        yield (a.data_ptr() + oa * a.element_size(), b.data_ptr() + ob * b.element_size(), P, va.stride(q), vb.stride(q))


def _lat_lerp_fwd_raw(x, tables, bias, scale, out):
    """``mk_lat_lerp_fwd`` of ``x`` ``[..., Hs, W]`` into ``out`` ``[..., Hd, W]`` (both row contiguous, any other strides)."""
    lib = _lib.load()
    W, C = x.shape[-1], (x.shape[-3] if x.dim() >= 3 else 1)
    for px, py, P, sx, sy in _plane_groups(x, out):
        _lib.check(lib.mk_lat_lerp_fwd(px, _pw_dtype(x), sx, x.stride(-2), py, _pw_dtype(out), sy, max(out.stride(-2), W),
                                       tables.idx.data_ptr(), tables.wgt.data_ptr(), _ptr(bias), _ptr(scale), C, P,
                                       tables.n_src_rows, tables.n_dst_rows, W, _stream()), "mk_lat_lerp_fwd")
    return out


class _LatInterp(torch.autograd.Function):
    """``mk_lat_lerp_fwd`` forward, ``mk_lat_lerp_bwd`` backward; no gradient to the tables, ``bias`` or ``scale``."""

    @staticmethod
    def forward(ctx, x, tables, bias, scale, out, out_dtype):
        if out is None:
            out = torch.empty(*x.shape[:-2], tables.n_dst_rows, x.shape[-1], dtype=out_dtype, device=x.device)
        else:
            ctx.mark_dirty(out)
        ctx.tables, ctx.scale, ctx.x_shape, ctx.x_dtype = tables, scale, x.shape, x.dtype
        return _lat_lerp_fwd_raw(x, tables, bias, scale, out)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        tables, scale = ctx.tables, ctx.scale
        gy = _lowp(gy)
        if not _row_contiguous(gy):
            gy = gy.contiguous()
        gx = torch.empty(ctx.x_shape, dtype=ctx.x_dtype, device=gy.device)
        lib = _lib.load()
        W, C = gx.shape[-1], (gx.shape[-3] if gx.dim() >= 3 else 1)
        for pg, px, P, sg, sx in _plane_groups(gy, gx):
            _lib.check(lib.mk_lat_lerp_bwd(pg, _pw_dtype(gy), sg, max(gy.stride(-2), W), px, _pw_dtype(gx), sx, W,
                                           tables.rowptr.data_ptr(), tables.term_row.data_ptr(), tables.term_coef.data_ptr(),
                                           _ptr(scale), C, P, tables.n_src_rows, tables.n_dst_rows, W, _stream()), "mk_lat_lerp_bwd")
        return gx, None, None, None, None, None


def lat_interp(x, tables, bias=None, scale=None, out=None, out_dtype=None):
    """Interpolation along latitude: ``y[..., k, :] = lerp(x'[..., i_k, :], x'[..., i_k + 1, :], w_k)`` for ``x`` ``[..., Hs, W]`` and the
    ``tables`` of ``lat_interp_tables`` (``Hs`` source rows, ``Hd`` destination rows, on ``x``'s device), with ``x' = x`` or, given
    ``bias`` and ``scale`` (both, ``C`` elements each, e.g. the ``[1, C, 1, 1]`` statistics files; ``C`` the last leading axis of
    ``x``), ``x' = (x - bias[c]) / scale[c]`` -- the loader's fp32 expression, a subtraction and an IEEE division.  ``out``, if
    given, is ``[..., Hd, W]`` with contiguous rows and any other strides (a channel slice of a larger buffer); ``out_dtype``
    (default: ``out``'s, else ``x``'s) may be fp32 or bf16 for either input.  Differentiable in ``x`` only.

    ``MK_GRID=hip`` (read on every call): CUDA fp32 / bf16 tensors take one ``mk_lat_lerp_fwd`` launch per run of planes with a
    single stride (one for a contiguous tensor), and one ``mk_lat_lerp_bwd`` launch backward: each source row read once per
    band of rows, each destination row written once, the same bits every run, capturable.  CPU tensors, float64 and
    ``MK_GRID=torch`` take ``_lat_interp_torch``, for fp32 the reference's ``torch.lerp`` expression exactly.  Deviation: for
    bf16 data the reference would round the weights to bf16 and blend in bf16; both paths here widen the data to fp32, blend
    with the fp32 weights and round the result once."""
    hip = _hip_or_torch("MK_GRID", GRID_DEFAULT)
    if not isinstance(tables, LatInterpTables):
        raise TypeError("lat_interp: tables must come from lat_interp_tables")
    if x.dim() < 2 or x.shape[-2] != tables.n_src_rows:
        raise ValueError(f"lat_interp: input {tuple(x.shape)} must be [..., {tables.n_src_rows}, W]")
    if x.device != tables.device:
        raise ValueError(f"lat_interp: input on {x.device}, tables on {tables.device}")
    if (bias is None) != (scale is None):
        raise ValueError("lat_interp: bias and scale come together")
    C = x.shape[-3] if x.dim() >= 3 else 1
    if bias is not None and (bias.numel() != C or scale.numel() != C):
        raise ValueError(f"lat_interp: bias / scale with {bias.numel()} / {scale.numel()} elements for {C} channels")
    shape = (*x.shape[:-2], tables.n_dst_rows, x.shape[-1])
    if out is not None:
        if tuple(out.shape) != shape or out.device != x.device or not _row_contiguous(out):
            raise ValueError(f"lat_interp: out {tuple(out.shape)} on {out.device} must be {shape} on {x.device} with contiguous rows")
        if out_dtype is not None and out_dtype != out.dtype:
            raise ValueError(f"lat_interp: out is {out.dtype}, out_dtype {out_dtype}")
        out_dtype = out.dtype
    elif out_dtype is None:
        out_dtype = x.dtype
    if not (hip and x.is_cuda and x.dtype in _LOWP and out_dtype in _LOWP) or x.numel() == 0:
        y = _lat_interp_torch(x, tables, bias, scale).to(out_dtype)
        return y if out is None else out.copy_(y)
    if not _row_contiguous(x):
        x = x.contiguous()
    bias, scale = (_f32(bias).to(x.device).reshape(-1), _f32(scale).to(x.device).reshape(-1)) if bias is not None else (None, None)
    if not (torch.is_grad_enabled() and x.requires_grad):
        if out is None:
            out = torch.empty(shape, dtype=out_dtype, device=x.device)
        return _lat_lerp_fwd_raw(x.detach(), tables, bias, scale, out)
    return _LatInterp.apply(x, tables, bias, scale, out, out_dtype)


# ----------------------------------------------------------------------------
# correlated spherical noise (csrc/noise.hip: mk_noise_spectrum): the draw behind noise.SphericalNoise
# ----------------------------------------------------------------------------
NOISE_DEFAULT = "hip"           # MK_NOISE: hip | torch.  No row of tools/noise_bench.py is slower than torch

_U32 = 0xFFFFFFFF
_PHILOX_M0, _PHILOX_M1, _PHILOX_W0, _PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def noise_words(seed, q, l, m, t):
    """The four Philox4x32-10 words of counter ``(q, l, m, t)`` (each in [0, 2^32)) under ``seed`` (an int in [0, 2^64)), from the
    host code the kernel shares (``mk_noise_words``; no GPU needed), as Python ints in [0, 2^32)."""
    for v in (q, l, m, t):
        if not 0 <= v <= _U32:
            raise ValueError(f"noise_words: counter word {v} outside [0, 2^32)")
    out = (ctypes.c_int * 4)()
    l, m, t = (v - (1 << 32) if v >= 1 << 31 else v for v in (l, m, t))         # the ABI's ints carry the 32 bits
    _lib.check(_lib.load().mk_noise_words(_seed_ll(seed), q, l, m, t, ctypes.addressof(out)), "mk_noise_words")
    return [v & _U32 for v in out]


def _seed_ll(seed):
    """``seed`` in [0, 2^64) as the two's complement long long the C ABI takes."""
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"noise: seed {seed} outside [0, 2^64)")
    return seed - (1 << 64) if seed >= 1 << 63 else seed


def _philox_torch(c0, c1, c2, c3, seed):
    """Philox4x32-10 on int64 tensors holding 32-bit values (broadcast against each other): the four output words.  A 32 x 32-bit
    product passes int63, but the low 64 bits of the wrapped int64 product are the product's: the high word is masked after
    the (arithmetic) shift."""
    k0, k1 = seed & _U32, seed >> 32
    for _ in range(10):
        p0, p1 = c0 * _PHILOX_M0, c2 * _PHILOX_M1
        c0, c1, c2, c3 = ((p1 >> 32) & _U32) ^ c1 ^ k0, p1 & _U32, ((p0 >> 32) & _U32) ^ c3 ^ k1, p0 & _U32
        k0, k1 = (k0 + _PHILOX_W0) & _U32, (k1 + _PHILOX_W1) & _U32
    return c0, c1, c2, c3


def _noise_spectrum_torch(state, sigma_l, row_scale, l_off, m_off, row0, seed, t, t_dev, phi):
    """``mk_noise_spectrum`` restated with torch ops on ``state``'s device: the same counters, words, ``u1`` and ``u2`` (integer
    ops), Box-Muller and the amplitude in float64, rounded ONCE to fp32; the AR(1) step then in fp32 as the kernel has it.  No
    host synchronisation (``t_dev`` stays on the device)."""
    L, M, BC = state.shape
    dev = state.device
    nq = (BC + 1) // 2
    i64 = dict(dtype=torch.int64, device=dev)
    q = (torch.arange(nq, **i64) + (row0 >> 1)).view(1, 1, nq)
    gl = (torch.arange(L, **i64) + l_off).view(L, 1, 1)
    gm = (torch.arange(M, **i64) + m_off).view(1, M, 1)
    T = torch.full((1, 1, 1), int(t) & _U32, **i64)
    if t_dev is not None:
        T = (T + t_dev.to(torch.int64).view(1, 1, 1)) & _U32
    w0, w1, w2, w3 = _philox_torch(q, gl, gm, T, int(seed))
    shape = (L, M, 2 * nq)
    a = torch.stack([w0.expand(L, M, nq), w2.expand(L, M, nq)], dim=-1).reshape(shape)[..., :BC]
    b = torch.stack([w1.expand(L, M, nq), w3.expand(L, M, nq)], dim=-1).reshape(shape)[..., :BC]
    u1 = ((a >> 8) + 1).double() * 2.0 ** -24
    u2 = (b >> 8).double() * 2.0 ** -24
    rad = torch.sqrt(-2.0 * torch.log(u1))
    sig = sigma_l.double().view(L, 1, 1)
    amp = torch.where(gm == 0, sig, sig * math.sqrt(0.5))
    if row_scale is not None:
        amp = amp * row_scale.double().view(1, 1, BC)
    amp = torch.where(gl >= gm, amp * rad, torch.zeros((), dtype=torch.float64, device=dev))
    ang = (2.0 * math.pi) * u2
    xi = torch.complex((amp * torch.cos(ang)).float(), torch.where(gm == 0, torch.zeros_like(amp), amp * torch.sin(ang)).float())
    if phi == 0.0:
        return state.copy_(xi)
    phi32 = torch.tensor(phi, dtype=torch.float32, device=dev)
    c32 = torch.tensor(math.sqrt(1.0 - float(phi32) ** 2), dtype=torch.float32, device=dev)
    upd = torch.view_as_complex(phi32 * torch.view_as_real(state) + c32 * torch.view_as_real(xi))
    return state.copy_(torch.where(gl >= gm, upd, torch.zeros((), dtype=torch.complex64, device=dev)))


@torch.no_grad()
def noise_spectrum(state, sigma_l, seed, t=0, t_dev=None, phi=0.0, row_scale=None, l_off=0, m_off=0, row0=0):
    """One step of an isotropic Gaussian random field in spectral space, in place: ``state`` (complex64 ``[L, M, BC]``, the packed
    spectrum, contiguous) becomes ``xi`` (``phi == 0``; the old contents are not read) or ``phi state + sqrt(1 - phi^2) xi``
    (``0 < phi < 1``), and exact zero where the global degree is below the global order.  ``xi`` for global degree ``l_off + l``,
    order ``m_off + m`` and global row ``row0 + bc`` comes from Philox4x32-10 with key ``seed`` (an int in [0, 2^64)) and counter
    ``(row >> 1, degree, order, T)``, ``T = t + t_dev[0]`` modulo 2^32 (``t_dev``: a device int32 tensor read on the device, so a
    captured call draws anew on replay), through Box-Muller, times ``row_scale[bc] * sigma_l[l]`` (order 0, real) or that over
    ``sqrt 2`` (include/makani_amd.h has every formula).  A shard's draw is bitwise the slice of the unsharded draw; ``row0`` must be
    even.  ``sigma_l`` fp32 ``[L]``, ``row_scale`` fp32 ``[BC]`` or None, both on ``state``'s device.

    ``MK_NOISE=hip`` (read on every call): CUDA tensors take one ``mk_noise_spectrum`` launch on the current stream, capturable,
    the same bits every run.  CPU tensors and ``MK_NOISE=torch`` take ``_noise_spectrum_torch``: the same random words, float64
    Box-Muller rounded once, so the two agree to the rounding of the kernel's fp32 functions."""
    hip = _hip_or_torch("MK_NOISE", NOISE_DEFAULT)
    if state.dtype != torch.complex64 or state.dim() != 3 or not state.is_contiguous() or state.numel() == 0:
        raise ValueError(f"noise_spectrum: state must be a contiguous non-empty complex64 [L, M, BC] tensor, got {state.dtype} {tuple(state.shape)}")
    L, M, BC = state.shape
    seed_ll = _seed_ll(seed)
    phi = float(phi)
    if not 0.0 <= phi < 1.0:
        raise ValueError(f"noise_spectrum: phi {phi} outside [0, 1)")
    if row0 < 0 or row0 % 2 or l_off < 0 or m_off < 0:
        raise ValueError(f"noise_spectrum: row0 {row0} must be even and non-negative, offsets ({l_off}, {m_off}) non-negative")
    t = int(t)
    if not 0 <= t < 1 << 31:
        raise ValueError(f"noise_spectrum: t {t} outside [0, 2^31)")
    if (row0 >> 1) + (BC + 1) // 2 > 1 << 32:
        raise ValueError("noise_spectrum: the row pair index passes 2^32")
    if tuple(sigma_l.shape) != (L,) or sigma_l.device != state.device:
        raise ValueError(f"noise_spectrum: sigma_l {tuple(sigma_l.shape)} on {sigma_l.device} must be [{L}] on {state.device}")
    if row_scale is not None and (tuple(row_scale.shape) != (BC,) or row_scale.device != state.device):
        raise ValueError(f"noise_spectrum: row_scale {tuple(row_scale.shape)} on {row_scale.device} must be [{BC}] on {state.device}")
    if t_dev is not None and (t_dev.dtype != torch.int32 or t_dev.numel() != 1 or t_dev.device != state.device):
        raise ValueError("noise_spectrum: t_dev must be an int32 tensor of one element on the state's device")
    sigma_l, row_scale = _f32(sigma_l), _f32(row_scale)
    if not (hip and state.is_cuda):
        return _noise_spectrum_torch(state, sigma_l, row_scale, l_off, m_off, row0, seed, t, t_dev, phi)
    _lib.check(_lib.load().mk_noise_spectrum(state.data_ptr(), sigma_l.data_ptr(), _ptr(row_scale), L, M, BC, l_off, m_off, row0,
                                             seed_ll, t, _ptr(t_dev), phi, _stream()),
               "mk_noise_spectrum")
    return state


# ----------------------------------------------------------------------------
# cosine of the solar zenith angle (csrc/zenith.hip)
# ----------------------------------------------------------------------------
@torch.no_grad()
def cos_zenith(eph, sin_lat, cos_lat, lon_rad, out=None):
    """The zenith channel ``[..., H, W]`` fp32 from ``eph`` ``[..., 4]`` = (sin dec, cos dec, GMST, right ascension) per
    time and the grid's tables ``sin_lat``, ``cos_lat`` ``[H]`` and ``lon_rad`` ``[W]``:
    ``sin_lat sin dec + (cos_lat cos dec) cos((GMST + lon_rad) - ra)``, every product and sum an fp32 rounding of its
    own (the kernel is compiled with fp contraction off) (``mk_cos_zenith``; see ``makani_amd/zenith.py`` for the scalars and the tables).  One store-only HIP pass on the
    current stream; slices of the tables give the slice of the field bit for bit.  ``out``, if given, is a contiguous
    fp32 tensor of that many elements on the same device at any element-aligned address.  CUDA only, no gradient."""
    _need_cuda(eph, sin_lat, cos_lat, lon_rad, *([out] if out is not None else []))
    if eph.dim() < 1 or eph.shape[-1] != 4:
        raise ValueError(f"cos_zenith: eph {tuple(eph.shape)} must be [..., 4]")
    if sin_lat.dim() != 1 or cos_lat.shape != sin_lat.shape or lon_rad.dim() != 1:
        raise ValueError(f"cos_zenith: tables {tuple(sin_lat.shape)}, {tuple(cos_lat.shape)}, {tuple(lon_rad.shape)} must be [H], [H], [W]")
    H, W = sin_lat.shape[0], lon_rad.shape[0]
    n = eph.numel() // 4
    if out is None:
        out = torch.empty(*eph.shape[:-1], H, W, dtype=torch.float32, device=eph.device)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != n * H * W or out.device != eph.device:
        raise ValueError(f"cos_zenith: out must be a contiguous fp32 tensor of {n} x {H} x {W} elements on {eph.device}")
    for t in (sin_lat, cos_lat, lon_rad):
        if t.device != eph.device:
            raise ValueError(f"cos_zenith: tables on {t.device}, eph on {eph.device}")

    eph, sin_lat, cos_lat, lon_rad = _f32(eph), _f32(sin_lat), _f32(cos_lat), _f32(lon_rad)
    _lib.check(_lib.load().mk_cos_zenith(eph.data_ptr(), sin_lat.data_ptr(), cos_lat.data_ptr(), lon_rad.data_ptr(),
                                         out.data_ptr(), n, H, W, _stream()), "mk_cos_zenith")
    return out


# ----------------------------------------------------------------------------
# scaled-dot-product attention (csrc/attn.hip): the attention of the ViT blocks
# ----------------------------------------------------------------------------
# The kernels are the default by the rule of DESIGN section 19: no row of tools/attn_bench.py is slower than the torch path
# (DESIGN section 24).
ATTN_DEFAULT = "hip"


def attn_hip():
    """``MK_ATTN=hip|torch`` (read at call time): bf16 attention on the ``mk_attn_*`` kernels, or ``F.scaled_dot_product_attention``."""
    return _hip_or_torch("MK_ATTN", ATTN_DEFAULT)


# The same attention on fp32 operands outside autocast (csrc/x3_attn.hip), fp32-accurate on the bf16x3 arithmetic, is opt-in by
# the rule of DESIGN section 19 (DESIGN section 31 has the rows of tools/attn_fp32_bench.py).
ATTN_FP32_DEFAULT = "torch"
ATTN_X3_MAX_HEAD = 64


def attn_fp32_hip():
    """``MK_ATTN_FP32=hip|torch`` (read at call time): fp32 attention outside autocast on the ``mk_attn_x3_*`` kernels, or
    ``F.scaled_dot_product_attention``.  Independent of ``MK_ATTN``."""
    return _hip_or_torch("MK_ATTN_FP32", ATTN_FP32_DEFAULT)


class _AttnArith(typing.NamedTuple):
    """What differs between the two attention arithmetics; everything below is written once over it."""
    prefix: str                 # the entry points are <prefix>_info / _fwd / _bwd_delta / _bwd_dkv / _bwd_dq
    dtype: torch.dtype          # of every operand, the output and the gradients; strides are multiples of 16 bytes of it
    max_head: int               # head sizes are the multiples of 16 in 16 ... max_head
    x3: bool                    # runs on the bf16x3 engine: needs it selected (SPECTRAL_GEMM) and no device autocast
    fwd: typing.Callable        # the raw wrappers, looked up in the module when called
    bwd: typing.Callable


_ATTN_BF16 = _AttnArith("mk_attn", torch.bfloat16, 128, False, lambda *a: attn_fwd_raw(*a), lambda *a: attn_bwd_raw(*a))
_ATTN_X3 = _AttnArith("mk_attn_x3", torch.float32, ATTN_X3_MAX_HEAD, True, lambda *a: attn_x3_fwd_raw(*a), lambda *a: attn_x3_bwd_raw(*a))


def _attn_info(a, head_dim):
    t = (ctypes.c_int * 6)()
    _lib.check(getattr(_lib.load(), a.prefix + "_info")(int(head_dim), ctypes.addressof(t)), a.prefix + "_info")
    return (t[0], t[1]), (t[2], t[3]), (t[4], t[5])


def attn_info(head_dim):
    """(query tile, key tile) of the forward, the dK / dV and the dQ kernel at this head size: three pairs."""
    return _attn_info(_ATTN_BF16, head_dim)


def attn_x3_info(head_dim):
    """(query tile, key tile) of the fp32 forward, dK / dV and dQ kernels at this head size: three pairs (no device needed)."""
    return _attn_info(_ATTN_X3, head_dim)


def _attn_strides(t):
    """(batch, head, token) element strides of a ``[B, H, N, D]`` view; an axis of size 1 has no stride of its own."""
    sb, sh, sn = t.stride(0), t.stride(1), t.stride(2)
    return (sb if t.shape[0] > 1 else 0, sh if t.shape[1] > 1 else 0, sn if t.shape[2] > 1 else t.shape[3])


def _attn_operand_ok(t, dtype):
    """A ``[B, H, N, D]`` device view of this dtype, D contiguous, 16-byte aligned, every stride a multiple of 16 bytes."""
    if t.dim() != 4 or not t.is_cuda or t.dtype != dtype or t.stride(3) != 1 or t.data_ptr() % 16:
        return False
    unit = 16 // t.element_size()
    sb, sh, sn = _attn_strides(t)
    return min(sb, sh) >= 0 and sb % unit == 0 and sh % unit == 0 and sn % unit == 0 and sn >= t.shape[3]


def _attn_supported(a, q, k, v):
    if a.x3 and SPECTRAL_GEMM != "bf16x3":
        return False
    if not all(torch.is_tensor(t) and t.dim() == 4 for t in (q, k, v)):
        return False
    if not (k.shape == v.shape and q.shape[:2] == k.shape[:2] and q.shape[3] == k.shape[3]):
        return False
    D = q.shape[3]
    if D % 16 or not 16 <= D <= a.max_head or min(q.shape[2], k.shape[2], q.shape[0], q.shape[1]) < 1:
        return False
    if not all(_attn_operand_ok(t, a.dtype) for t in (q, k, v)):
        return False
    return not a.x3 or _autocast_dtype() is None


def attention_supported(q, k, v):
    """True when the kernels take these ``[B, H, N, D]`` views as they are: bf16 on the device, D a multiple of 16 in 16 ... 128 and
    contiguous, 16-byte aligned, batch / head / token strides multiples of 8 elements."""
    return _attn_supported(_ATTN_BF16, q, k, v)


def attention_x3_supported(q, k, v):
    """True when the ``mk_attn_x3_*`` kernels take these ``[B, H, N, D]`` views as they are: fp32 on the device with device
    autocast NOT active, the engine selected (``MK_SPECTRAL_GEMM=bf16x3``, as ``token_linear_x3_supported`` requires), D a
    multiple of 16 in 16 ... 64 and contiguous, 16-byte aligned, batch / head / token strides multiples of 4 elements."""
    return _attn_supported(_ATTN_X3, q, k, v)


def _attn_stride_array(*tensors):
    flat = [s for t in tensors for s in _attn_strides(t)]
    return (ctypes.c_longlong * len(flat))(*flat)


def _attn_fwd(a, q, k, v, o, lse, scale):
    B, H, Nq, D = q.shape
    st = _attn_stride_array(q, k, v, o)
    _lib.check(getattr(_lib.load(), a.prefix + "_fwd")(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), _ptr(lse), B, H, Nq,
                                                       k.shape[2], D, ctypes.addressof(st), float(scale), _stream()), a.prefix + "_fwd")


def _attn_bwd(a, q, k, v, o, go, lse, dq, dk, dv, scale):
    B, H, Nq, D = q.shape
    Nk = k.shape[2]
    lib = _lib.load()
    delta = torch.empty(B, H, Nq, dtype=torch.float32, device=q.device)
    st = _attn_stride_array(o, go)
    _lib.check(getattr(lib, a.prefix + "_bwd_delta")(o.data_ptr(), go.data_ptr(), delta.data_ptr(), B, H, Nq, D, ctypes.addressof(st),
                                                     _stream()), a.prefix + "_bwd_delta")
    st = _attn_stride_array(q, k, v, go, dk, dv)
    _lib.check(getattr(lib, a.prefix + "_bwd_dkv")(q.data_ptr(), k.data_ptr(), v.data_ptr(), go.data_ptr(), lse.data_ptr(), delta.data_ptr(),
                                                   dk.data_ptr(), dv.data_ptr(), B, H, Nq, Nk, D, ctypes.addressof(st), float(scale),
                                                   _stream()), a.prefix + "_bwd_dkv")
    st = _attn_stride_array(q, k, v, go, dq)
    _lib.check(getattr(lib, a.prefix + "_bwd_dq")(q.data_ptr(), k.data_ptr(), v.data_ptr(), go.data_ptr(), lse.data_ptr(), delta.data_ptr(),
                                                  dq.data_ptr(), B, H, Nq, Nk, D, ctypes.addressof(st), float(scale), _stream()),
               a.prefix + "_bwd_dq")


def attn_fwd_raw(q, k, v, o, lse, scale):
    """``o`` (a ``[B, H, Nq, D]`` view, written in place) and, unless None, ``lse`` ``[B, H, Nq]`` fp32 from ``[B, H, N, D]`` views."""
    _attn_fwd(_ATTN_BF16, q, k, v, o, lse, scale)


def attn_bwd_raw(q, k, v, o, go, lse, dq, dk, dv, scale):
    """The three gradients, written in place into the ``[B, H, N, D]`` views ``dq``, ``dk``, ``dv``: delta, then dK / dV, then dQ."""
    _attn_bwd(_ATTN_BF16, q, k, v, o, go, lse, dq, dk, dv, scale)


def attn_x3_fwd_raw(q, k, v, o, lse, scale):
    """``attn_fwd_raw`` on fp32 views."""
    _attn_fwd(_ATTN_X3, q, k, v, o, lse, scale)


def attn_x3_bwd_raw(q, k, v, o, go, lse, dq, dk, dv, scale):
    """``attn_bwd_raw`` on fp32 views: delta, then dK / dV, then dQ."""
    _attn_bwd(_ATTN_X3, q, k, v, o, go, lse, dq, dk, dv, scale)


def _attn_grad_out(go):
    """The upstream gradient as a view the kernels take (a token-major ``[B, N, H D]`` gradient already is one)."""
    return go if _attn_operand_ok(go, go.dtype) else go.contiguous()


def _node(name, doc, forward, backward):
    """An autograd function of this name -- its graph nodes are ``<name>Backward`` -- from two plain functions."""
    return type(name, (torch.autograd.Function,), dict(
        __doc__=doc, __module__=__name__, forward=staticmethod(forward),
        backward=staticmethod(torch.autograd.function.once_differentiable(backward))))


def _attention_node(name, a, doc):
    def forward(ctx, q, k, v, scale):
        B, H, Nq, D = q.shape
        o = torch.empty(B, Nq, H, D, dtype=q.dtype, device=q.device).permute(0, 2, 1, 3)
        need = any(ctx.needs_input_grad[:3])
        lse = torch.empty(B, H, Nq, dtype=torch.float32, device=q.device) if need else None
        a.fwd(q, k, v, o, lse, scale)
        if need:
            ctx.save_for_backward(q, k, v, o, lse)
            ctx.scale = scale
        return o

    def backward(ctx, go):
        q, k, v, o, lse = ctx.saved_tensors
        B, H, Nq, D = q.shape
        Nk = k.shape[2]
        dq = torch.empty(B, Nq, H, D, dtype=q.dtype, device=q.device).permute(0, 2, 1, 3)
        dk = torch.empty(B, Nk, H, D, dtype=q.dtype, device=q.device).permute(0, 2, 1, 3)
        dv = torch.empty(B, Nk, H, D, dtype=q.dtype, device=q.device).permute(0, 2, 1, 3)
        a.bwd(q, k, v, o, _attn_grad_out(go), lse, dq, dk, dv, ctx.scale)
        return dq, dk, dv, None

    return _node(name, doc, forward, backward)


_Attention = _attention_node("_Attention", _ATTN_BF16, """``softmax(scale q k^T) v`` on ``[B, H, N, D]`` views.  The output and the
    gradients are token-major buffers ``[B, N, H, D]`` seen through a permutation, so the ``transpose(1, 2).reshape(B, N, C)``
    behind the op is a view.""")
_AttentionX3 = _attention_node("_AttentionX3", _ATTN_X3, """``_Attention`` on fp32 views and the ``mk_attn_x3_*`` kernels: the same
    saved set, the same permuted-view outputs.""")


def _qkv_views(qkv, B, N, H, D):
    return tuple(t.permute(0, 2, 1, 3) for t in qkv.view(B, N, 3, H, D).unbind(2))


def _attention_packed_node(name, a, doc):
    def forward(ctx, qkv, H, scale):
        B, N, C3 = qkv.shape
        D = C3 // (3 * H)
        q, k, v = _qkv_views(qkv, B, N, H, D)
        o = torch.empty(B, N, H * D, dtype=qkv.dtype, device=qkv.device)
        need = ctx.needs_input_grad[0]
        lse = torch.empty(B, H, N, dtype=torch.float32, device=qkv.device) if need else None
        a.fwd(q, k, v, o.view(B, N, H, D).permute(0, 2, 1, 3), lse, scale)
        if need:
            ctx.save_for_backward(qkv, o, lse)
            ctx.args = (H, scale)
        return o

    def backward(ctx, go):
        qkv, o, lse = ctx.saved_tensors
        H, scale = ctx.args
        B, N, C3 = qkv.shape
        D = C3 // (3 * H)
        q, k, v = _qkv_views(qkv, B, N, H, D)
        dqkv = torch.empty(B, N, C3, dtype=qkv.dtype, device=qkv.device)
        dq, dk, dv = _qkv_views(dqkv, B, N, H, D)
        go = _attn_grad_out(go.reshape(B, N, H, D).permute(0, 2, 1, 3))
        a.bwd(q, k, v, o.view(B, N, H, D).permute(0, 2, 1, 3), go, lse, dq, dk, dv, scale)
        return dqkv, None, None

    return _node(name, doc, forward, backward)


_AttentionPacked = _attention_packed_node("_AttentionPacked", _ATTN_BF16, """The same on the projection output ``qkv``
    ``[B, N, 3 H D]`` as it stands: q, k, v are three strided views of it, the output is ``[B, N, H D]`` and the gradient one
    ``[B, N, 3 H D]`` buffer the kernels write in place.  No permuted copy, no cat.""")
_AttentionPackedX3 = _attention_packed_node("_AttentionPackedX3", _ATTN_X3, """``_AttentionPacked`` on an fp32 projection output
    ``[B, N, 3 H D]``: one gradient tensor, written in place.""")


def _attn_scale(scale, D):
    return float(scale) if scale is not None else 1.0 / math.sqrt(D)


def _attn_autocast(*tensors):
    """Under device autocast ``F.scaled_dot_product_attention`` takes its operands in the autocast dtype; so do these ops (the
    fp32 output of a ``qk_norm`` LayerNorm reaches the product as bf16 either way)."""
    dt = _autocast_dtype() if tensors[0].is_cuda else None
    return tensors if dt is None else tuple(t.to(dt) for t in tensors)


def _attn_arith(knobs, t, dropout_p):
    """The arithmetic of ``t``'s dtype when its knob is at ``hip`` and there is no dropout, else None: the torch call."""
    for a, on in zip((_ATTN_BF16, _ATTN_X3), knobs):
        if on and dropout_p == 0.0 and t.dtype == a.dtype:
            return a
    return None


def attention(q, k, v, scale=None, dropout_p=0.0):
    """``F.scaled_dot_product_attention(q, k, v)`` (no mask, not causal) for ``[B, H, N, D]`` views; returns ``[B, H, Nq, D]``.
    bf16 device tensors that ``attention_supported`` accepts run on the ``mk_attn_*`` kernels under ``MK_ATTN=hip``; fp32 device
    tensors outside autocast that ``attention_x3_supported`` accepts run on the ``mk_attn_x3_*`` kernels under ``MK_ATTN_FP32=hip``;
    fp16 inputs, CPU tensors, other head sizes or strides, ``dropout_p > 0`` and the knobs at ``torch`` take the torch formulation."""
    knobs = attn_hip(), attn_fp32_hip()
    q, k, v = _attn_autocast(q, k, v)
    a = _attn_arith(knobs, q, dropout_p)
    if a is not None and _attn_supported(a, q, k, v):
        return (_AttentionX3 if a.x3 else _Attention).apply(q, k, v, _attn_scale(scale, q.shape[-1]))
    return torch.nn.functional.scaled_dot_product_attention(q, k, v, dropout_p=dropout_p, scale=scale)


def attention_packed(qkv, num_heads, scale=None, dropout_p=0.0):
    """Self-attention on a fused projection output: ``qkv`` ``[B, N, 3 H D]`` laid out as ``[B, N, 3, H, D]`` -> ``[B, N, H D]``.
    Same dispatch as ``attention``; the HIP path reads q, k, v in place and returns the gradient as one tensor."""
    if qkv.dim() != 3 or qkv.shape[2] % (3 * int(num_heads)):
        raise ValueError(f"attention_packed: qkv {tuple(qkv.shape)} must be [B, N, 3 * {num_heads} * D]")
    B, N, C3 = qkv.shape
    H = int(num_heads)
    D = C3 // (3 * H)
    knobs = attn_hip(), attn_fp32_hip()
    (qkv,) = _attn_autocast(qkv)
    a = _attn_arith(knobs, qkv, dropout_p)
    if a is not None and qkv.is_cuda:
        x = qkv if (qkv.stride(2) == 1 and qkv.data_ptr() % 16 == 0) else qkv.contiguous()
        if _attn_supported(a, *_qkv_views(x.detach(), B, N, H, D)):
            return (_AttentionPackedX3 if a.x3 else _AttentionPacked).apply(x, H, _attn_scale(scale, D))
    q, k, v = (t.permute(0, 2, 1, 3) for t in qkv.reshape(B, N, 3, H, D).unbind(2))
    o = torch.nn.functional.scaled_dot_product_attention(q, k, v, dropout_p=dropout_p, scale=scale)
    return o.transpose(1, 2).reshape(B, N, H * D)


# ----------------------------------------------------------------------------
# layer norm over the trailing axes with the residual add fused in (csrc/toknorm.hip): the norms of ViT and AFNO
# ----------------------------------------------------------------------------
# Opt-in by the rule of DESIGN section 19: 8 of the 22 rows of tools/toknorm_bench.py are slower than the torch path (the
# single-kernel rows at (8100, 768), which are bound by the host, and four of the AFNO rows).
TOKEN_NORM_DEFAULT = "torch"


def token_norm_hip():
    """``MK_TOKEN_NORM=hip|torch`` (read at call time): trailing-axis layer norms on the ``mk_token_layernorm_*`` kernels, or
    ``F.layer_norm``."""
    return _hip_or_torch("MK_TOKEN_NORM", TOKEN_NORM_DEFAULT)


def _trailing(normalized_shape):
    shape = (normalized_shape,) if isinstance(normalized_shape, int) else tuple(normalized_shape)
    return shape, math.prod(shape)


def _rows_contiguous(t, k):
    """The last ``k`` axes of ``t`` are contiguous among themselves (from the strides: no view is made, this runs on every call)."""
    want = 1
    for size, stride in zip(reversed(t.shape[t.dim() - k:]), reversed(t.stride()[t.dim() - k:])):
        if size != 1 and stride != want:
            return False
        want *= size
    return True


def token_layer_norm_supported(x, normalized_shape, weight=None, bias=None):
    """True for device fp32 / bf16 tensors whose trailing axes are ``normalized_shape``, contiguous among themselves, next to
    fp32 parameters (or none).  Everything else is the caller's torch path."""
    shape, L = _trailing(normalized_shape)
    k = len(shape)
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype in _LOWP and k >= 1 and x.dim() >= k):
        return False
    if tuple(x.shape[x.dim() - k:]) != shape or x.numel() == 0:
        return False
    if any(p is not None and (p.dtype != torch.float32 or not p.is_cuda or tuple(p.shape) != shape) for p in (weight, bias)):
        return False
    return _rows_contiguous(x, k)


def _token_rows(t, k, L):
    """``t`` as rows the kernels take, and their element stride: itself where its memory already is ``rows`` rows of ``L``
    contiguous elements at one stride, a contiguous copy otherwise."""
    if t.is_contiguous():
        return t, L
    if t.dim() == k + 1 and _rows_contiguous(t, k) and (t.shape[0] == 1 or t.stride(0) >= L):
        return t, (L if t.shape[0] == 1 else t.stride(0))
    return t.contiguous(), L


def _tok3(t, ld=0):
    """(pointer, dtype code, row stride) of an optional tensor."""
    return (None, 0, 0) if t is None else (t.data_ptr(), _pw_dtype(t), ld)


def token_layernorm_fwd_raw(x, x_ld, r, r_ld, weight, bias, y, y2, s_out, stats, rows, L, eps):
    """One launch of ``mk_token_layernorm_fwd``; ``y``, ``y2``, ``s_out`` contiguous ``[rows, L]`` outputs or None."""
    _lib.check(_lib.load().mk_token_layernorm_fwd(*_tok3(x, x_ld), *_tok3(r, r_ld), _ptr(weight), _ptr(bias), *_tok3(y, L), _ptr(y2), L,
                                                  *_tok3(s_out, L), _ptr(stats), rows, L, float(eps), _stream()),
               "mk_token_layernorm_fwd")


def token_layernorm_bwd_raw(x, x_ld, r, r_ld, gy, gy_ld, gy2, gy2_ld, gs, gs_ld, stats, weight, gx, gr, gwb, rows, L):
    """``mk_token_layernorm_bwd``: one launch, plus the finishing launch when ``gwb`` ``[2, L]`` is asked for.  ``gx`` / ``gr`` have
    the layout of ``x`` / ``r``."""
    lib = _lib.load()
    ws = None
    if gwb is not None:
        ws = torch.empty(lib.mk_token_layernorm_workspace(rows, L), dtype=torch.float32, device=x.device)
    _lib.check(lib.mk_token_layernorm_bwd(*_tok3(x, x_ld), *_tok3(r, r_ld), *_tok3(gy, gy_ld), _ptr(gy2), gy2_ld, *_tok3(gs, gs_ld),
                                          stats.data_ptr(), _ptr(weight), gx.data_ptr(), _ptr(gr), _ptr(ws), _ptr(gwb), rows, L,
                                          _stream()), "mk_token_layernorm_bwd")


class _TokenLayerNorm(torch.autograd.Function):
    """``s = x + residual``, ``y = layer_norm(s)`` over the last ``k`` axes, with up to three results from one launch: ``y``, its
    bf16 copy ``y2`` (rounded from the same fp32 value) and ``s``.  Saves ``x``, ``residual`` and the per-row (mean, rstd): the
    backward recomputes ``s``, takes the gradients of all results in one launch and returns those of ``x``, ``residual``, the
    weight and the bias."""

    @staticmethod
    def forward(ctx, x, residual, weight, bias, eps, k, y_dtype, s_dtype, lowp, want_sum):
        _need_cuda(x)
        L = math.prod(x.shape[x.dim() - k:])
        rows = x.numel() // L
        x, x_ld = _token_rows(x, k, L)
        r, r_ld = (None, 0) if residual is None else _token_rows(residual, k, L)
        wf = None if weight is None else weight.contiguous()
        bf = None if bias is None else bias.contiguous()
        y = torch.empty(x.shape, dtype=y_dtype, device=x.device)
        y2 = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device) if lowp else None
        s = torch.empty(x.shape, dtype=s_dtype, device=x.device) if want_sum else None
        need = any(ctx.needs_input_grad[:4])
        stats = torch.empty(rows, 2, dtype=torch.float32, device=x.device) if need else None
        token_layernorm_fwd_raw(x, x_ld, r, r_ld, wf, bf, y, y2, s, stats, rows, L, eps)
        if need:
            ctx.save_for_backward(x, r, stats, wf)
            ctx.cfg = (k, L, rows, x_ld, r_ld, r is not None, weight is not None, bias is not None, bool(lowp), bool(want_sum))
            ctx.set_materialize_grads(False)
        return tuple(t for t in (y, y2, s) if t is not None)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        x, r, stats, wf = ctx.saved_tensors
        k, L, rows, x_ld, r_ld, has_r, has_w, has_b, lowp, want_sum = ctx.cfg
        grads = list(grads)
        gy = grads.pop(0)
        gy2 = grads.pop(0) if lowp else None
        gs = grads.pop(0) if want_sum else None

        def rows_of(g, dtypes):
            if g is None:
                return None, 0
            return _token_rows(g if g.dtype in dtypes else g.to(dtypes[0]), k, L)

        gy, gy_ld = rows_of(gy, _LOWP)
        gy2, gy2_ld = rows_of(gy2, (torch.bfloat16,))
        gs, gs_ld = rows_of(gs, _LOWP)
        gx = torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device=x.device)
        gr = torch.empty_strided(r.shape, r.stride(), dtype=r.dtype, device=x.device) if has_r and ctx.needs_input_grad[1] else None
        want = (has_w and ctx.needs_input_grad[2]) or (has_b and ctx.needs_input_grad[3])
        gwb = torch.empty(2, L, dtype=torch.float32, device=x.device) if want else None
        token_layernorm_bwd_raw(x, x_ld, r, r_ld, gy, gy_ld, gy2, gy2_ld, gs, gs_ld, stats, wf, gx, gr, gwb, rows, L)
        gw = gb = None
        if want:
            gw, gb = gwb.view(2, *x.shape[x.dim() - k:]).unbind(0)
            gw = gw if (has_w and ctx.needs_input_grad[2]) else None
            gb = gb if (has_b and ctx.needs_input_grad[3]) else None
        return (gx if ctx.needs_input_grad[0] else None), gr, gw, gb, None, None, None, None, None, None


def token_layer_norm(x, weight, bias, eps, residual=None, out_dtype=None, lowp=False, want_sum=False, normalized_shape=None):
    """``layer_norm(x + residual)`` over the trailing axes ``normalized_shape`` on the ``mk_token_layernorm_*`` kernels.
    ``normalized_shape`` None: the axes that ``weight`` / ``bias`` span, and the last axis when there are no parameters -- a norm
    without parameters over several axes has to name them; parameters of another shape are refused.  Returns ``y``, then its bf16 copy if ``lowp``, then the sum ``s`` if ``want_sum`` -- a
    single tensor when only ``y`` is asked for.  ``out_dtype`` None is the dtype of the sum (of ``x`` without a residual), and
    fp32 under device autocast, which is what torch's autocast gives ``layer_norm``.  There is no fallback: what
    ``token_layer_norm_supported`` declines is the caller's torch path."""
    ref = weight if weight is not None else bias
    if normalized_shape is not None:
        shape = _trailing(normalized_shape)[0]
    else:
        shape = tuple(ref.shape) if ref is not None else tuple(x.shape[-1:])
    ok = token_layer_norm_supported(x, shape, weight, bias) and (
        residual is None or (residual.shape == x.shape and token_layer_norm_supported(residual, shape)))
    if not ok:
        raise RuntimeError("makani_amd: token_layer_norm needs fp32 / bf16 tensors on a HIP device with contiguous trailing axes and "
                           "fp32 parameters; there is no fallback")
    if out_dtype not in (None, torch.float32, torch.bfloat16):
        raise TypeError(f"makani_amd token_layer_norm: unsupported out_dtype {out_dtype}")
    s_dtype = x.dtype if residual is None else torch.promote_types(x.dtype, residual.dtype)
    if out_dtype is None:
        out_dtype = torch.float32 if torch.is_autocast_enabled() else s_dtype
    out = _TokenLayerNorm.apply(x, residual, weight, bias, eps, len(shape), out_dtype, s_dtype, bool(lowp), bool(want_sum))
    return out[0] if len(out) == 1 else out


# ----------------------------------------------------------------------------
# token-major linear layers (csrc/toklinear.hip): nn.Linear on [..., features] activations
# ----------------------------------------------------------------------------
# Opt-in by the rule of DESIGN section 19: 14 of the 34 rows of tools/toklinear_bench.py are slower than the torch path (the
# compute-bound products of vit_73ch_big, and forward + backward of the small qkv / proj, which the host bounds).
TOKEN_LINEAR_DEFAULT = "torch"


def token_linear_hip():
    """``MK_TOKEN_LINEAR=hip|torch`` (read at call time): token-major linears on the ``mk_token_linear_*`` kernels, or ``F.linear``."""
    return _hip_or_torch("MK_TOKEN_LINEAR", TOKEN_LINEAR_DEFAULT)


def token_linear_info():
    """The tiles of the kernels (no device needed): ``tr``, ``tc``, ``tk`` -- row tile, output tile and contraction step of the
    GEMM -- and ``to``, ``ti``, ``ts`` -- output tile, input tile and token step of the weight gradient."""
    t = (ctypes.c_int * 6)()
    _lib.check(_lib.load().mk_token_linear_info(ctypes.addressof(t)), "mk_token_linear_info")
    return dict(zip(("tr", "tc", "tk", "to", "ti", "ts"), t))


def _row_stride(t):
    """The one element stride between the rows of ``t`` ``[..., L]`` seen as ``[rows, L]``, or None when the leading axes do not
    collapse to one stride or the last axis is not contiguous."""
    L = t.shape[-1]
    if t.dim() < 1 or (L != 1 and t.stride(-1) != 1):
        return None
    ld = None
    want = None                         # the stride the next axis outward must have
    for size, stride in zip(reversed(t.shape[:-1]), reversed(t.stride()[:-1])):
        if size == 1:
            continue
        if ld is None:
            ld = stride
        elif stride != want:
            return None
        want = stride * size
    return L if ld is None else ld


# The same linears on fp32 rows outside autocast (csrc/x3_toklinear.hip), fp32-accurate on the bf16x3 engine, are opt-in by the
# rule of DESIGN section 19 until every row of tools/toklinear_fp32_bench.py has been measured faster than the torch path
# (DESIGN section 30).
TOKEN_LINEAR_FP32_DEFAULT = "torch"


def token_linear_fp32_hip():
    """``MK_TOKEN_LINEAR_FP32=hip|torch`` (read at call time): fp32 token-major linears outside autocast on the
    ``mk_token_linear_x3_*`` kernels, or ``F.linear``.  Independent of ``MK_TOKEN_LINEAR``."""
    return _hip_or_torch("MK_TOKEN_LINEAR_FP32", TOKEN_LINEAR_FP32_DEFAULT)


def token_linear_x3_info():
    """The tile of the kernels (no device needed): ``tr`` rows, ``tc`` columns, ``tk`` contraction step."""
    t = (ctypes.c_int * 3)()
    _lib.check(_lib.load().mk_token_linear_x3_info(ctypes.addressof(t)), "mk_token_linear_x3_info")
    return dict(zip(("tr", "tc", "tk"), t))


class _LinearArith(typing.NamedTuple):
    """What differs between the two arithmetics of the token-major linears and the patch embedding.  The
    nodes, the predicates and the dispatch below are written once over it.  The functions are looked up in the module when
    they are called."""
    dtype: torch.dtype          # of the rows, the results and the data gradients
    unit: int                   # feature counts and every row stride (an fp32 addend's too) are multiples of it: 16 bytes of dtype
    param_dtypes: tuple         # of weights and biases
    x3: bool                    # runs on the bf16x3 engine: needs it selected (SPECTRAL_GEMM) and no bf16 device autocast
    weight: typing.Callable     # (weight) -> what the forward GEMM reads, saved for the backward
    gemm: typing.Callable       # (x, x_ld, w, bias, R, out, gelu, want_pre, addend, addend_ld) -> pre or None
    dgrad: typing.Callable      # (g, g_ld, saved w, R, out, aux, aux_ld): the data gradient, times gelu'(aux) with aux
    wgrad: typing.Callable      # the weight / bias gradient: the raw wrapper's signature
    gelu_grad: typing.Callable  # (g, g_ld, pre, R, O) -> g gelu'(pre) as contiguous rows, where no GEMM epilogue takes it


def _toklin_rows(t, unit):
    """``t`` ``[..., L]`` as the kernels of the arithmetic with this stride unit take it, and its row stride: itself where its
    layout fits, else a contiguous copy."""
    ld = _row_stride(t)
    if ld is None or ld % unit or ld < t.shape[-1] or t.data_ptr() % 16:
        return t.contiguous(), t.shape[-1]
    return t, ld


def _toklin_param_ok(a, p, shape, device):
    return torch.is_tensor(p) and p.device == device and p.dtype in a.param_dtypes and tuple(p.shape) == shape


def _toklin_supported(a, x, weight, bias):
    if a.x3 and SPECTRAL_GEMM != "bf16x3":
        return False
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() >= 1 and x.numel() > 0 and torch.is_tensor(weight) and weight.dim() == 2):
        return False
    O, I = weight.shape
    if x.shape[-1] != I or I % a.unit or O % a.unit or I < a.unit or O < a.unit:
        return False
    lowp = _autocast_dtype() == torch.bfloat16      # F.linear would take x in bf16
    if a.x3:
        if x.dtype != torch.float32 or lowp:
            return False
    elif x.dtype != torch.bfloat16 and not (x.is_floating_point() and lowp):
        return False
    if not _toklin_param_ok(a, weight, (O, I), x.device) or (bias is not None and not _toklin_param_ok(a, bias, (O,), x.device)):
        return False
    ld = _row_stride(x)
    if ld is None or ld % a.unit or ld < I:
        return False
    return x.dtype != a.dtype or x.data_ptr() % 16 == 0      # a cast under autocast makes a fresh, aligned tensor


def token_linear_supported(x, weight, bias=None):
    """True for what the ``mk_token_linear_*`` kernels take as it is: ``x`` ``[..., I]`` on the device in bf16 -- or in any
    floating-point dtype under bf16 device autocast, which takes it in bf16 as ``F.linear`` does --, its last axis contiguous, its
    rows at one common stride that is a multiple of 8, 16-byte aligned; ``I`` and ``O`` multiples of 8; ``weight`` ``[O, I]``
    and ``bias`` ``[O]`` (or None) fp32 or bf16 on the same device."""
    return _toklin_supported(_TOKLIN_BF16, x, weight, bias)


def token_linear_x3_supported(x, weight, bias=None):
    """True for what the ``mk_token_linear_x3_*`` kernels take as it is: ``x`` ``[..., I]`` fp32 on the device with bf16 device
    autocast NOT active, its last axis contiguous, its rows at one common stride that is a multiple of 4 and at least ``I``,
    16-byte aligned; ``I`` and ``O`` multiples of 4; ``weight`` ``[O, I]`` and ``bias`` ``[O]`` (or None) fp32 on the same device;
    and the engine selected (``MK_SPECTRAL_GEMM=bf16x3``, the default: with ``f32`` the torch path is taken)."""
    return _toklin_supported(_TOKLIN_X3, x, weight, bias)


def token_linear_pack_raw(weight, transpose=False):
    """The bf16 image ``[O, I]`` of ``weight`` (fp32 or bf16), or ``[I, O]`` with ``transpose``: one launch."""
    w = weight.detach()
    w = w if (w.stride(1) == 1 and w.stride(0) % 8 == 0 and w.stride(0) >= w.shape[1] and w.data_ptr() % 16 == 0) else w.contiguous()
    O, I = w.shape
    out = torch.empty((I, O) if transpose else (O, I), dtype=torch.bfloat16, device=w.device)
    _lib.check(_lib.load().mk_token_linear_pack(w.data_ptr(), _pw_dtype(w), w.stride(0), out.data_ptr(), out.shape[1], O, I,
                                                int(bool(transpose)), _stream()), "mk_token_linear_pack")
    return out


def _pl(t, ld=0):
    """(pointer, row stride) of an optional matrix."""
    return (None, 0) if t is None else (t.data_ptr(), ld)


def token_linear_fwd_raw(x, x_ld, wimg, bias, R, y=None, act=None, pre=None, addend=None, addend_ld=0, out_f32=None, aux=None, aux_ld=0):
    """One launch of ``mk_token_linear_fwd``: ``x`` ``R`` rows at stride ``x_ld``, ``wimg`` a contiguous bf16 image ``[O, I]``; the
    outputs (``y``, ``act``, ``pre``, ``out_f32``) contiguous ``[R, O]``; the epilogue follows from what is given."""
    O, I = wimg.shape
    _lib.check(_lib.load().mk_token_linear_fwd(x.data_ptr(), x_ld, wimg.data_ptr(), I, _ptr(bias), *_pl(y, O), *_pl(act, O), *_pl(pre, O),
                                               *_pl(addend, addend_ld), *_pl(out_f32, O), *_pl(aux, aux_ld), R, O, I, _stream()),
               "mk_token_linear_fwd")


def token_linear_wgrad_raw(dy, dy_ld, x, x_ld, R, O, I, want_db, slabs=0):
    """``dW`` fp32 ``[O, I]`` and ``db`` fp32 ``[O]`` (None unless ``want_db``) from ``dy`` ``[R, O]`` and ``x`` ``[R, I]``."""
    lib = _lib.load()
    dw = torch.empty(O, I, dtype=torch.float32, device=x.device)
    db = torch.empty(O, dtype=torch.float32, device=x.device) if want_db else None
    nbytes = lib.mk_token_linear_wgrad_workspace(R, O, I, slabs)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device) if nbytes > 0 else None
    _lib.check(lib.mk_token_linear_wgrad(dy.data_ptr(), dy_ld, x.data_ptr(), x_ld, dw.data_ptr(), I, _ptr(db), _ptr(ws), R, O, I, slabs,
                                         _stream()), "mk_token_linear_wgrad")
    return dw, db


def _toklin_x3_weight(weight):
    """The weight as the x3 kernels read it (no image is packed): itself, or a contiguous copy of a strided or misaligned one."""
    w = weight.detach()
    return w if (w.stride(1) == 1 and w.stride(0) % 4 == 0 and w.stride(0) >= w.shape[1] and w.data_ptr() % 16 == 0) else w.contiguous()


def token_linear_x3_fwd_raw(x, x_ld, w, bias, R, O, I, kmajor=False, y=None, pre=None, addend=None, addend_ld=0, aux=None, aux_ld=0,
                            gelu=False):
    """One launch of ``mk_token_linear_x3_fwd`` into the contiguous fp32 ``y`` ``[R, O]``: ``x`` ``R`` rows of ``I`` at stride
    ``x_ld``; ``w`` ``[O, I]``, or with ``kmajor`` ``[I, O]`` (the data gradient from the stored weight)."""
    _lib.check(_lib.load().mk_token_linear_x3_fwd(x.data_ptr(), x_ld, w.data_ptr(), w.stride(0), int(bool(kmajor)), _ptr(bias),
                                                  y.data_ptr(), O, *_pl(pre, O), *_pl(addend, addend_ld), *_pl(aux, aux_ld),
                                                  int(bool(gelu)), R, O, I, _stream()), "mk_token_linear_x3_fwd")
    return y


def token_linear_x3_wgrad_raw(dy, dy_ld, x, x_ld, R, O, I, want_db, slabs=0):
    """``dW`` fp32 ``[O, I]`` and ``db`` fp32 ``[O]`` (None unless ``want_db``) from fp32 ``dy`` ``[R, O]`` and ``x`` ``[R, I]``."""
    lib = _lib.load()
    dw = torch.empty(O, I, dtype=torch.float32, device=x.device)
    db = torch.empty(O, dtype=torch.float32, device=x.device) if want_db else None
    nbytes = lib.mk_token_linear_x3_wgrad_workspace(R, O, I, slabs)
    if nbytes < 0:
        raise RuntimeError(f"makani_amd mk_token_linear_x3_wgrad: sizes R = {R}, O = {O}, I = {I}, slabs = {slabs} are refused")
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    _lib.check(lib.mk_token_linear_x3_wgrad(dy.data_ptr(), dy_ld, x.data_ptr(), x_ld, dw.data_ptr(), I, _ptr(db), ws.data_ptr(), R, O, I,
                                            slabs, _stream()), "mk_token_linear_x3_wgrad")
    return dw, db


# ---- the GEMM is where the arithmetics really differ: a packed bf16 image and one output per epilogue, against the fp32 weight as
# ---- stored (k-major for the data gradient) and one output with a gelu flag.  Two short functions each, behind the description.
def _toklin_bf16_gemm(x, x_ld, wimg, bias, R, out, gelu=False, want_pre=False, addend=None, addend_ld=0):
    if addend is not None:
        token_linear_fwd_raw(x, x_ld, wimg, bias, R, addend=addend, addend_ld=addend_ld, out_f32=out)
    elif gelu:
        pre = torch.empty(out.shape, dtype=torch.bfloat16, device=out.device) if want_pre else None
        token_linear_fwd_raw(x, x_ld, wimg, bias, R, act=out, pre=pre)
        return pre
    else:
        token_linear_fwd_raw(x, x_ld, wimg, bias, R, y=out)
    return None


def _toklin_x3_gemm(x, x_ld, w, bias, R, out, gelu=False, want_pre=False, addend=None, addend_ld=0):
    O, I = w.shape
    pre = torch.empty(R, O, dtype=torch.float32, device=out.device) if (gelu and want_pre) else None
    token_linear_x3_fwd_raw(x, x_ld, w, bias, R, O, I, y=out, pre=pre, addend=addend, addend_ld=addend_ld, gelu=gelu)
    return pre


def _toklin_bf16_dgrad(g, g_ld, wimg, R, out, aux=None, aux_ld=0):
    token_linear_fwd_raw(g, g_ld, token_linear_pack_raw(wimg, transpose=True), None, R, y=out, aux=aux, aux_ld=aux_ld)


def _toklin_x3_dgrad(g, g_ld, w, R, out, aux=None, aux_ld=0):
    O, I = w.shape
    token_linear_x3_fwd_raw(g, g_ld, w, None, R, I, O, kmajor=True, y=out, aux=aux, aux_ld=aux_ld)


def _toklin_bf16_gelu_grad(g, g_ld, pre, R, O):
    """Rounded to bf16 as torch's gelu backward rounds it."""
    gp = torch.empty(R, O, dtype=torch.bfloat16, device=g.device)
    _lib.check(_lib.load().mk_token_linear_gelu_grad(g.data_ptr(), g_ld, pre.data_ptr(), O, gp.data_ptr(), O, R, O, _stream()),
               "mk_token_linear_gelu_grad")
    return gp


def _toklin_x3_gelu_grad(g, g_ld, pre, R, O):
    """One pointwise pass (``mk_bias_gelu_bwd``): it takes whole 8-element groups, which ``token_linear`` sees to."""
    gc = g if g_ld == O else g.contiguous()
    return gelu_backward(pre.view(1, 1, R * O), gc.view(1, 1, R * O))[0].view(R, O)


_TOKLIN_BF16 = _LinearArith(torch.bfloat16, 8, _LOWP, False, lambda w: token_linear_pack_raw(w),
                            _toklin_bf16_gemm, _toklin_bf16_dgrad, lambda *a: token_linear_wgrad_raw(*a), _toklin_bf16_gelu_grad)
_TOKLIN_X3 = _LinearArith(torch.float32, 4, (torch.float32,), True, _toklin_x3_weight,
                          _toklin_x3_gemm, _toklin_x3_dgrad, lambda *a: token_linear_x3_wgrad_raw(*a), _toklin_x3_gelu_grad)


def _toklin_grad_rows(g, O, a):
    """The incoming gradient as rows ``[R, O]`` in the arithmetic's dtype (for bf16: the gradient of the bf16 result that an fp32
    sum was formed from)."""
    g = g.reshape(-1, O)
    return _toklin_rows(g if g.dtype == a.dtype else g.to(a.dtype), a.unit)


def _toklin_param_grad(g, dtype):
    """The fp32 gradient in the parameter's dtype: a cast for a bf16 parameter, itself otherwise."""
    return None if g is None else (g if g.dtype == dtype else g.to(dtype))


def _dtype_of(t):
    return None if t is None else t.dtype


def _token_linear_node(name, a, doc):
    def forward(ctx, x, weight, bias, gelu, addend):
        O, I = weight.shape
        xr, x_ld = _toklin_rows(x, a.unit)
        R = x.numel() // I
        w = a.weight(weight)
        bf = _f32(bias)
        need = any(ctx.needs_input_grad[:3])
        ar, a_ld = (None, 0) if addend is None else _toklin_rows(addend.detach().reshape(-1, O), a.unit)
        out = torch.empty(x.shape[:-1] + (O,), dtype=a.dtype if addend is None else torch.float32, device=x.device)
        pre = a.gemm(xr, x_ld, w, bf, R, out, gelu, need, ar, a_ld)
        if need:
            ctx.save_for_backward(xr, w, pre)
        ctx.cfg = (x_ld, R, tuple(x.shape), weight.dtype, _dtype_of(bias))
        return out

    def backward(ctx, g):
        if not ctx.saved_tensors:               # only the addend asks for a gradient: the incoming one
            return None, None, None, None, g
        xr, w, pre = ctx.saved_tensors
        x_ld, R, x_shape, w_dtype, b_dtype = ctx.cfg
        O, I = w.shape
        need = ctx.needs_input_grad
        g_in = g
        g, g_ld = _toklin_grad_rows(g, O, a)
        if pre is not None:                     # through the GELU: g gelu'(pre)
            g, g_ld = a.gelu_grad(g, g_ld, pre, R, O), O
        dx = dw = db = None
        if need[0]:
            dx = torch.empty(x_shape, dtype=a.dtype, device=g.device)
            a.dgrad(g, g_ld, w, R, dx)
        want_db = b_dtype is not None and need[2]
        if need[1] or want_db:
            dw, db = a.wgrad(g, g_ld, xr, x_ld, R, O, I, want_db)
            dw = _toklin_param_grad(dw, w_dtype) if need[1] else None
            db = _toklin_param_grad(db, b_dtype)
        return dx, dw, db, None, (g_in if need[4] else None)

    return _node(name, doc, forward, backward)


_TokenLinear = _token_linear_node("_TokenLinear", _TOKLIN_BF16, """``y = x W^T + b`` on bf16 rows, optionally through the exact GELU
    or added to an fp32 ``addend``: one pack and one GEMM.  Saves ``x``, the bf16 weight image and, with ``gelu``, the
    pre-activation.  Backward: ``g gelu'(pre)`` first with ``gelu``, a transposed pack and the GEMM again for ``dx``, the slab
    kernel for ``dW`` and ``db`` (fp32, cast to a bf16 parameter's dtype).""")
_TokenLinearX3 = _token_linear_node("_TokenLinearX3", _TOKLIN_X3, """The same on fp32 rows: one GEMM on the bf16x3 engine.  Saves
    ``x``, the weight itself and, with ``gelu``, the pre-activation.  Backward: ``g gelu'(pre)`` first with ``gelu``, the k-major
    GEMM on the stored weight for ``dx``, the slab kernel for ``dW`` and ``db``.  All fp32.""")


def _token_mlp_node(name, a, doc):
    def forward(ctx, x, w1, b1, w2, b2, addend):
        H, I = w1.shape
        O = w2.shape[0]
        xr, x_ld = _toklin_rows(x, a.unit)
        R = x.numel() // I
        w1p, w2p = a.weight(w1), a.weight(w2)
        need = any(ctx.needs_input_grad[:5])
        act = torch.empty(R, H, dtype=a.dtype, device=x.device)
        pre = a.gemm(xr, x_ld, w1p, _f32(b1), R, act, True, need)
        ar, a_ld = (None, 0) if addend is None else _toklin_rows(addend.detach().reshape(-1, O), a.unit)
        out = torch.empty(x.shape[:-1] + (O,), dtype=a.dtype if addend is None else torch.float32, device=x.device)
        a.gemm(act, H, w2p, _f32(b2), R, out, False, False, ar, a_ld)
        if need:
            ctx.save_for_backward(xr, w1p, w2p, pre, act)
        ctx.cfg = (x_ld, R, tuple(x.shape), w1.dtype, _dtype_of(b1), w2.dtype, _dtype_of(b2))
        return out

    def backward(ctx, g):
        if not ctx.saved_tensors:               # only the addend asks for a gradient: the incoming one
            return None, None, None, None, None, g
        xr, w1p, w2p, pre, act = ctx.saved_tensors
        x_ld, R, x_shape, w1, b1, w2, b2 = ctx.cfg                 # the parameters' dtypes; None: no bias
        H, I = w1p.shape
        O = w2p.shape[0]
        need = ctx.needs_input_grad
        g_in = g
        g, g_ld = _toklin_grad_rows(g, O, a)
        dw2 = db2 = dw1 = db1 = dx = None
        if need[3] or (b2 is not None and need[4]):
            dw2, db2 = a.wgrad(g, g_ld, act, H, R, O, H, b2 is not None and need[4])
            dw2 = _toklin_param_grad(dw2, w2) if need[3] else None
            db2 = _toklin_param_grad(db2, b2)
        if need[0] or need[1] or (b1 is not None and need[2]):
            dpre = torch.empty(R, H, dtype=a.dtype, device=g.device)
            a.dgrad(g, g_ld, w2p, R, dpre, aux=pre, aux_ld=H)
            if need[1] or (b1 is not None and need[2]):
                dw1, db1 = a.wgrad(dpre, H, xr, x_ld, R, H, I, b1 is not None and need[2])
                dw1 = _toklin_param_grad(dw1, w1) if need[1] else None
                db1 = _toklin_param_grad(db1, b1)
            if need[0]:
                dx = torch.empty(x_shape, dtype=a.dtype, device=g.device)
                a.dgrad(dpre, H, w1p, R, dx)
        return dx, dw1, db1, dw2, db2, (g_in if need[5] else None)

    return _node(name, doc, forward, backward)


_TokenMLP = _token_mlp_node("_TokenMLP", _TOKLIN_BF16, """``fc2(gelu(fc1(x)))`` (+ an fp32 ``addend``) on bf16 rows: two packs and two
    GEMMs, ``fc1``'s with the GELU epilogue (``pre`` stored in grad mode only), ``fc2``'s with the addend.  Saves ``x``, the two
    weight images, ``pre`` and ``act``.  Backward, in order: ``fc2``'s weight gradient on ``act``; ``fc2``'s data gradient with the
    GELU' epilogue on ``pre``, which is ``dpre``; ``fc1``'s weight gradient and data gradient from ``dpre``; the addend's gradient
    is the incoming gradient.""")
_TokenMLPX3 = _token_mlp_node("_TokenMLPX3", _TOKLIN_X3, """``_TokenMLP`` on fp32 rows: two GEMMs on the bf16x3 engine.  Saves ``x``,
    the two weights themselves, ``pre`` and ``act``; the data gradients are k-major GEMMs on the stored weights.  All fp32.""")


def _toklin_addend_fused(addend, x, O):
    """The kernels add an fp32 device addend of the output's shape in their epilogue; any other is added by torch."""
    return (addend is not None and torch.is_tensor(addend) and addend.dtype == torch.float32 and addend.device == x.device
            and tuple(addend.shape) == tuple(x.shape[:-1]) + (O,))


def _toklin_takes(a, x, weight, bias, second):
    """The kernels of arithmetic ``a`` take this linear and, for the MLP, the ``second = (w2, b2)`` behind it."""
    if not _toklin_supported(a, x, weight, bias):
        return False
    if second is None:
        return True
    w2, b2 = second
    return (torch.is_tensor(w2) and w2.dim() == 2 and w2.shape[1] == weight.shape[0] and w2.shape[0] % a.unit == 0
            and _toklin_param_ok(a, w2, tuple(w2.shape), x.device) and (b2 is None or _toklin_param_ok(a, b2, (w2.shape[0],), x.device)))


def _toklin_arith(x, weight, bias, second=None):
    """The arithmetic whose knob is at ``hip`` and whose kernels take this: bf16 first, then fp32; None is the torch path."""
    fp32_hip = token_linear_fp32_hip()
    if token_linear_hip() and _toklin_takes(_TOKLIN_BF16, x, weight, bias, second):
        return _TOKLIN_BF16
    if fp32_hip and _toklin_takes(_TOKLIN_X3, x, weight, bias, second):
        return _TOKLIN_X3
    return None


def token_linear(x, weight, bias=None, gelu=False, addend=None):
    """``F.linear(x, weight, bias)`` over any leading axes -- ``F.gelu`` of it with ``gelu``, ``addend +`` it with ``addend`` (not
    both) -- as one autograd function on the ``mk_token_linear_*`` kernels: bf16 result, or the fp32 sum with an fp32 ``addend``.
    fp32 rows outside bf16 autocast take, under ``MK_TOKEN_LINEAR_FP32=hip`` and for what ``token_linear_x3_supported`` accepts, the
    same node on the ``mk_token_linear_x3_*`` kernels (fp32 results).  What both decline, CPU tensors and the knobs at ``torch``
    take ``F.linear`` / ``F.gelu``."""
    if gelu and addend is not None:
        raise ValueError("token_linear: gelu and addend cannot be combined")
    a = _toklin_arith(x, weight, bias)
    if a is not None:
        node = _TokenLinearX3 if a.x3 else _TokenLinear
        xa = x if x.dtype == a.dtype else x.to(a.dtype)
        if addend is None:
            if gelu and a.x3 and (x.numel() // x.shape[-1] * weight.shape[0]) % 8:     # the GELU-gradient pass takes whole 8-element groups
                return torch.nn.functional.gelu(node.apply(xa, weight, bias, False, None))
            return node.apply(xa, weight, bias, bool(gelu), None)
        if _toklin_addend_fused(addend, x, weight.shape[0]):
            return node.apply(xa, weight, bias, False, addend)
        return addend + node.apply(xa, weight, bias, False, None)
    y = torch.nn.functional.linear(x, weight, bias)
    if gelu:
        y = torch.nn.functional.gelu(y)
    return y if addend is None else addend + y


def token_mlp(x, w1, b1, w2, b2, addend=None):
    """``F.linear(F.gelu(F.linear(x, w1, b1)), w2, b2)`` (``addend +`` it with ``addend``) as one autograd function on the
    ``mk_token_linear_*`` kernels, with the GELU in ``fc1``'s epilogue, the addend in ``fc2``'s and the GELU gradient in the
    epilogue of ``fc2``'s data gradient.  Same dispatch as ``token_linear``: the bf16 branch, then the fp32 one, then torch."""
    a = _toklin_arith(x, w1, b1, second=(w2, b2))
    if a is not None:
        node = _TokenMLPX3 if a.x3 else _TokenMLP
        xa = x if x.dtype == a.dtype else x.to(a.dtype)
        if addend is None or _toklin_addend_fused(addend, x, w2.shape[0]):
            return node.apply(xa, w1, b1, w2, b2, addend)
        return addend + node.apply(xa, w1, b1, w2, b2, None)
    F = torch.nn.functional
    y = F.linear(F.gelu(F.linear(x, w1, b1)), w2, b2)
    return y if addend is None else addend + y


# ----------------------------------------------------------------------------
# patch rows (csrc/patch.hip): the gather in front of the patch-embedding GEMM and the un-patchify behind the heads
# ----------------------------------------------------------------------------
# Opt-in by the rule of DESIGN section 19 until every row of tools/patch_bench.py has been measured faster than the torch path
# (DESIGN section 29).
PATCH_DEFAULT = "torch"


def patch_hip():
    """``MK_PATCH=hip|torch`` (read at call time): patch embedding and un-patchify on ``mk_patchify`` / ``mk_unpatchify`` around the
    ``mk_token_linear_*`` GEMM, or ``nn.Conv2d`` and torch's permuted copies."""
    return _hip_or_torch("MK_PATCH", PATCH_DEFAULT)


def _patch_geometry(C, H, W, patch):
    p0, p1 = int(patch[0]), int(patch[1])
    if p0 < 1 or p1 < 1 or H % p0 or W % p1:
        raise ValueError(f"patch {p0} x {p1} does not divide the grid {H} x {W}")
    return p0, p1, H // p0, W // p1, C * p0 * p1


def _patchify_torch(img, patch, order):
    B, C, H, W = img.shape
    p0, p1, hp, wp, F = _patch_geometry(C, H, W, patch)
    v = img.reshape(B, C, hp, p0, wp, p1)
    v = v.permute(0, 2, 4, 1, 3, 5) if order == 0 else v.permute(0, 2, 4, 3, 5, 1)
    return v.reshape(B, hp * wp, F)


def _patch_batch(tok, hp, wp, F):
    """The batch of token rows ``[B, ..., F]`` with ``hp wp`` rows per sample; refuses any other shape."""
    if tok.dim() < 2 or tok.shape[-1] != F or tok.numel() == 0 or tok.numel() % (hp * wp * F):
        raise ValueError(f"token rows of shape {tuple(tok.shape)} are not [B, ..., {F}] with {hp * wp} rows per sample")
    return tok.numel() // (hp * wp * F)


def _unpatchify_torch(tok, patch, C, H, W, order):
    p0, p1, hp, wp, F = _patch_geometry(C, H, W, patch)
    B = _patch_batch(tok, hp, wp, F)
    if order == 0:
        v = tok.reshape(B, hp, wp, C, p0, p1).permute(0, 3, 1, 4, 2, 5)
    else:
        v = tok.reshape(B, hp, wp, p0, p1, C).permute(0, 5, 1, 3, 2, 4)
    return v.reshape(B, C, H, W)


def _patch_order(order):
    if order not in (0, 1):
        raise ValueError(f"unknown patch feature order {order!r} (0: (c, i, j), the convolution's | 1: (i, j, c), the heads')")
    return int(order)


def patchify_raw(img, tok, patch, order=0, ldt=None):
    """``mk_patchify``: ``img`` ``[B, C, H, W]`` contiguous -> the preallocated rows ``tok`` (``B hp wp`` rows at stride ``ldt``,
    default the features of a token), fp32 or bf16 on either side."""
    _need_cuda(img, tok)
    B, C, H, W = img.shape
    assert img.is_contiguous() and img.device == tok.device
    _lib.check(_lib.load().mk_patchify(img.data_ptr(), _DTYPE_CODE[img.dtype], tok.data_ptr(), _DTYPE_CODE[tok.dtype],
                                       C * patch[0] * patch[1] if ldt is None else ldt, B, C, H, W, patch[0], patch[1], order,
                                       _stream()), "mk_patchify")
    return tok


def unpatchify_raw(tok, img, patch, order=0, ldt=None):
    """``mk_unpatchify``: the rows ``tok`` (stride ``ldt``) -> the preallocated contiguous ``img`` ``[B, C, H, W]``."""
    _need_cuda(img, tok)
    B, C, H, W = img.shape
    assert img.is_contiguous() and img.device == tok.device
    _lib.check(_lib.load().mk_unpatchify(tok.data_ptr(), _DTYPE_CODE[tok.dtype], C * patch[0] * patch[1] if ldt is None else ldt,
                                         img.data_ptr(), _DTYPE_CODE[img.dtype], B, C, H, W, patch[0], patch[1], order, _stream()),
               "mk_unpatchify")
    return img


class _Patchify(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, patch, order, dtype):
        B, C, H, W = img.shape
        p0, p1, hp, wp, F = _patch_geometry(C, H, W, patch)
        ctx.cfg = (tuple(img.shape), img.dtype, (p0, p1), order)
        return patchify_raw(img.contiguous(), torch.empty(B, hp * wp, F, dtype=dtype, device=img.device), (p0, p1), order)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        shape, dtype, patch, order = ctx.cfg
        g = _lowp(g)
        return unpatchify_raw(g.contiguous(), torch.empty(shape, dtype=dtype, device=g.device), patch, order), None, None, None


class _Unpatchify(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tok, patch, C, H, W, order, dtype):
        p0, p1, hp, wp, F = _patch_geometry(C, H, W, patch)
        B = _patch_batch(tok, hp, wp, F)
        ctx.cfg = (tuple(tok.shape), tok.dtype, (p0, p1), order)
        return unpatchify_raw(tok.contiguous(), torch.empty(B, C, H, W, dtype=dtype, device=tok.device), (p0, p1), order)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        shape, dtype, patch, order = ctx.cfg
        g = _lowp(g)
        return (patchify_raw(g.contiguous(), torch.empty(shape, dtype=dtype, device=g.device), patch, order),) + (None,) * 6


def _patch_kernels_take(t, dtype):
    return t.is_cuda and t.numel() > 0 and t.dtype in _DTYPE_CODE and dtype in _DTYPE_CODE


def patchify(img, patch, order=0, dtype=None):
    """``img`` ``[B, C, H, W]`` -> the patch rows ``[B, hp wp, C p0 p1]`` in ``dtype`` (default the image's): row ``y wp + x`` is the
    patch at ``(y p0, x p1)``, its features in ``order`` 0 ``(c, i, j)`` -- a convolution weight's ``view(E, -1)`` -- or 1
    ``(i, j, c)``, the heads'.  One ``mk_patchify`` pass on the device (fp32 / bf16; the cast in the same pass), its backward one
    ``mk_unpatchify`` pass into the image's dtype.  CPU tensors, other dtypes and ``MK_PATCH=torch`` take ``reshape`` / ``permute``."""
    order = _patch_order(order)
    dtype = img.dtype if dtype is None else dtype
    assert img.dim() == 4, "[B, C, H, W]"
    if patch_hip() and _patch_kernels_take(img, dtype):
        return _Patchify.apply(img, tuple(patch), order, dtype)
    return _patchify_torch(img, patch, order).to(dtype)


def unpatchify(tok, patch, out_chans, img_shape, order, dtype=None):
    """The inverse of ``patchify``: ``tok`` ``[B, ..., C p0 p1]`` (``hp wp`` rows per sample) -> ``[B, C, H, W]`` with ``C =
    out_chans``, ``(H, W) = img_shape``.  ``order`` 1 is the rearrangement behind both patch heads (``einsum("nhwpqc->nchpwq")`` of
    ViT, ``permute(0, 5, 1, 3, 2, 4)`` of AFNOv1).  One ``mk_unpatchify`` pass, its backward one ``mk_patchify`` pass into the
    rows' dtype; same dispatch as ``patchify``."""
    order = _patch_order(order)
    dtype = tok.dtype if dtype is None else dtype
    H, W = int(img_shape[0]), int(img_shape[1])
    if patch_hip() and _patch_kernels_take(tok, dtype):
        return _Unpatchify.apply(tok, tuple(patch), int(out_chans), H, W, order, dtype)
    return _unpatchify_torch(tok, patch, int(out_chans), H, W, order).to(dtype)


def _patch_embed_supported(a, img, weight, bias):
    if a.x3 and SPECTRAL_GEMM != "bf16x3":
        return False
    if not (torch.is_tensor(img) and img.is_cuda and img.dim() == 4 and img.numel() > 0 and torch.is_tensor(weight) and weight.dim() == 4):
        return False
    E, C, p0, p1 = weight.shape
    F = C * p0 * p1
    if img.shape[1] != C or img.shape[2] % p0 or img.shape[3] % p1 or F % a.unit or E % a.unit:
        return False
    lowp = _autocast_dtype() == torch.bfloat16      # the convolution would take the image in bf16
    if a.x3:
        if img.dtype != torch.float32 or lowp:
            return False
    elif img.dtype not in _DTYPE_CODE or not (lowp or all(t.dtype == torch.bfloat16 for t in (img, weight, bias) if t is not None)):
        return False
    return _toklin_param_ok(a, weight, (E, C, p0, p1), img.device) and (bias is None or _toklin_param_ok(a, bias, (E,), img.device))


def patch_embed_supported(img, weight, bias=None):
    """True for what ``_PatchEmbed`` takes: ``img`` ``[B, C, H, W]`` on the device, fp32 or bf16 under bf16 device autocast -- which
    takes it in bf16 as the convolution does -- or, without autocast, bf16 with bf16 parameters (``nn.Conv2d`` refuses mixed dtypes
    there, and so does this); ``weight`` ``[E, C, p0, p1]`` with a patch that divides the grid, ``C p0 p1`` and ``E`` multiples of 8,
    ``weight`` and ``bias`` ``[E]`` (or None) fp32 or bf16 on the same device.  Independent of ``MK_TOKEN_LINEAR``."""
    return _patch_embed_supported(_TOKLIN_BF16, img, weight, bias)


def patch_embed_x3_supported(img, weight, bias=None):
    """True for what ``_PatchEmbedX3`` takes: ``img`` ``[B, C, H, W]`` fp32 on the device with bf16 device autocast NOT active,
    ``weight`` ``[E, C, p0, p1]`` with a patch that divides the grid, ``C p0 p1`` and ``E`` multiples of 4, ``weight`` and ``bias``
    ``[E]`` (or None) fp32 on the same device, and the bf16x3 engine selected (``MK_SPECTRAL_GEMM``)."""
    return _patch_embed_supported(_TOKLIN_X3, img, weight, bias)


def _patch_embed_node(name, a, doc):
    def forward(ctx, img, weight, bias, pos):
        B, C, H, W = img.shape
        E, _, p0, p1 = weight.shape
        _, _, hp, wp, F = _patch_geometry(C, H, W, (p0, p1))
        N = hp * wp
        rows = patchify_raw(img.detach().contiguous(), torch.empty(B * N, F, dtype=a.dtype, device=img.device), (p0, p1), 0)
        w = a.weight(weight.detach().reshape(E, F))
        bf = _f32(bias)
        out = torch.empty(B, N, E, dtype=a.dtype if pos is None else torch.float32, device=img.device)
        if pos is not None:
            pr, p_ld = _toklin_rows(pos.detach().reshape(N, E), a.unit)
            for b in range(B):
                a.gemm(rows[b * N:(b + 1) * N], F, w, bf, N, out[b], False, False, pr, p_ld)
        else:
            a.gemm(rows, F, w, bf, B * N, out)
        if any(ctx.needs_input_grad[:3]):
            ctx.save_for_backward(rows, w)
        ctx.cfg = (tuple(img.shape), img.dtype, tuple(weight.shape), weight.dtype, _dtype_of(bias), None if pos is None else tuple(pos.shape))
        return out

    def backward(ctx, g):
        img_shape, img_dtype, w_shape, w_dtype, b_dtype, pos_shape = ctx.cfg
        need = ctx.needs_input_grad
        dpos = g.sum(0).reshape(pos_shape) if (pos_shape is not None and need[3]) else None
        if not ctx.saved_tensors:
            return None, None, None, dpos
        rows, w = ctx.saved_tensors
        E, F = w.shape
        R = rows.shape[0]
        gr, g_ld = _toklin_grad_rows(g, E, a)
        dx = dw = db = None
        want_db = b_dtype is not None and need[2]
        if need[1] or want_db:
            dw, db = a.wgrad(gr, g_ld, rows, F, R, E, F, want_db)
            dw = _toklin_param_grad(dw, w_dtype).view(w_shape) if need[1] else None
            db = _toklin_param_grad(db, b_dtype)
        if need[0]:
            dxr = torch.empty(R, F, dtype=a.dtype, device=g.device)
            a.dgrad(gr, g_ld, w, R, dxr)
            dx = unpatchify_raw(dxr, torch.empty(img_shape, dtype=img_dtype, device=g.device), w_shape[2:], 0)
        return dx, dw, db, dpos

    return _node(name, doc, forward, backward)


_PatchEmbed = _patch_embed_node("_PatchEmbed", _TOKLIN_BF16, """A non-overlapping strided convolution as one GEMM on patch rows:
    ``mk_patchify`` (order 0, to bf16: the autocast cast of the image in the same pass), the weight's bf16 image,
    ``mk_token_linear_fwd`` with the fp32 bias.  With ``pos`` (fp32 ``[N, E]``) one GEMM launch per sample with ``pos`` as its
    addend: ``pos + float(bf16(acc + bias))``, fp32.  Saves the patch rows and the weight image.  Backward: the slab kernel for
    ``dW`` / ``db``; the batch sum of the gradient for ``pos``; for the image, where it asks, a transposed pack, the GEMM to bf16
    rows and ``mk_unpatchify`` into the image's dtype.""")
_PatchEmbedX3 = _patch_embed_node("_PatchEmbedX3", _TOKLIN_X3, """``_PatchEmbed`` on fp32 images outside autocast: fp32 patch rows,
    then ``mk_token_linear_x3_fwd`` on the weight's ``[E, F]`` view with the bias.  Saves the patch rows and the weight view; the
    image's gradient is the k-major GEMM on the stored weight and ``mk_unpatchify``.  All fp32.""")


def _patch_pos_fused(pos, img, N, E):
    return (torch.is_tensor(pos) and pos.dtype == torch.float32 and pos.device == img.device
            and tuple(pos.shape) in ((1, N, E), (N, E)))


def patch_embed(img, weight, bias=None, pos=None):
    """``F.conv2d(img, weight, bias, stride=patch).flatten(2).transpose(1, 2)`` (``+ pos``): ``[B, C, H, W]`` -> ``[B, N, E]`` for
    ``weight`` ``[E, C, p0, p1]``.  Under ``MK_PATCH=hip``, for what ``patch_embed_supported`` takes, one autograd function on
    ``mk_patchify`` and the ``mk_token_linear_*`` kernels: a bf16 result, or with an fp32 ``pos`` (``[1, N, E]`` or ``[N, E]``) the
    fp32 sum ``pos + float(bf16(conv))`` from the GEMM's epilogue -- the rounding points of the torch expression under bf16
    autocast.  An fp32 image outside autocast, under ``MK_PATCH=hip`` AND ``MK_TOKEN_LINEAR_FP32=hip`` and for what
    ``patch_embed_x3_supported`` takes, is the same node on fp32 rows and the ``mk_token_linear_x3_*`` kernels: an fp32 result.
    Everything else takes the torch expression."""
    patch, fp32_hip = patch_hip(), token_linear_fp32_hip()
    node = None
    if patch and _patch_embed_supported(_TOKLIN_BF16, img, weight, bias):
        node = _PatchEmbed
    elif patch and fp32_hip and _patch_embed_supported(_TOKLIN_X3, img, weight, bias):
        node = _PatchEmbedX3
    if node is not None:
        E, _, p0, p1 = weight.shape
        N = (img.shape[2] // p0) * (img.shape[3] // p1)
        if pos is None or _patch_pos_fused(pos, img, N, E):
            return node.apply(img, weight, bias, pos)
        return node.apply(img, weight, bias, None) + pos
    y = torch.nn.functional.conv2d(img, weight, bias, stride=tuple(weight.shape[2:])).flatten(2).transpose(1, 2)
    return y if pos is None else y + pos
