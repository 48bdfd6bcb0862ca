"""CPU tests of the planar transform's host side: the latitude DFT table (``mk_latdft_table``) against numpy float64, the
exported symbols and their argument checks, and the modules on CPU tensors, which stay on the torch formulation bit for bit.
No kernel launches here."""
import math
import os
import re

import numpy as np
import pytest
import torch

from makani_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = [(16, 10), (64, 21), (33, 33), (721, 240)]
NEW_SYMBOLS = ("mk_latdft_table_len", "mk_latdft_table", "mk_latdft_fwd", "mk_latdft_inv", "mk_irfft_sums_ws")
_P = 4096      # non-null, 16-byte aligned, never dereferenced: validation returns before any launch


def _pad4(n):
    return (n + 3) // 4 * 4


def _freqs(nlat, lmax):
    """Kept rows of the full DFT: the first ceil(lmax / 2) and the last floor(lmax / 2), as ``RealFFT2`` concatenates them."""
    hi = math.ceil(lmax / 2)
    return np.array([l if l < hi else nlat - lmax + l for l in range(lmax)], dtype=np.int64)


def _parts(nlat, lmax):
    t = ops.latdft_table(nlat, lmax).numpy()
    kp, lp = _pad4(nlat), _pad4(lmax)
    assert t.size == 2 * lmax * kp + 2 * nlat * lp == _lib.load().mk_latdft_table_len(nlat, lmax)
    fwd = t[: 2 * lmax * kp].reshape(2, lmax, kp)
    inv = t[2 * lmax * kp:].reshape(2, nlat, lp)
    return fwd, inv


@pytest.mark.parametrize("nlat,lmax", GRIDS)
def test_table_matches_numpy_float64(nlat, lmax):
    fwd, inv = _parts(nlat, lmax)
    f = _freqs(nlat, lmax)
    k = np.arange(nlat, dtype=np.int64)
    ang = 2.0 * np.pi * ((f[:, None] * k[None, :]) % nlat).astype(np.float64) / nlat
    want = np.stack([np.cos(ang), np.sin(ang)]) / np.sqrt(float(nlat))       # W = cos - i sin
    # fp32 roundings of values no larger than 1 / sqrt(nlat)
    bound = 2.0 ** -24 / math.sqrt(nlat)
    assert np.abs(fwd[:, :, :nlat].astype(np.float64) - want).max() <= bound
    assert np.abs(inv[:, :, :lmax].astype(np.float64) - want.transpose(0, 2, 1)).max() <= bound
    # the inverse half is the transpose of the analysis half, entry for entry
    assert np.array_equal(inv[:, :, :lmax], fwd[:, :, :nlat].transpose(0, 2, 1))
    # padding to 16-byte groups is zero
    assert np.all(fwd[:, :, nlat:] == 0) and np.all(inv[:, :, lmax:] == 0)


@pytest.mark.parametrize("nlat,lmax", [(16, 10), (64, 21), (33, 33), (12, 12), (9, 2), (9, 3)])
def test_frequency_map_is_the_modules_truncation(nlat, lmax):
    """The table's rows are the rows ``RealFFT2`` keeps: applying it to a column equals the truncated ortho FFT (odd and even lmax)."""
    from makani_amd.layers import RealFFT2
    fwd, _ = _parts(nlat, lmax)
    w = fwd[0, :, :nlat].astype(np.float64) - 1j * fwd[1, :, :nlat].astype(np.float64)
    rng = np.random.default_rng(nlat * 100 + lmax)
    x = rng.standard_normal(nlat) + 1j * rng.standard_normal(nlat)
    full = np.fft.fft(x, norm="ortho")
    m = RealFFT2(nlat, 8, lmax=lmax, mmax=5)
    want = np.concatenate([full[: m.lmax_high], full[nlat - m.lmax_low:]]) if m.lmax_low else full[: m.lmax_high]
    assert np.abs(w @ x - want).max() < 1e-6
    assert list(_freqs(nlat, lmax)[: m.lmax_high]) == list(range(m.lmax_high))
    assert list(_freqs(nlat, lmax)[m.lmax_high:]) == list(range(nlat - m.lmax_low, nlat))


def test_library_exports_the_new_symbols():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "makani_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(mk_[a-z0-9_]+)\s*\(", text))
    for n in NEW_SYMBOLS:
        assert n in declared, f"{n} is not declared in include/makani_amd.h"
        assert hasattr(lib, n) and n in _lib.SIGNATURES


@pytest.mark.parametrize("nlat,lmax", [(1, 1), (16, 1), (16, 17), (0, 0)])
def test_table_rejects_bad_sizes(nlat, lmax):
    lib = _lib.load()
    assert lib.mk_latdft_table_len(nlat, lmax) == 0
    buf = np.zeros(64, dtype=np.float32)
    assert lib.mk_latdft_table(nlat, lmax, buf.ctypes.data) == 1 and lib.mk_last_error()
    with pytest.raises(ValueError):
        ops.latdft_table(nlat, lmax)


def test_table_rejects_null():
    assert _lib.load().mk_latdft_table(16, 10, None) == 1


LAUNCH_REJECTED = [
    dict(a=None), dict(t=None), dict(c=None),                   # null pointers
    dict(t=_P + 4), dict(a=_P + 4), dict(c=_P + 2),             # misaligned table / operands
    dict(nlat=1), dict(lmax=1), dict(lmax=17), dict(ncols=0),   # sizes
    dict(ncols=1 << 23),                                        # 33 * 2 * ncols * 4 bytes >= 2^31
    dict(nlat=20000, lmax=20000),                               # table over 2^31 bytes
]


@pytest.mark.parametrize("name", ["mk_latdft_fwd", "mk_latdft_inv"])
@pytest.mark.parametrize("bad", LAUNCH_REJECTED, ids=["-".join(f"{k}={v}" for k, v in b.items()) for b in LAUNCH_REJECTED])
def test_launchers_reject_bad_arguments(name, bad):
    lib = _lib.load()
    a = dict(dict(a=_P, t=_P, c=_P, nlat=16, lmax=10, ncols=12), **bad)
    lib.mk_quadrature(7, 10, 0, 0)      # leaves another function's message behind
    assert getattr(lib, name)(a["a"], a["t"], a["c"], a["nlat"], a["lmax"], a["ncols"], None) == 1
    msg = lib.mk_last_error()
    assert msg and b"unknown grid" not in msg


def test_irfft_sums_ws_rejects_bad_arguments():
    lib = _lib.load()
    good = [_P, _P, 0, _P, 48, 4, 480, 33, 1.0, 1.0, 1.0, 0, 0, 0, _P, _P]
    for pos, val in ((15, None), (14, None), (6, 64), (11, 2)):      # no workspace, no accumulators, a length without split kernels, layout
        a = list(good)
        a[pos] = val
        assert lib.mk_irfft_sums_ws(*a, None) == 1 and lib.mk_last_error()


def test_ops_refuse_cpu_tensors():
    tab = ops.latdft_table(16, 10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.lat_dft(torch.zeros(16, 3, 2, dtype=torch.complex64), tab, 10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.lat_idft(torch.zeros(10, 3, 2, dtype=torch.complex64), tab, 16)


@pytest.mark.parametrize("nlat,nlon,lmax,mmax", [(16, 32, 10, 9), (33, 64, 33, 33), (12, 9, 5, 3), (8, 16, 1, 4)])
@pytest.mark.parametrize("knob", [None, "hip", "torch"])
def test_cpu_modules_are_the_torch_formulation(monkeypatch, nlat, nlon, lmax, mmax, knob):
    """CPU tensors never reach a kernel, whatever ``MK_PLANAR_FFT`` says: bit-identical to ``_forward_torch``, fp32 and fp64,
    for sizes with (even nlon, lmax >= 2) and without buffers."""
    from makani_amd.layers import InverseRealFFT2, RealFFT2
    if knob is None:
        monkeypatch.delenv("MK_PLANAR_FFT", raising=False)
    else:
        monkeypatch.setenv("MK_PLANAR_FFT", knob)
    f, fi = RealFFT2(nlat, nlon, lmax=lmax, mmax=mmax), InverseRealFFT2(nlat, nlon, lmax=lmax, mmax=mmax)
    assert list(f.state_dict()) == [] and list(fi.state_dict()) == []
    has = nlon % 2 == 0 and lmax >= 2
    assert ("dft_table" in dict(f.named_buffers())) == has and ("twiddles" in dict(fi.named_buffers())) == has
    torch.manual_seed(0)
    for dt in (torch.float32, torch.float64):
        x = torch.randn(2, 3, nlat, nlon, dtype=dt)
        y = f(x)
        assert torch.equal(y, f._forward_torch(x))
        if lmax >= 2:       # (lmax = 1: the reference's `y[-0:]` keeps every row -- whatever it does, the module does the same)
            assert tuple(y.shape) == (2, 3, f.lmax, f.mmax)
        assert torch.equal(fi(y), fi._forward_torch(y))


def test_fft_scale_factors_passed_to_the_launches(monkeypatch):
    """Without a scale ``ops.rfft`` / ``ops.irfft`` hand the launches the SHT's factors, forward and backward, as before; with one,
    that factor and the adjoint triples of the header (``mk_irfft(s, s / 2, s)``, ``mk_rfft(s, 2 s, s)``)."""
    seen = []

    def fake_rfft(x, tw, mmax, s0, sm, sh, kmajor=False):
        seen.append(("rfft", s0, sm, sh))
        return torch.zeros(x.shape[1], mmax, x.shape[0], dtype=torch.complex64)

    def fake_irfft(xf, tw, nlon, s0, sm, sh, out_dtype=torch.float32, kmajor=False):
        seen.append(("irfft", s0, sm, sh))
        return torch.zeros(xf.shape[2], xf.shape[0], nlon)

    monkeypatch.setattr(ops, "rfft_raw", fake_rfft)
    monkeypatch.setattr(ops, "irfft_raw", fake_irfft)
    n, tw = 32, ops.fft_twiddles(32)
    for scale in (None, 1.0 / math.sqrt(n)):
        seen.clear()
        x = torch.zeros(2, 4, n, requires_grad=True)
        ops.rfft(x, tw, 9, True, scale=scale).sum().abs().backward()
        xf = torch.zeros(4, 9, 2, dtype=torch.complex64, requires_grad=True)
        ops.irfft(xf, tw, n, torch.float32, True, scale=scale).sum().backward()
        if scale is None:
            a, b = 2.0 * math.pi / n, math.pi / n
            want = [("rfft", a, a, a), ("irfft", a, b, a), ("irfft", 1.0, 1.0, 1.0), ("rfft", 1.0, 2.0, 1.0)]
        else:
            want = [("rfft", scale, scale, scale), ("irfft", scale, 0.5 * scale, scale), ("irfft", scale, scale, scale),
                    ("rfft", scale, 2.0 * scale, scale)]
        assert seen == want      # exact equality: the same Python floats
