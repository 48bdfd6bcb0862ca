"""CPU tests of the diagonal filter on the private spectrum: the knob ``MK_SPEC_DIAG``, the path CPU tensors keep, and the
argument checks of ``mk_spec_diag_fwd`` / ``_dgrad`` / ``_wgrad`` (code 1 and a message before any launch).  No kernel runs here."""
import pytest
import torch

from makani_amd import _lib, ops
from makani_amd.layers import InverseRealFFT2, RealFFT2
from makani_amd.spectral_convolution import SpectralConv

ENTRY_POINTS = ["mk_spec_diag_fwd", "mk_spec_diag_dgrad", "mk_spec_diag_wgrad"]


def _conv():
    torch.manual_seed(5)
    return SpectralConv(RealFFT2(33, 64, lmax=9, mmax=9), InverseRealFFT2(16, 32, lmax=9, mmax=9), 4, 6, operator_type="diagonal")


def _run(conv, x, gy, gr):
    xd = x.clone().requires_grad_(True)
    conv.zero_grad()
    y, r = conv(xd)
    (y * gy).sum().add((r * gr).sum()).backward()
    return y.detach(), r.detach(), xd.grad.detach(), conv.weight.grad.detach().clone()


def test_knob_values(monkeypatch):
    monkeypatch.delenv("MK_SPEC_DIAG", raising=False)
    assert ops.spec_diag_fused() is False           # opt-in: the default is the public path
    monkeypatch.setenv("MK_SPEC_DIAG", "public")
    assert ops.spec_diag_fused() is False
    monkeypatch.setenv("MK_SPEC_DIAG", "fused")
    assert ops.spec_diag_fused() is True
    monkeypatch.setenv("MK_SPEC_DIAG", "hip")
    with pytest.raises(ValueError, match="MK_SPEC_DIAG"):
        ops.spec_diag_fused()


def test_invalid_knob_raises_on_every_call(monkeypatch):
    """The knob is read and validated by every call of a diagonal ``SpectralConv``, CPU input included."""
    conv, x = _conv(), torch.randn(1, 4, 33, 64)
    conv(x)
    monkeypatch.setenv("MK_SPEC_DIAG", "Fused")
    with pytest.raises(ValueError, match="MK_SPEC_DIAG"):
        conv(x)
    monkeypatch.setenv("MK_SPEC_DIAG", "fused")
    conv(x)


def test_cpu_tensors_keep_the_generic_path_bit_for_bit(monkeypatch):
    conv = _conv()
    g = torch.Generator().manual_seed(6)
    x, gy, gr = torch.randn(2, 4, 33, 64, generator=g), torch.randn(2, 6, 16, 32, generator=g), torch.randn(2, 4, 16, 32, generator=g)
    monkeypatch.delenv("MK_SPEC_DIAG", raising=False)
    want = _run(conv, x, gy, gr)
    monkeypatch.setenv("MK_SPEC_DIAG", "fused")
    got = _run(conv, x, gy, gr)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_cpu_tensors_never_reach_a_kernel():
    c = torch.zeros(4, 4, 2, dtype=torch.complex64)
    w = torch.zeros(2, 3, 4, 4, dtype=torch.complex64)
    assert not ops.spec_diag_supported(c, w)
    for call in (lambda: ops.spec_diag(c, w, 1), lambda: ops.spec_diag_fwd_raw(c, w, 1),
                 lambda: ops.spec_diag_dgrad_raw(torch.zeros(4, 4, 3, dtype=torch.complex64), w, 1),
                 lambda: ops.spec_diag_wgrad_raw(c, torch.zeros(4, 4, 3, dtype=torch.complex64), 1)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


_P = 4096      # a non-null, 16-byte aligned address that is never dereferenced: validation returns before any launch
_DEFAULTS = dict(a=_P, b=_P, out=_P, lloc=4, mloc=6, batch=2, cin=3, cout=5, l_off=0, m_off=0, dense=0)
REJECTED = [
    dict(a=None), dict(b=None), dict(out=None),                                     # a null pointer
    dict(a=_P + 4), dict(out=_P + 4),                                               # not aligned to a complex64
    dict(lloc=0), dict(mloc=-1), dict(batch=0), dict(cin=0), dict(cout=-3),         # a non-positive size
    dict(l_off=-1), dict(dense=2),
    dict(cin=1 << 30), dict(cout=2400, cin=200),                                    # beyond the LDS rows / cin * cout in int
    dict(batch=1 << 20),                                                            # batch * channels beyond int
    dict(l_off=2147483647 - 2), dict(m_off=2147483647 - 3),                         # global degree / order beyond int
    dict(lloc=1 << 30, mloc=1 << 20),                                               # more position runs than a grid holds
]


@pytest.mark.parametrize("bad", REJECTED, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_entry_points_reject_bad_input(name, bad):
    lib = _lib.load()
    a = dict(_DEFAULTS, **bad)
    lib.mk_quadrature(7, 10, 0, 0)      # leaves a message of another function behind: the one below must replace it
    rc = getattr(lib, name)(a["a"], a["b"], a["out"], a["lloc"], a["mloc"], a["batch"], a["cin"], a["cout"], a["l_off"], a["m_off"],
                            a["dense"], None)
    assert rc == 1
    msg = lib.mk_last_error()
    assert msg and msg.startswith(name.encode() + b": ") and b"unknown grid" not in msg
