"""GPU tests of ``SpectralConv(operator_type="diagonal")`` and the FNO network with ``MK_SPEC_DIAG=fused`` (``ops.spec_diag`` on the
private spectrum between ``forward_packed`` and ``inverse_packed``) against the same modules at ``public`` (the generic path:
the modules' public ``forward``, ``ops.diag_contract``, the public inverse).

Criterion of the module comparisons: ``kernel_checks.row_rel <= 1e-5`` on every row, the project's stated fp32 criterion; both
sides are fp32 paths of the same transforms.  Every test prints its figures before it asserts.
"""
import numpy as np
import pytest
import torch

import kernel_checks as kc

pytestmark = pytest.mark.gpu

TOL = 1e-5


@pytest.fixture(autouse=True)
def _hip_planar(monkeypatch):
    monkeypatch.setenv("MK_PLANAR_FFT", "hip")
    monkeypatch.delenv("MK_SPEC_DIAG", raising=False)


def _pair(kind, inp, out, modes, dev):
    from makani_amd.layers import InverseRealFFT2, RealFFT2
    from makani_amd.sht import InverseRealSHT, RealSHT
    L, M = modes
    if kind == "planar":
        return RealFFT2(*inp, lmax=L, mmax=M).to(dev), InverseRealFFT2(*out, lmax=L, mmax=M).to(dev)
    return RealSHT(*inp, lmax=L, mmax=M, grid="equiangular").to(dev), InverseRealSHT(*out, lmax=L, mmax=M, grid="equiangular").to(dev)


def _conv(kind, inp, out, modes, dev, cin=4, cout=6, **kw):
    from makani_amd.spectral_convolution import SpectralConv
    torch.manual_seed(3)
    return SpectralConv(*_pair(kind, inp, out, modes, dev), cin, cout, operator_type="diagonal", **kw).to(dev)


def _run(conv, x, gy, gr):
    xd = x.clone().requires_grad_(True)
    conv.zero_grad()
    y, r = conv(xd)
    (y * gy).sum().add((r * gr).sum()).backward()
    return y.detach(), r.detach(), xd.grad.detach(), conv.weight.grad.detach().clone()


class _count_launches:
    """Counts, inside the block, the launches of the layout passes (``spec_unpack`` / ``spec_pack``), of the public contraction
    (``mk_diag_*``) and of the kernels on the private spectrum (``mk_spec_diag_*``), forward and backward alike."""
    NAMES = ("spec_unpack_raw", "spec_pack_raw", "_diag_launch", "_spec_diag_launch")

    def __enter__(self):
        from makani_amd import ops
        self.ops, self.saved, self.n = ops, {k: getattr(ops, k) for k in self.NAMES}, {k: 0 for k in self.NAMES}

        def wrap(name, fn):
            def inner(*a, **k):
                self.n[name] += 1
                return fn(*a, **k)
            return inner
        for k, fn in self.saved.items():
            setattr(ops, k, wrap(k, fn))
        return self.n

    def __exit__(self, *exc):
        for k, fn in self.saved.items():
            setattr(self.ops, k, fn)
        return False


CONVS = [
    ("planar", (16, 32), (16, 32), (9, 9)),
    ("planar", (33, 64), (16, 32), (9, 9)),         # scaled residual: synthesised from the private spectrum
    ("sht", (17, 32), (17, 32), (8, 8)),
]


def _operands(inp, out, scaled, dev, cin=4, cout=6, B=2):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, cin, *inp, generator=g).to(dev)
    gy = torch.randn(B, cout, *out, generator=g).to(dev)
    gr = torch.randn(B, cin, *(out if scaled else inp), generator=g).to(dev)
    return x, gy, gr


@pytest.mark.parametrize("kind,inp,out,modes", CONVS, ids=[f"{c[0]}-{c[1][0]}x{c[1][1]}-{c[2][0]}x{c[2][1]}" for c in CONVS])
def test_fused_matches_public(dev, monkeypatch, kind, inp, out, modes):
    conv = _conv(kind, inp, out, modes, dev)
    x, gy, gr = _operands(inp, out, conv.scale_residual, dev)
    monkeypatch.setenv("MK_SPEC_DIAG", "fused")
    with _count_launches() as n:
        fused = _run(conv, x, gy, gr)
    # the fused run: no layout pass, no public contraction; one forward, one data-gradient and one weight-gradient launch
    assert n["spec_unpack_raw"] == 0 and n["spec_pack_raw"] == 0 and n["_diag_launch"] == 0 and n["_spec_diag_launch"] == 3, n
    monkeypatch.setenv("MK_SPEC_DIAG", "public")
    with _count_launches() as n:
        public = _run(conv, x, gy, gr)
    assert n["_spec_diag_launch"] == 0 and n["_diag_launch"] == 3 and n["spec_unpack_raw"] > 0 and n["spec_pack_raw"] > 0, n
    errs = {}
    for name, a, b in zip(("y", "residual", "gx", "gw"), fused, public):
        assert a.shape == b.shape and a.dtype == b.dtype
        if name == "gw" and kind == "sht":
            # rows (i, o, l) of the weight gradient: exact zeros on both sides where l < m, data where m <= l
            assert torch.equal(a == 0, b == 0)
        errs[name] = float(kc.row_rel(a.cpu().numpy(), b.cpu().numpy().astype(np.complex128 if b.is_complex() else np.float64)).max())
    print(f"[spec_diag] SpectralConv {kind} {inp}->{out}: " + "  ".join(f"{k}={v:.3e}" for k, v in errs.items()))
    assert max(errs.values()) <= TOL


@pytest.mark.parametrize("kind,inp,modes", [("planar", (8, 480), (6, 6)), ("sht", (9, 480), (8, 8))])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_row_statistics_of_the_returned_rows(dev, monkeypatch, kind, inp, modes, dtype):
    """``want_row_sums=True`` on the fused path hands over the inverse FFT's statistics (``mk_irfft_sums``): float64 sums of the
    returned rows within the limit of ``tests/test_kernels_gpu.py::test_irfft_row_statistics`` (2e-6 of sum |x| resp. sum x^2).
    At ``public`` the path cannot deliver them: None."""
    conv = _conv(kind, inp, inp, modes, dev)
    x = torch.randn(2, 4, *inp, generator=torch.Generator().manual_seed(8)).to(dev).to(dtype)
    monkeypatch.setenv("MK_SPEC_DIAG", "public")
    with torch.no_grad():
        assert conv(x, want_row_sums=True)[2] is None
    monkeypatch.setenv("MK_SPEC_DIAG", "fused")
    with torch.no_grad():
        y, _, sums = conv(x, want_row_sums=True)
    assert y.dtype == dtype and sums is not None and sums.dtype == torch.float64 and tuple(sums.shape) == (2 * 6, 2)
    yd = y.double().view(2 * 6, *inp)
    sq = (yd * yd).sum(dim=(1, 2))
    want, scale = torch.stack([yd.sum(dim=(1, 2)), sq], dim=1), torch.stack([yd.abs().sum(dim=(1, 2)), sq], dim=1)
    err = ((sums - want).abs() / scale).max().item()
    print(f"[spec_diag] row sums {kind} {dtype}: {err:.3e}")
    assert err < 2e-6


@pytest.mark.parametrize("knob", [None, "public"])
@pytest.mark.parametrize("kind,inp,out,modes", CONVS[1:], ids=["planar-scaled", "sht"])
def test_default_is_the_generic_composition(dev, monkeypatch, knob, kind, inp, out, modes):
    """Knob unset or ``public``: output and gradients equal, bit for bit, the explicit composition of the generic path."""
    from makani_amd import ops
    if knob is not None:
        monkeypatch.setenv("MK_SPEC_DIAG", knob)
    conv = _conv(kind, inp, out, modes, dev)
    x, gy, gr = _operands(inp, out, conv.scale_residual, dev)
    got = _run(conv, x, gy, gr)

    xd = x.clone().requires_grad_(True)
    conv.zero_grad()
    c = conv.forward_transform(xd).contiguous()
    r = conv.inverse_transform(c) if conv.scale_residual else xd
    y = conv.inverse_transform(ops.diag_contract(c, conv.weight).contiguous())
    (y * gy).sum().add((r * gr).sum()).backward()
    want = (y.detach(), r.detach(), xd.grad.detach(), conv.weight.grad.detach())
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_factorized_dense_follows(dev, monkeypatch):
    """``FactorizedSpectralConv`` with ``ComplexDense`` takes the same path through ``_weight_tensor()``."""
    from makani_amd.spectral_convolution import FactorizedSpectralConv
    torch.manual_seed(4)
    conv = FactorizedSpectralConv(*_pair("planar", (16, 32), (16, 32), (9, 9), dev), 4, 6, operator_type="diagonal").to(dev)
    x = torch.randn(2, 4, 16, 32, generator=torch.Generator().manual_seed(9)).to(dev)
    monkeypatch.setenv("MK_SPEC_DIAG", "fused")
    with _count_launches() as n, torch.no_grad():
        fused = conv(x)[0]
    assert n["_spec_diag_launch"] == 1 and n["_diag_launch"] == 0 and n["spec_pack_raw"] == 0
    monkeypatch.setenv("MK_SPEC_DIAG", "public")
    with torch.no_grad():
        public = conv(x)[0]
    assert float(kc.row_rel(fused.cpu().numpy(), public.cpu().numpy().astype(np.float64)).max()) <= TOL


def test_other_inputs_keep_the_generic_path(dev, monkeypatch):
    """fp64 input, or a separable layer, with the knob at ``fused``: today's path (no launch on the private spectrum)."""
    monkeypatch.setenv("MK_SPEC_DIAG", "fused")
    conv = _conv("planar", (16, 32), (16, 32), (9, 9), dev)
    x = torch.randn(2, 4, 16, 32, generator=torch.Generator().manual_seed(10)).to(dev)
    with _count_launches() as n, torch.no_grad():
        y = conv(x.double())[0]
    assert n["_spec_diag_launch"] == 0 and n["_diag_launch"] == 1 and y.dtype == torch.float64
    assert not conv.takes_spectral_mix()


def test_fno_net_step_matches_public(dev, monkeypatch):
    """A training step of a diagonal FNO under bf16 autocast: loss and every parameter gradient of the ``fused`` run against the
    ``public`` run, within the limit of ``tests/test_fft2_gpu.py::test_fno_net_step_matches_torch_path`` (relative L2, 1e-5)."""
    from makani_amd.sfnonet import FourierNeuralOperatorNet
    torch.manual_seed(11)
    net = FourierNeuralOperatorNet(inp_shape=(32, 64), out_shape=(32, 64), inp_chans=3, out_chans=3, embed_dim=4, num_layers=2,
                                   operator_type="diagonal", scale_factor=2, max_modes=(8, 8)).to(dev)
    g = torch.Generator().manual_seed(12)
    x, tar = torch.randn(2, 3, 32, 64, generator=g).to(dev), torch.randn(2, 3, 32, 64, generator=g).to(dev)

    def rel(a, b):
        a, b = (t.to(torch.complex128) if t.is_complex() else t.double() for t in (a, b))
        return (torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b)).item()

    def step():
        net.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = ((net(x).float() - tar) ** 2).mean()
        loss.backward()
        return [loss.detach()] + [p.grad.detach().clone() for p in net.parameters() if p.grad is not None]

    monkeypatch.setenv("MK_SPEC_DIAG", "fused")
    with _count_launches() as n:
        fused = step()
    assert n["_spec_diag_launch"] == 6 and n["_diag_launch"] == 0, n         # two layers: forward, data and weight gradient
    monkeypatch.setenv("MK_SPEC_DIAG", "public")
    with _count_launches() as n:
        public = step()
    assert n["_spec_diag_launch"] == 0 and n["_diag_launch"] == 6, n
    assert len(fused) == len(public) > 10
    errs = [rel(a, b) for a, b in zip(fused, public)]
    print(f"[spec_diag] FNO step: loss={errs[0]:.3e} worst parameter gradient={max(errs[1:]):.3e}")
    assert max(errs) < TOL
