"""GPU tests of the planar transform on the HIP path (``MK_PLANAR_FFT=hip``): the HIP real FFT with scale 1 / sqrt(nlon) and the
latitude DFT on the bf16x3 MFMA engine (``mk_latdft_fwd`` / ``mk_latdft_inv``), under ``RealFFT2`` / ``InverseRealFFT2``,
``SpectralConv`` and the FNO network.

Truth is the module's own torch formulation (``_forward_torch``) on the CPU in float64.  The error measure and the bound are
the reference's (``tests/distributed/tests_fft.py``): the mean over (b, c) of the per-field relative L2 error, at most 1e-6,
for outputs and for input gradients.  A six-product bf16x3 contraction of length 16 ... 721 was emulated at 4e-8 ... 1.3e-7 in
this measure and fp32 ``torch.fft`` gives 6e-8 ... 2e-7 on the same inputs, so the bound leaves roughly 8x.  Every test prints
its figures (``-s`` shows them) before it asserts.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND = 1e-6          # the reference's tolerance for DistributedRealFFT2 / DistributedInverseRealFFT2
TOL = 1e-5            # file-wide tolerance of tests/test_model_gpu.py (module stack against another evaluation of itself)

# nlat, nlon, lmax, mmax, B, C
CASES = [
    (16, 32, 10, 9, 2, 3),          # ref_fft2.npz (the reference's own numbers)
    (64, 96, 21, 17, 2, 6),         # odd lmax, truncation
    (33, 64, 33, 33, 1, 5),         # no truncation, odd nlat, K not a multiple of 4
    (91, 180, 70, 61, 1, 4),        # more than one row tile, ragged column tile
    (361, 720, 361, 361, 1, 2),     # the reference's test shape
    (256, 512, 256, 257, 2, 4),     # the reference's test shape
    (30, 480, 20, 21, 1, 8),        # split FFT kernels: bf16 rows and row sums
]
IDS = ["x".join(str(v) for v in c) for c in CASES]
SPLIT_CASE = CASES[-1]


def field_err(a, b):
    """mean over the leading dims of ||a - b||_2 / ||b||_2 over the last two (the measure of the reference's tests_fft.py)."""
    a, b = a.detach().cpu(), b.detach().cpu()
    cplx = a.is_complex() or b.is_complex()
    a = a.to(torch.complex128) if cplx else a.double()
    b = b.to(torch.complex128) if cplx else b.double()
    return torch.mean(torch.linalg.vector_norm(a - b, dim=(-2, -1)) / torch.linalg.vector_norm(b, dim=(-2, -1))).item()


def rel(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    cplx = a.is_complex() or b.is_complex()
    a = a.to(torch.complex128) if cplx else a.double()
    b = b.to(torch.complex128) if cplx else b.double()
    return (torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b)).item()


@pytest.fixture(autouse=True)
def _hip_path(monkeypatch):
    monkeypatch.setenv("MK_PLANAR_FFT", "hip")


_truth = {}


def truth(case):
    """Inputs, cotangents and the float64 CPU results of both modules for one case: computed once, shared, never modified."""
    if case not in _truth:
        from makani_amd.layers import InverseRealFFT2, RealFFT2
        nlat, nlon, lmax, mmax, B, C = case
        g = torch.Generator().manual_seed(1000 + nlat)
        x = torch.randn(B, C, nlat, nlon, generator=g)
        gy = torch.complex(torch.randn(B, C, lmax, mmax, generator=g), torch.randn(B, C, lmax, mmax, generator=g))
        c = torch.complex(torch.randn(B, C, lmax, mmax, generator=g), torch.randn(B, C, lmax, mmax, generator=g))
        gx = torch.randn(B, C, nlat, nlon, generator=g)
        f, fi = RealFFT2(nlat, nlon, lmax=lmax, mmax=mmax), InverseRealFFT2(nlat, nlon, lmax=lmax, mmax=mmax)
        x64 = x.double().requires_grad_(True)
        y64 = f._forward_torch(x64)
        y64.backward(gy.to(torch.complex128))
        c64 = c.to(torch.complex128).requires_grad_(True)
        xi64 = fi._forward_torch(c64)
        xi64.backward(gx.double())
        _truth[case] = dict(x=x, gy=gy, c=c, gx=gx, y=y64.detach(), x_grad=x64.grad, xi=xi64.detach(), c_grad=c64.grad)
    return _truth[case]


def modules(case, dev):
    from makani_amd.layers import InverseRealFFT2, RealFFT2
    nlat, nlon, lmax, mmax = case[:4]
    return RealFFT2(nlat, nlon, lmax=lmax, mmax=mmax).to(dev), InverseRealFFT2(nlat, nlon, lmax=lmax, mmax=mmax).to(dev)


class _count_launches:
    """Counts the latitude DFT launches (``ops.lat_dft_raw`` / ``ops.lat_idft_raw``, forward and backward alike) inside the block:
    fp32 ``torch.fft`` meets the bounds of this file too, so a test of the HIP path also shows that the kernels ran."""

    def __enter__(self):
        from makani_amd import ops
        self.ops, self.saved, self.n = ops, (ops.lat_dft_raw, ops.lat_idft_raw), dict(lat_dft=0, lat_idft=0)

        def wrap(name, fn):
            def inner(*a, **k):
                self.n[name] += 1
                return fn(*a, **k)
            return inner
        ops.lat_dft_raw, ops.lat_idft_raw = wrap("lat_dft", self.saved[0]), wrap("lat_idft", self.saved[1])
        return self.n

    def __exit__(self, *exc):
        self.ops.lat_dft_raw, self.ops.lat_idft_raw = self.saved
        return False


def _report(name, case, **figs):
    print(f"[fft2] {name} {'x'.join(str(v) for v in case)}: " + "  ".join(f"{k}={v:.3e}" for k, v in figs.items()))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_and_input_gradient(dev, case):
    t = truth(case)
    f, _ = modules(case, dev)
    x = t["x"].to(dev).requires_grad_(True)
    assert f.hip_ready(x)
    with _count_launches() as n:
        y = f(x)
    assert n["lat_dft"] == 1 and n["lat_idft"] == 0       # the kernels ran, not torch.fft
    assert y.dtype == torch.complex64 and tuple(y.shape) == tuple(t["y"].shape)
    y.backward(t["gy"].to(dev))
    e_y, e_g = field_err(y, t["y"]), field_err(x.grad, t["x_grad"])
    with torch.no_grad():
        e_t = field_err(f._forward_torch(t["x"].to(dev)), t["y"])
    _report("RealFFT2", case, out=e_y, grad=e_g, torch_fft_fp32=e_t)
    assert e_y <= BOUND and e_g <= BOUND


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_inverse_and_input_gradient(dev, case):
    t = truth(case)
    _, fi = modules(case, dev)
    c = t["c"].to(dev).requires_grad_(True)
    assert fi.hip_ready(c)
    with _count_launches() as n:
        xi = fi(c)
    assert n["lat_idft"] == 1 and n["lat_dft"] == 0
    assert xi.dtype == torch.float32 and tuple(xi.shape) == tuple(t["xi"].shape)
    xi.backward(t["gx"].to(dev))
    e_x, e_g = field_err(xi, t["xi"]), field_err(c.grad, t["c_grad"])
    with torch.no_grad():
        e_t = field_err(fi._forward_torch(t["c"].to(dev)), t["xi"])
    _report("InverseRealFFT2", case, out=e_x, grad=e_g, torch_fft_fp32=e_t)
    assert e_x <= BOUND and e_g <= BOUND


def test_reference_golden(dev, golden_dir):
    """``ref_fft2.npz`` was written by the reference's own ``layers.py``: forward of ``x`` against ``y``, inverse of ``y`` against ``xi``."""
    g = np.load(os.path.join(golden_dir, "ref_fft2.npz"))
    f, fi = modules(CASES[0], dev)
    with _count_launches() as n:
        y = f(torch.from_numpy(g["x"]).to(dev))
        xi = fi(torch.from_numpy(g["y"]).to(dev))
    assert n["lat_dft"] == 1 and n["lat_idft"] == 1
    e_y, e_x = field_err(y, torch.from_numpy(g["y"])), field_err(xi, torch.from_numpy(g["xi"]))
    _report("golden", CASES[0], forward=e_y, inverse=e_x)
    assert e_y <= BOUND and e_x <= BOUND


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_latitude_kernels_adjoint_and_round_trip(dev, case):
    """``<lat_dft x, y> = <x, lat_idft y>`` to 1e-6 relative; without truncation the two are inverse to each other."""
    from makani_amd import ops
    nlat, nlon, lmax, mmax, B, C = case
    g = torch.Generator().manual_seed(77 + nlat)
    tab = ops.latdft_table(nlat, lmax).to(dev)
    x = torch.complex(torch.randn(nlat, mmax, B * C, generator=g), torch.randn(nlat, mmax, B * C, generator=g)).to(dev)
    y = torch.complex(torch.randn(lmax, mmax, B * C, generator=g), torch.randn(lmax, mmax, B * C, generator=g)).to(dev)
    ax, aty = ops.lat_dft(x, tab, lmax), ops.lat_idft(y, tab, nlat)
    assert tuple(ax.shape) == (lmax, mmax, B * C) and tuple(aty.shape) == (nlat, mmax, B * C)
    lhs = torch.vdot(y.cpu().to(torch.complex128).flatten(), ax.cpu().to(torch.complex128).flatten())
    rhs = torch.vdot(aty.cpu().to(torch.complex128).flatten(), x.cpu().to(torch.complex128).flatten())
    e_adj = (abs(lhs - rhs) / abs(lhs)).item()
    figs = dict(adjoint=e_adj)
    if lmax == nlat:
        figs["round_trip"] = rel(ops.lat_idft(ax, tab, nlat), x)
    _report("lat_dft", case, **figs)
    assert e_adj <= 1e-6
    if lmax == nlat:
        assert figs["round_trip"] <= 1e-6


def test_packed_interfaces_bf16_rows(dev):
    """The split FFT kernels under the packed interfaces: bf16 input rows, bf16 output rows within one bf16 rounding of the fp32 rows."""
    from makani_amd import ops
    case = SPLIT_CASE
    nlat, nlon, lmax, mmax, B, C = case
    t = truth(case)
    f, fi = modules(case, dev)
    assert ops.irfft_sums_supported(nlon, mmax)
    x3 = t["x"].to(dev).view(B * C, nlat, nlon)
    c = f.forward_packed(x3)
    assert tuple(c.shape) == (lmax, mmax, B * C) and c.dtype == torch.complex64
    want = t["y"].reshape(B * C, lmax, mmax).permute(1, 2, 0)
    e_c = rel(c, want)
    # bf16 input rows: the transform of the rounded field, exactly as the fp32 kernel sees the same values
    xb = x3.to(torch.bfloat16)
    e_b = rel(f.forward_packed(xb), f.forward_packed(xb.float()))
    cp = ops.spec_pack(t["c"].to(dev).reshape(B * C, lmax, mmax), mmax, 0)
    x32 = fi.inverse_packed(cp)
    x16 = fi.inverse_packed(cp, torch.bfloat16)
    assert x32.dtype == torch.float32 and x16.dtype == torch.bfloat16 and tuple(x32.shape) == (B * C, nlat, nlon)
    e_x = field_err(x32, t["xi"].reshape(B * C, nlat, nlon))
    e_16 = rel(x16.float(), x32)
    _report("packed", case, spectrum=e_c, bf16_in=e_b, rows=e_x, bf16_rows=e_16)
    assert e_c <= BOUND and e_x <= BOUND and e_b <= BOUND
    assert e_16 <= 2.0 ** -9 + 1e-6
    # (x, sums) / (x, None) conventions of InverseRealSHT.inverse_packed
    xs, sums = fi.inverse_packed(cp, torch.bfloat16, True)
    assert torch.equal(xs, x16) and sums.dtype == torch.float64 and tuple(sums.shape) == (B * C, 2)
    f2, fi2 = modules(CASES[0], dev)
    cp2 = ops.spec_pack(truth(CASES[0])["c"].to(dev).reshape(6, 10, 9), 9, 0)
    x2, none = fi2.inverse_packed(cp2, torch.float32, True)
    assert none is None and torch.equal(x2, fi2.inverse_packed(cp2))


def test_row_sums_match_stored_rows(dev):
    """The sums returned with the bf16 rows against float64 sums of the rows as stored, 1e-12 relative: ``mk_irfft_sums`` adds the
    stored values and their (exact) squares in float64 from the first add."""
    from makani_amd import ops
    case = SPLIT_CASE
    nlat, nlon, lmax, mmax, B, C = case
    _, fi = modules(case, dev)
    cp = ops.spec_pack(truth(case)["c"].to(dev).reshape(B * C, lmax, mmax), mmax, 0)
    errs = {}
    for dt in (torch.bfloat16, torch.float32):
        x, sums = fi.inverse_packed(cp, dt, True)
        xd = x.double()
        want = torch.stack([xd.sum(dim=(1, 2)), (xd * xd).sum(dim=(1, 2))], dim=1)
        errs[dt] = ((sums - want).abs() / want.abs()).max().item()
        print(f"[fft2] row sums {dt}: {errs[dt]:.3e}")
    assert errs[torch.bfloat16] <= 1e-12 and errs[torch.float32] <= 1e-12


def test_two_runs_are_bit_equal(dev):
    case = CASES[3]
    t = truth(case)
    f, fi = modules(case, dev)
    x, c = t["x"].to(dev), t["c"].to(dev)
    with _count_launches() as n:
        assert torch.equal(f(x), f(x)) and torch.equal(fi(c), fi(c))
    assert n["lat_dft"] == 2 and n["lat_idft"] == 2


def test_graph_capture_replays_bit_equal(dev):
    """Forward + inverse captured with ``torch.cuda.graph`` and replayed on new input equal the eager result bit for bit."""
    case = CASES[1]
    f, fi = modules(case, dev)
    t = truth(case)
    static = t["x"].to(dev).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        fi(f(static))
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad(), _count_launches() as n:
        out = fi(f(static))
    assert n["lat_dft"] == 1 and n["lat_idft"] == 1
    new = torch.randn(static.shape, generator=torch.Generator().manual_seed(5)).to(dev)
    static.copy_(new)
    graph.replay()
    torch.cuda.synchronize()
    with torch.no_grad():
        eager = fi(f(new))
    assert torch.equal(out, eager)


def _conv_run(conv, x, gy, gr, dev):
    xd = x.to(dev).requires_grad_(True)
    conv.zero_grad()
    y, r = conv(xd)
    (y * gy.to(dev)).sum().add((r * gr.to(dev)).sum()).backward()
    return y.detach(), r.detach(), xd.grad.detach(), conv.weight.grad.detach().clone()


@pytest.mark.parametrize("op,shapes,modes", [
    ("dhconv", ((16, 32), (16, 32)), (10, 9)),
    ("dhconv", ((33, 64), (16, 32)), (10, 9)),      # scaled residual: synthesised from the private spectrum
    ("diagonal", ((16, 32), (16, 32)), (9, 9)),
])
def test_spectral_conv_matches_generic_path(dev, monkeypatch, op, shapes, modes):
    from makani_amd.layers import InverseRealFFT2, RealFFT2
    from makani_amd.spectral_convolution import SpectralConv
    torch.manual_seed(3)
    (ki, ni), (ko, no) = shapes
    L, M = modes
    conv = SpectralConv(RealFFT2(ki, ni, lmax=L, mmax=M), InverseRealFFT2(ko, no, lmax=L, mmax=M), 4, 6, operator_type=op).to(dev)
    x = torch.randn(2, 4, ki, ni)
    gy = torch.randn(2, 6, ko, no)
    gr = torch.randn(2, 4, ko, no) if conv.scale_residual else torch.randn(2, 4, ki, ni)
    with _count_launches() as n:
        hip = _conv_run(conv, x, gy, gr, dev)
    # forward: one analysis, one synthesis (two with a synthesised residual); backward: each one's adjoint launch
    nres = 1 if conv.scale_residual else 0
    assert n["lat_dft"] == 2 + nres and n["lat_idft"] == 2 + nres
    if op == "dhconv":      # the fused path on the private spectrum: no layout round trip through the modules' forward()
        assert conv._planar
    monkeypatch.setenv("MK_PLANAR_FFT", "torch")
    with _count_launches() as n:
        ref = _conv_run(conv, x, gy, gr, dev)
    assert n["lat_dft"] == 0 and n["lat_idft"] == 0
    errs = [rel(a, b) for a, b in zip(hip, ref)]
    print(f"[fft2] SpectralConv {op} {shapes}: y={errs[0]:.3e} residual={errs[1]:.3e} gx={errs[2]:.3e} gw={errs[3]:.3e}")
    assert max(errs) < TOL


def test_fno_net_step_matches_torch_path(dev, monkeypatch):
    from makani_amd.sfnonet import FourierNeuralOperatorNet
    torch.manual_seed(11)
    net = FourierNeuralOperatorNet(inp_shape=(32, 48), out_shape=(32, 48), inp_chans=3, out_chans=3, embed_dim=4, num_layers=2).to(dev)
    x = torch.randn(2, 3, 32, 48)
    tar = torch.randn(2, 3, 32, 48).to(dev)

    def step():
        net.zero_grad()
        xd = x.to(dev).requires_grad_(True)
        y = net(xd)
        ((y - tar) ** 2).mean().backward()
        return [y.detach(), xd.grad.detach()] + [p.grad.detach().clone() for p in net.parameters() if p.grad is not None]

    with _count_launches() as n:
        hip = step()
    assert n["lat_dft"] > 0 and n["lat_dft"] == n["lat_idft"]     # every transform of the step and its adjoint on the kernels
    monkeypatch.setenv("MK_PLANAR_FFT", "torch")
    with _count_launches() as n:
        ref = step()
    assert n["lat_dft"] == 0 and n["lat_idft"] == 0
    assert len(hip) == len(ref)
    errs = [rel(a, b) for a, b in zip(hip, ref)]
    print(f"[fft2] FNO step: out={errs[0]:.3e} gx={errs[1]:.3e} worst parameter gradient={max(errs[2:]):.3e}")
    assert max(errs) < TOL
