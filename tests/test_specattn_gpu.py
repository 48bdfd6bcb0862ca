"""The non-linear spectral filter on the ``mk_spec_cmlp_*`` kernels: each kernel alone through the raw wrappers against
float64 einsums masked to l >= m, ``SpectralAttention`` on its fused path against the float64 chain that
``tests/test_parity_gpu.py::test_spectral_attention_filter`` spells out (SHT and planar pair), fused against fallback, the row
statistics for norm0, a captured net step, and two latitude shards on one card.

Criterion: relative L2 error <= 1e-5 (the project's fp32 criterion, ``tests/test_kernels_gpu.py``); the module's gradients
<= 5e-5 (the bounds of the existing attention test)."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import kernel_checks as kc
from kernel_checks import bf16_ulp as _bf16_ulp
from test_kernels_gpu import DH_CASES, rel, tril_mask

pytestmark = pytest.mark.gpu

TOL = 1e-5
SENTINEL = np.complex64(-77.0 + 55.0j)

# DH_CASES: the l shard and the m shard with empty degrees, > 1 column tile with a ragged edge (O = 130), > 128 rows,
# > 128 input channels -- and a dense spectrum (l_off >= mmax: every entry is data)
CASES = DH_CASES + [(12, 9, 2, 8, 16, 9, 0)]


def _f64(t):
    t = t.detach().cpu()
    return t.to(torch.complex128) if t.is_complex() else t.double()


def trel(a, b):
    a, b = _f64(a), _f64(b)
    return (torch.linalg.norm(a - b) / torch.linalg.norm(b)).item()


def _act_np(h, act):
    if act == 1:
        return np.maximum(h.real, 0) + 1j * h.imag
    if act == 2:
        return np.maximum(h.real, 0) + 1j * np.maximum(h.imag, 0)
    return h


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernels alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_degree", [False, True], ids=["shared", "per_degree"])
@pytest.mark.parametrize("L,M,B,I,O,l_off,m_off", CASES)
def test_kernels_alone(dev, L, M, B, I, O, l_off, m_off, per_degree):
    """Forward (act 0 / 1 / 2, bias and none), masked data gradient (the mask operand given explicitly: the reference uses the
    same one), weight gradient and bias gradient, for one weight panel and one per degree.  Every output's entries with l < m
    keep the sentinel written before the launch; the two reductions give equal bits on two runs.
    The kernels take even channel counts only (the bf16x3 engine); the first of ``DH_CASES`` has O = 5, and for it the contract
    is the launcher's refusal."""
    from makani_amd import ops
    rng = np.random.default_rng(31)

    def crand(*s):
        return (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(np.complex64)

    x, gy, a = crand(L, M, B, I), crand(L, M, B, O), crand(L, M, B, I)
    w = crand(L, I, O) if per_degree else crand(I, O)
    bias = crand(O)
    mask = tril_mask(L, M, l_off, m_off)[:, :, None, None]
    xd, gyd, ad = (torch.from_numpy(t.reshape(L, M, -1)).to(dev) for t in (x, gy, a))
    wd, bd = torch.from_numpy(w).to(dev), torch.from_numpy(bias).to(dev)
    if I % 2 or O % 2:
        with pytest.raises(RuntimeError, match="even channel counts"):
            ops.spec_cmlp_fwd_raw(xd, wd, None, B, 0, l_off, m_off)
        with pytest.raises(RuntimeError, match="even channel counts"):
            ops.spec_cmlp_dgrad_raw(gyd, wd, None, B, 0, l_off, m_off)
        with pytest.raises(RuntimeError, match="even channel counts"):
            ops.spec_cmlp_wgrad_raw(xd, gyd, B, per_degree, l_off, m_off)
        return
    x64, gy64, w64 = x.astype(np.complex128), np.where(mask, gy, 0).astype(np.complex128), w.astype(np.complex128)
    eq = "lmbi,lio->lmbo" if per_degree else "lmbi,io->lmbo"
    pre = np.einsum(eq, x64, w64)

    def sentinel_kept(out):
        return bool(np.all(out[~np.broadcast_to(mask, out.shape)] == SENTINEL))

    for act in (0, 1, 2):
        for b in (None, bd):
            out = torch.full((L, M, B * O), complex(SENTINEL), dtype=torch.complex64, device=dev)
            y = ops.spec_cmlp_fwd_raw(xd, wd, b, B, act, l_off, m_off, out=out)
            assert y is out
            y = y.cpu().numpy().reshape(L, M, B, O)
            want = _act_np(pre + (0 if b is None else bias.astype(np.complex128)), act)
            e = rel(np.where(mask, y, 0), np.where(mask, want, 0))
            print(f"[specattn] fwd {(L, M, B, I, O, l_off, m_off)} per_degree={per_degree} act={act} bias={b is not None}: {e:.2e}")
            assert e < TOL and sentinel_kept(y)
    # data gradient: gx = (gy conj(w)^T) * relu'(a), the imaginary parts always pass in mode 1
    eqd = "lmbo,lio->lmbi" if per_degree else "lmbo,io->lmbi"
    gfull = np.einsum(eqd, gy64, np.conj(w64))
    for act in (0, 1, 2):
        out = torch.full((L, M, B * I), complex(SENTINEL), dtype=torch.complex64, device=dev)
        gx = ops.spec_cmlp_dgrad_raw(gyd, wd, ad if act else None, B, act, l_off, m_off, out=out).cpu().numpy().reshape(L, M, B, I)
        mr = (a.real > 0) if act else True
        mi = (a.imag > 0) if act == 2 else True
        want = np.where(mr, gfull.real, 0) + 1j * np.where(mi, gfull.imag, 0)
        e = rel(np.where(mask, gx, 0), want)
        print(f"[specattn] dgrad {(L, M, B, I, O, l_off, m_off)} per_degree={per_degree} act={act}: {e:.2e}")
        assert e < TOL and sentinel_kept(gx)
    # weight gradient
    gw = ops.spec_cmlp_wgrad_raw(xd, gyd, B, per_degree, l_off, m_off)
    want = np.einsum("lmbi,lmbo->lio" if per_degree else "lmbi,lmbo->io", np.conj(np.where(mask, x64, 0)), gy64)
    assert tuple(gw.shape) == want.shape
    e = rel(gw.cpu().numpy(), want)
    print(f"[specattn] wgrad {(L, M, B, I, O, l_off, m_off)} per_degree={per_degree}: {e:.2e}")
    assert e < TOL
    assert torch.equal(gw, ops.spec_cmlp_wgrad_raw(xd, gyd, B, per_degree, l_off, m_off))
    # bias gradient: float64 sums in a fixed order
    gb = ops.spec_cmlp_bgrad_raw(gyd, B, l_off, m_off)
    e = rel(gb.cpu().numpy(), gy64.sum(axis=(0, 1, 2)))
    print(f"[specattn] bgrad {(L, M, B, I, O, l_off, m_off)}: {e:.2e}")
    assert e < TOL
    assert torch.equal(gb, ops.spec_cmlp_bgrad_raw(gyd, B, l_off, m_off))


def test_shared_weight_gradient_over_several_degree_groups(dev):
    """Enough degrees and tiles that a workgroup of the shared weight gradient contracts several degrees (of different row
    counts) and the fixed-order pass adds many partial panels: L = 200 with 136 x 130 channels is 2 x 3 tiles,
    ceil(1200 / 768) = 2 degrees per group, 100 partial panels; the workspace query must say so.  Held to the whole-tensor
    norm and, element by element, to ``kernel_checks.x3_elementwise`` (tests/test_x3_guard_gpu.py runs the same shape through
    the C ABI between guard bands)."""
    from makani_amd import _lib, ops
    L, M, B, I, O = 200, 20, 1, 136, 130
    assert _lib.load().mk_spec_cmlp_wgrad_workspace(L, I, O, 0) == 100 * I * O * 8
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((L, M, B, I)) + 1j * rng.standard_normal((L, M, B, I))).astype(np.complex64)
    gy = (rng.standard_normal((L, M, B, O)) + 1j * rng.standard_normal((L, M, B, O))).astype(np.complex64)
    mask = tril_mask(L, M)[:, :, None, None]
    xd, gyd = torch.from_numpy(x.reshape(L, M, -1)).to(dev), torch.from_numpy(gy.reshape(L, M, -1)).to(dev)
    gw = ops.spec_cmlp_wgrad_raw(xd, gyd, B, False)
    want = np.einsum("lmbi,lmbo->io", np.conj(np.where(mask, x, 0).astype(np.complex128)), np.where(mask, gy, 0).astype(np.complex128))
    assert rel(gw.cpu().numpy(), want) < TOL
    assert torch.equal(gw, ops.spec_cmlp_wgrad_raw(xd, gyd, B, False))
    # every element, under the engine's fp32-result criterion; the fixed-order sum of the 100 panels is the slack
    xm, gm = torch.from_numpy(np.where(mask, x, 0)), torch.from_numpy(np.where(mask, gy, 0))
    mag = kc.absdot("lmbi,lmbo->io", xm, gm)
    worst = kc.x3_elementwise(gw.cpu(), torch.from_numpy(want), mag, slack64=kc.x3_slack_sum(100, mag), what="shared wgrad, 100 panels")
    print(f"[specattn] shared wgrad over 100 panels: worst |err| / (2^-23 mag) {worst:.2f} of {kc.X3_C}")


# ---------------------------------------------------------------------------------------------------------------------
# 2. / 4. the module against the float64 chain
# ---------------------------------------------------------------------------------------------------------------------
VARIANTS = [("diagonal", "real", False), ("l-dependant", "cartesian", True), ("diagonal", "cartesian", True)]
# seeds picked on the CPU so that no masked pre-activation component of the float64 chain lies within 1e-5 rms of zero
# (_chain asserts it): a ReLU mask is discontinuous, and an entry at the edge would compare two different functions
# (margins of the chosen seeds: 3.5e-4, 1.9e-4, 6.1e-5 and, planar, 2.1e-4 rms; of seeds 0..7, 7 / 8 / 7 / 7 pass 1e-5)
SEEDS = {("sht",) + VARIANTS[0]: 3, ("sht",) + VARIANTS[1]: 4, ("sht",) + VARIANTS[2]: 5, ("fft",) + VARIANTS[1]: 5}
SHT_SHAPE = dict(nlat=33, nlon=64, lmax=20, mmax=21)
FFT_SHAPE = dict(nlat=32, nlon=64, lmax=16, mmax=17)


def _reference_transforms(kind, nlat, nlon, lmax, mmax):
    """float64 CPU transforms: the oracle's SHT, or the planar pair's torch formulation (both take float64 as it comes)."""
    if kind == "sht":
        from oracle import spectral as osp
        kw = dict(lmax=lmax, mmax=mmax, grid="equiangular")
        return osp.TorchRealSHT(nlat, nlon, **kw), osp.TorchInverseRealSHT(nlat, nlon, **kw)
    from makani_amd.layers import InverseRealFFT2, RealFFT2
    return RealFFT2(nlat, nlon, lmax=lmax, mmax=mmax)._forward_torch, InverseRealFFT2(nlat, nlon, lmax=lmax, mmax=mmax)._forward_torch


def _build(kind, variant, seed, nlat, nlon, lmax, mmax, C=6, B=2):
    from makani_amd.spectral_convolution import SpectralAttention
    operator_type, activation, bias = variant
    torch.manual_seed(seed)
    if kind == "sht":
        from makani_amd.sht import InverseRealSHT, RealSHT
        kw = dict(lmax=lmax, mmax=mmax, grid="equiangular")
        ft, it = RealSHT(nlat, nlon, **kw), InverseRealSHT(nlat, nlon, **kw)
    else:
        from makani_amd.layers import InverseRealFFT2, RealFFT2
        ft, it = RealFFT2(nlat, nlon, lmax=lmax, mmax=mmax), InverseRealFFT2(nlat, nlon, lmax=lmax, mmax=mmax)
    mod = SpectralAttention(ft, it, C, C, operator_type=operator_type, hidden_size_factor=2, complex_activation=activation,
                            bias=bias, spectral_layers=2)
    x, g = torch.randn(B, C, nlat, nlon), torch.randn(B, C, nlat, nlon)
    return mod, x, g


def _chain(kind, mod, x, g, variant, nlat, nlon, lmax, mmax):
    """The float64 chain of ``test_spectral_attention_filter``; returns (y, input gradient, parameter gradients by name, the
    smallest distance of a masked pre-activation component from zero in units of their rms)."""
    operator_type, activation, bias = variant
    fwd, inv = _reference_transforms(kind, nlat, nlon, lmax, mmax)
    params = {n: _f64(p).requires_grad_(True) for n, p in mod.named_parameters()}
    xo = x.double().requires_grad_(True)
    c = fwd(xo)
    eq = "bixy,io->boxy" if operator_type == "diagonal" else "bixy,xio->boxy"
    valid = torch.from_numpy(tril_mask(lmax, mmax)) if kind == "sht" else torch.ones(lmax, mmax, dtype=torch.bool)
    margin = float("inf")
    for layer in range(2):
        c = torch.einsum(eq, c, params[f"w.{layer}"])
        if bias:
            c = c + params[f"b.{layer}"]
        comps = [c.real] if activation == "real" else [c.real, c.imag]
        vals = torch.stack([t.detach()[..., valid] for t in comps])
        margin = min(margin, (vals.abs().min() / vals.square().mean().sqrt()).item())
        c = torch.complex(torch.relu(c.real), c.imag if activation == "real" else torch.relu(c.imag))
    yo = inv(torch.einsum(eq, c, params["wout"]))
    yo.backward(g.double())
    return yo.detach(), xo.grad, {n: p.grad for n, p in params.items()}, margin


def _count_calls(monkeypatch, name):
    from makani_amd import ops
    calls, real = [], getattr(ops, name)
    monkeypatch.setattr(ops, name, lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def _module_against_chain(dev, monkeypatch, kind, variant, shape):
    monkeypatch.setenv("MK_SPEC_ATTN", "hip")
    mod, x, g = _build(kind, variant, SEEDS[(kind,) + variant], **shape)
    yo, gxo, gpo, margin = _chain(kind, mod, x, g, variant, **shape)
    print(f"[specattn] {kind} {variant}: smallest masked pre-activation component {margin:.2e} rms")
    assert margin > 1e-5, "pick another seed: a pre-activation of the float64 reference sits on the edge of the ReLU mask"
    mod = mod.to(dev)
    fwd_calls, chain_calls = _count_calls(monkeypatch, "spec_cmlp_fwd_raw"), _count_calls(monkeypatch, "spec_channel_mlp")
    xd = x.to(dev).requires_grad_(True)
    y, res = mod(xd)
    assert len(chain_calls) == 1 and len(fwd_calls) == 3, "not a run of the fused path"
    assert res is xd and y.shape == x.shape
    y.backward(g.to(dev))
    errs = {"y": trel(y, yo), "x.grad": trel(xd.grad, gxo)}
    for n, p in mod.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and p.grad.stride() == p.stride(), n
        errs[n] = trel(p.grad, gpo[n])
    print(f"[specattn] {kind} {variant}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs.pop("y") < 1e-5
    worst = max(errs, key=errs.get)
    assert errs[worst] < 5e-5, (worst, errs[worst])


@pytest.mark.parametrize("variant", VARIANTS, ids=["-".join(map(str, v)) for v in VARIANTS])
def test_module_against_float64_chain(dev, monkeypatch, variant):
    _module_against_chain(dev, monkeypatch, "sht", variant, SHT_SHAPE)


def test_planar_pair_against_float64_chain(dev, monkeypatch):
    """``RealFFT2`` / ``InverseRealFFT2`` on their HIP path: the dense spectrum (every (l, m) entry is data)."""
    monkeypatch.setenv("MK_PLANAR_FFT", "hip")
    _module_against_chain(dev, monkeypatch, "fft", VARIANTS[1], FFT_SHAPE)


# ---------------------------------------------------------------------------------------------------------------------
# 3. fused against fallback, and the row statistics
# ---------------------------------------------------------------------------------------------------------------------
def test_fused_equals_fallback_fp32(dev, monkeypatch):
    """The same module and input with ``MK_SPEC_ATTN=hip`` and ``torch``: output and input gradient (the seeded case of the
    chain test above, whose pre-activations keep their distance from the edge of the mask)."""
    variant = VARIANTS[1]
    mod, x, g = _build("sht", variant, SEEDS[("sht",) + variant], **SHT_SHAPE)
    mod = mod.to(dev)
    calls = _count_calls(monkeypatch, "spec_channel_mlp")
    res = {}
    for knob in ("hip", "torch"):
        monkeypatch.setenv("MK_SPEC_ATTN", knob)
        del calls[:]
        xd = x.to(dev).requires_grad_(True)
        y, r = mod(xd)
        assert len(calls) == (1 if knob == "hip" else 0) and r is xd
        y.backward(g.to(dev))
        res[knob] = (y.detach(), xd.grad)
    e = (trel(res["hip"][0], res["torch"][0]), trel(res["hip"][1], res["torch"][1]))
    print(f"[specattn] fused vs fallback fp32: y {e[0]:.2e}, x.grad {e[1]:.2e}")
    assert max(e) < 1e-5




def test_fused_equals_fallback_bf16_autocast_and_row_sums(dev, monkeypatch):
    """A bf16 field under bf16 autocast on a grid whose inverse FFT writes bf16 rows itself (nlon = 480), different grids in
    and out so that the residual is a synthesis too.  Both paths compute in fp32 and round the result to bf16 once, so an entry
    differs by at most one bf16 ulp of the output: the ulp at the larger of the two values, for entries below rms / 256 the ulp
    at rms / 256 (1.5e-5 rms, the fp32 criterion: two fp32 evaluations of an entry near zero differ by that much before either
    is rounded).
    ``want_row_sums`` through ``SpectralFilterLayer``: the sums the inverse FFT hands norm0 against float64 sums of the rows it
    returned, 1e-12 relative (the bound of ``tests/test_fft2_gpu.py::test_row_sums_match_stored_rows``)."""
    from makani_amd.sfnonet import SpectralFilterLayer
    from makani_amd.sht import InverseRealSHT, RealSHT
    torch.manual_seed(4)
    B, C = 2, 6
    ft = RealSHT(33, 64, lmax=20, mmax=21, grid="equiangular")
    it = InverseRealSHT(30, 480, lmax=20, mmax=21, grid="legendre-gauss")
    layer = SpectralFilterLayer(ft, it, C, filter_type="non-linear", operator_type="l-dependant", hidden_size_factor=2,
                                complex_activation="cartesian", spectral_layers=2, bias=True).to(dev)
    x = torch.randn(B, C, 33, 64, device=dev).to(torch.bfloat16)
    calls = _count_calls(monkeypatch, "spec_channel_mlp")
    res = {}
    for knob in ("hip", "torch"):
        monkeypatch.setenv("MK_SPEC_ATTN", knob)
        del calls[:]
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            y, r, sums = layer(x, want_row_sums=True)
        assert len(calls) == (1 if knob == "hip" else 0)
        assert y.dtype == torch.bfloat16 and r.dtype == torch.bfloat16 and tuple(y.shape) == (B, C, 30, 480) == tuple(r.shape)
        res[knob] = (y.double(), r.double(), sums)
    assert res["torch"][2] is None
    for k, name in ((0, "y"), (1, "residual")):
        a, b = res["hip"][k], res["torch"][k]
        rms = b.square().mean().sqrt()
        tol = _bf16_ulp(torch.maximum(torch.maximum(a.abs(), b.abs()), rms / 256))
        worst = ((a - b).abs() / tol).max().item()
        print(f"[specattn] fused vs fallback bf16 {name}: worst difference {worst:.2f} ulp, {(a != b).double().mean().item():.2%} differ")
        assert worst <= 1.0
    yd, sums = res["hip"][0].reshape(B * C, 30, 480), res["hip"][2]
    assert sums is not None and sums.dtype == torch.float64 and tuple(sums.shape) == (B * C, 2)
    want = torch.stack([yd.sum(dim=(1, 2)), (yd * yd).sum(dim=(1, 2))], dim=1)
    e = ((sums - want).abs() / want.abs()).max().item()
    print(f"[specattn] row sums: {e:.3e}")
    assert e <= 1e-12
    # fp32 rows, and the plain call without the statistics
    monkeypatch.setenv("MK_SPEC_ATTN", "hip")
    with torch.no_grad():
        y32, _, s32 = layer(x.float(), want_row_sums=True)
        y2, _ = layer(x.float())
    yd = y32.double().reshape(B * C, 30, 480)
    want = torch.stack([yd.sum(dim=(1, 2)), (yd * yd).sum(dim=(1, 2))], dim=1)
    assert ((s32 - want).abs() / want.abs()).max().item() <= 1e-12 and torch.equal(y2, y32)


def test_chain_without_activation(dev):
    """``ops.spec_channel_mlp`` with ``act=None`` is a chain of plain products: the backward passes no mask operand (the
    launcher refuses one without an activation mode).  Output and every gradient against float64 einsums on the triangle."""
    from makani_amd import ops
    L, M, B, I, H, O = 10, 11, 2, 4, 6, 4
    gen = torch.Generator().manual_seed(9)

    def crand(*s):
        return torch.complex(torch.randn(*s, generator=gen), torch.randn(*s, generator=gen))

    c, w0, b0, wout, g = crand(L, M, B, I), crand(I, H), crand(H), crand(H, O), crand(L, M, B, O)
    mask = torch.from_numpy(tril_mask(L, M))[:, :, None, None]
    leaves = [t.to(dev).requires_grad_(True) for t in (c.reshape(L, M, B * I), w0, b0, wout)]
    y = ops.spec_channel_mlp(leaves[0], [leaves[1]], [leaves[2]], leaves[3], B, None, False)
    y.backward(torch.where(mask, g, 0).reshape(L, M, B * O).to(dev))
    ref = [t.to(torch.complex128).requires_grad_(True) for t in (c, w0, b0, wout)]
    yo = torch.einsum("lmbh,ho->lmbo", torch.where(mask, torch.einsum("lmbi,ih->lmbh", ref[0], ref[1]) + ref[2], 0), ref[3])
    yo.backward(torch.where(mask, g, 0).to(torch.complex128))
    assert trel(torch.where(mask, y.detach().cpu().reshape(L, M, B, O), 0), yo.detach()) < TOL
    for name, a, b in zip(("c", "w", "b", "wout"), leaves, ref):
        got = a.grad.cpu().reshape(b.shape)
        got = torch.where(mask, got, 0) if name == "c" else got
        assert trel(got, b.grad) < TOL, name


def test_fallback_cases_do_not_touch_the_kernels(dev, monkeypatch):
    """``modulus``, odd channel counts and active dropout stay on the torch formulation with ``MK_SPEC_ATTN=hip``."""
    from makani_amd.sht import InverseRealSHT, RealSHT
    from makani_amd.spectral_convolution import SpectralAttention
    monkeypatch.setenv("MK_SPEC_ATTN", "hip")
    calls = _count_calls(monkeypatch, "spec_channel_mlp")
    kw = dict(lmax=8, mmax=9, grid="equiangular")
    x = torch.randn(1, 4, 9, 16, device=dev)
    for C, extra, train in ((4, dict(complex_activation="modulus"), False), (3, {}, False), (4, dict(drop_rate=0.5), True),
                            (4, dict(drop_rate=0.5), False), (4, {}, False)):
        mod = SpectralAttention(RealSHT(9, 16, **kw), InverseRealSHT(9, 16, **kw), C, C, **extra).to(dev).train(train)
        del calls[:]
        y, _ = mod(x[:, :C])
        assert torch.isfinite(y).all()
        fused = C == 4 and extra.get("complex_activation") != "modulus" and not (train and "drop_rate" in extra)
        assert len(calls) == int(fused), (C, extra, train)


# ---------------------------------------------------------------------------------------------------------------------
# 5. a net step, captured
# ---------------------------------------------------------------------------------------------------------------------
def test_net_step_captured_and_replayed(dev, monkeypatch):
    """A non-linear SFNO at the sizes of ``test_sfno_with_non_linear_filter_steps``: forward + loss + backward captured in a
    HIP graph (the sequence of ``test_graph_capture_replay_with_spec_mix``); two replays are bit-equal to each other and
    within 1e-5 of the eager step.
    Bit-equal: the loss (the whole forward) and every parameter gradient but the weights of the fp32 1x1 convolutions, whose
    gradient kernel adds its pixel slabs with fp32 atomics (``conv_x3_kernel`` MODE 2) and so gives other last
    bits from one eager run to the next too, whatever filter the blocks hold; those are held to the 1e-5 of the eager step.
    Everything the filter computes -- its own weight and bias gradients, and the data gradient every parameter in front of it
    receives (norms, biases, position embedding) -- is in the bit-equal set."""
    import gc
    from makani_amd.layers import Conv1x1
    from makani_amd.sfnonet import SphericalFourierNeuralOperatorNet
    monkeypatch.setenv("MK_SPEC_ATTN", "hip")
    torch.manual_seed(2)
    kw = dict(inp_shape=(33, 64), out_shape=(33, 64), scale_factor=2, inp_chans=3, out_chans=2, embed_dim=8, num_layers=2)
    net = SphericalFourierNeuralOperatorNet(filter_type="non-linear", operator_type="diagonal", **kw).to(dev)
    x, tar = torch.randn(2, 3, 33, 64, device=dev), torch.randn(2, 2, 33, 64, device=dev)
    static_inp, static_tar = x.clone(), tar.clone()
    calls = _count_calls(monkeypatch, "spec_channel_mlp")
    capture_stream = torch.cuda.Stream()
    capture_stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(capture_stream):
        for _ in range(3):
            net.zero_grad(set_to_none=True)
            static_loss = ((net(static_inp) - static_tar) ** 2).mean()
            static_loss.backward()
        capture_stream.synchronize()
        assert len(calls) == 3 * 2          # one chain per block and step
        ref_loss = static_loss.item()
        ref_grads = {n: p.grad.clone() for n, p in net.named_parameters()}
        gc.collect()
        torch.cuda.empty_cache()
        graph = torch.cuda.CUDAGraph()
        net.zero_grad(set_to_none=True)
        graph.capture_begin()
        static_loss = ((net(static_inp) - static_tar) ** 2).mean()
        static_loss.backward()
        graph.capture_end()
    torch.cuda.current_stream().wait_stream(capture_stream)
    replays = []
    for _ in range(2):
        static_inp.copy_(x)
        static_tar.copy_(tar)
        graph.replay()
        torch.cuda.synchronize()
        replays.append((static_loss.clone(), {n: p.grad.clone() for n, p in net.named_parameters()}))
    assert torch.equal(replays[0][0], replays[1][0])
    assert abs(replays[0][0].item() - ref_loss) <= 1e-5 * abs(ref_loss)
    atomic = {f"{mn}.weight" for mn, m in net.named_modules() if isinstance(m, Conv1x1)}
    names = [n for n, _ in net.named_parameters()]
    differ = [n for n in names if not torch.equal(replays[0][1][n], replays[1][1][n])]
    print(f"[specattn] replays: {len(names)} gradients, {len(atomic)} of them atomic sums; not bit-equal: {differ}")
    assert atomic < set(names) and any(".filter." in n for n in set(names) - atomic)
    for n, p in net.named_parameters():
        assert p.grad is not None, n
        assert n in atomic or torch.equal(replays[0][1][n], replays[1][1][n]), n
        assert torch.equal(p.grad, ref_grads[n]) or trel(p.grad, ref_grads[n]) < 1e-5, n


# ---------------------------------------------------------------------------------------------------------------------
# 6. two latitude shards on one card (the machinery of tests/test_fft2_dist_gpu.py: gloo wire, ranks take turns on the card)
# ---------------------------------------------------------------------------------------------------------------------
DIST_BOUND = 1e-6      # the reference's distributed bound (tests/distributed: forward output and input gradient)


def _field_err(a, b):
    """Mean per-field relative L2 error, the measure of the reference's distributed tests."""
    a, b = _f64(a), _f64(b)
    return torch.mean(torch.linalg.vector_norm(a - b, dim=(-2, -1)) / torch.linalg.vector_norm(b, dim=(-2, -1))).item()


def _body_h2(dev, operator_type):
    from test_distributed_gpu import _gather, _shard
    from makani_amd import comm, mappings, ops
    from makani_amd.distributed import DistributedInverseRealSHT, DistributedRealSHT
    from makani_amd.sht import InverseRealSHT, RealSHT
    from makani_amd.spectral_convolution import SpectralAttention
    hr = comm.get_rank("h")
    B, C = 2, 4
    fkw, ikw = dict(lmax=21, mmax=22, grid="equiangular"), dict(lmax=21, mmax=22, grid="legendre-gauss")
    akw = dict(operator_type=operator_type, hidden_size_factor=2, complex_activation="cartesian", bias=True, spectral_layers=2)
    torch.manual_seed(100 + hr)
    mod = SpectralAttention(DistributedRealSHT(33, 64, **fkw), DistributedInverseRealSHT(32, 64, **ikw), C, C, **akw)
    gen = torch.Generator().manual_seed(5)      # the shards differ from rank to rank, the replicated parameters must not
    with torch.no_grad():
        for p in mod.parameters():
            if getattr(p, "sharded_dims_mp", [None])[0] != "h":
                p.copy_(0.5 * torch.randn(p.shape, generator=gen, dtype=torch.complex64))
    mod = mod.to(dev)
    assert mod.modes_lat_local == (11, 10)[hr] and mod.l_off == (0, 11)[hr]
    ref = SpectralAttention(RealSHT(33, 64, **fkw), InverseRealSHT(32, 64, **ikw), C, C, **akw).to(dev)
    with torch.no_grad():
        for (n, p), q in zip(mod.named_parameters(), ref.parameters()):
            q.copy_(_gather(p.detach(), 0, "h") if getattr(p, "sharded_dims_mp", [None])[0] == "h" else p)
    torch.manual_seed(7)
    xg, gg, rg = torch.randn(B, C, 33, 64), torch.randn(B, C, 32, 64), torch.randn(B, C, 32, 64)
    calls, real = [], ops.spec_channel_mlp
    ops.spec_channel_mlp = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        xo = xg.to(dev).requires_grad_(True)
        yo, ro = ref(xo)
        ((yo * gg.to(dev)).sum() + (ro * rg.to(dev)).sum()).backward()
        xl = _shard(xg, 2, "h").to(dev).requires_grad_(True)
        yl, rl = mod(xl)
        ((yl * _shard(gg, 2, "h").to(dev)).sum() + (rl * _shard(rg, 2, "h").to(dev)).sum()).backward()
    finally:
        ops.spec_channel_mlp = real
    assert len(calls) == 2, "both modules run the fused path"
    mappings.reduce_shared_gradients(mod)
    e = {"y": _field_err(yl, _shard(yo.detach(), 2, "h")), "residual": _field_err(rl, _shard(ro.detach(), 2, "h")),
         "x.grad": _field_err(xl.grad, _shard(xo.grad, 2, "h"))}
    for (n, p), q in zip(mod.named_parameters(), ref.parameters()):
        want = q.grad
        if getattr(p, "sharded_dims_mp", [None])[0] == "h":
            want = torch.split(want, [11, 10], dim=0)[hr]
        e[n] = trel(p.grad, want)
    print(f"[specattn] h = 2 rank {hr} {operator_type}: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    worst = max(e, key=e.get)
    assert e[worst] <= DIST_BOUND, (worst, e[worst])


def _worker(rank, world, port, q, lock):
    held = False
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                          MK_SPEC_ATTN="hip")
        from test_distributed_gpu import _take_turns_on_the_card
        from makani_amd import comm
        comm.init(model_parallel_sizes=[world, 1, 1, 1], backend="gloo")
        dev = torch.device("cuda:0")
        _take_turns_on_the_card(lock)
        lock.acquire()
        held = True
        for operator_type in ("diagonal", "l-dependant"):
            _body_h2(dev, operator_type)
        torch.cuda.synchronize()
        dist.barrier()
        q.put((rank, "ok"))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, "".join(traceback.format_exception(type(e), e, e.__traceback__))))
    finally:
        if held:
            try:
                lock.release()
            except ValueError:
                pass
        if dist.is_initialized():
            dist.destroy_process_group()


def test_h2_two_ranks_on_one_gpu():
    """h = 2 over gloo, lmax = 21 (11 and 10 degrees): each rank's output, residual and input gradient equal the slices of the
    single-rank module built from the gathered weights; after ``reduce_shared_gradients`` the replicated parameters' gradients
    equal the single-rank ones and the per-degree weights' their slices."""
    from test_distributed_gpu import _free_port
    assert torch.cuda.device_count() >= 1
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    lock = ctx.Lock()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, lock)) for r in range(2)]
    for p in procs:
        p.start()
    results = [q.get(timeout=600) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    bad = [r for r in results if r[1] != "ok"]
    assert not bad, "\n".join(f"rank {r}: {m}" for r, m in bad)
