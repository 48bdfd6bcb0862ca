"""GPU tests of the channel layer norm (csrc/chnorm.hip, ops.channel_layer_norm, DistributedLayerNorm, the FNO block and the
net with normalization_layer="layer_norm"): parity against float64, degenerate inputs, spatial shards bit-equal to slices of
the full field, determinism, graph capture, and the module / block / network wiring.
  The parity tests print the errors they measure; DESIGN.md section 17 records them."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
EPS = 1e-6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from makani_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return (torch.linalg.norm(a - b) / max(torch.linalg.norm(b).item(), 1e-30)).item()


def _f64(t):
    t = t.detach().cpu()
    return t.to(torch.complex128) if t.is_complex() else t.double()


def y_tol(dtype):      # the bounds of tests/test_kernels_gpu.py::test_instance_norm
    return 2e-5 if dtype == F32 else 1e-2


def g_tol(dtype):
    return 1e-4 if dtype == F32 else 3e-2


@functools.lru_cache(maxsize=None)
def _case(shape, x_dtype, y_dtype, fuse, has_w, has_b):
    """Inputs (x in x_dtype, gy in y_dtype, fp32 parameters) and the float64 results on exactly those values; computed once
    per case and never modified."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(4)
    x = (torch.randn(B, C, H, W, generator=g) * 3 + 5).to(x_dtype)      # mean >> 0: a variance formula that cancels shows up
    w = torch.randn(C, generator=g) if has_w else None
    b = torch.randn(C, generator=g) if has_b else None
    gy = torch.randn(B, C, H, W, generator=g).to(y_dtype)
    xo = x.double().requires_grad_(True)
    wo = None if w is None else w.double().requires_grad_(True)
    bo = None if b is None else b.double().requires_grad_(True)
    yo = F.layer_norm(xo.permute(0, 2, 3, 1), (C,), wo, bo, EPS).permute(0, 3, 1, 2)
    if fuse:
        yo = F.gelu(yo)
    yo.backward(gy.double())
    return dict(x=x, w=w, b=b, gy=gy, y=yo.detach(), gx=xo.grad, gw=None if wo is None else wo.grad,
                gb=None if bo is None else bo.grad)


def _run(dev, case, fuse, y_dtype, eps=EPS):
    from makani_amd import ops
    xd = case["x"].to(dev).requires_grad_(True)
    wd = None if case["w"] is None else case["w"].to(dev).requires_grad_(True)
    bd = None if case["b"] is None else case["b"].to(dev).requires_grad_(True)
    y = ops.channel_layer_norm(xd, wd, bd, eps, fuse, y_dtype)
    y.backward(case["gy"].to(dev))
    return y.detach(), xd.grad, None if wd is None else wd.grad, None if bd is None else bd.grad


def _check(dev, shape, x_dtype, y_dtype, fuse, has_w=True, has_b=True):
    case = _case(shape, x_dtype, y_dtype, fuse, has_w, has_b)
    y, gx, gw, gb = _run(dev, case, fuse, y_dtype)
    assert y.dtype == y_dtype and gx.dtype == x_dtype and y.is_contiguous() and y.shape == case["x"].shape
    errs = dict(y=rel(y, case["y"]), gx=rel(gx, case["gx"]))
    if has_w:
        assert gw.dtype == F32
        errs["gw"] = rel(gw, case["gw"])
    if has_b:
        assert gb.dtype == F32
        errs["gb"] = rel(gb, case["gb"])
    print(f"chnorm parity {shape} x={x_dtype} y={y_dtype} fuse={fuse} w={has_w} b={has_b}: "
          + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert errs["y"] < y_tol(y_dtype), errs
    # the parameter gradients follow the sibling test: its bounds go by the dtype of the field
    for k in ("gx", "gw", "gb"):
        if k in errs:
            assert errs[k] < g_tol(x_dtype), errs


SHAPES = [
    (2, 5, 3, 5),          # P = 15: below a wave, odd
    (1, 73, 33, 63),       # odd P, C no multiple of anything, bf16 rows misaligned
    (2, 384, 7, 9),        # production channel count, tiny field
    (1, 1030, 5, 13),      # beyond the on-chip path of the backward
    (1, 8, 91, 180),       # many tiles with a tail
    (3, 16, 16, 24),       # fully aligned
    (1, 384, 8, 1440),     # production row width
    (1, 2500, 3, 8),       # beyond the on-chip path of the forward too, aligned stores
]


@pytest.mark.parametrize("fuse", [False, True])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_parity_vs_float64(dev, shape, dtype, fuse):
    _check(dev, shape, dtype, dtype, fuse)


@pytest.mark.parametrize("fuse", [False, True])
@pytest.mark.parametrize("x_dtype,y_dtype,has_w,has_b", [
    (F32, F32, True, False), (BF16, BF16, True, False),        # weight only (bias=False)
    (F32, F32, False, False), (BF16, BF16, False, False),      # elementwise_affine=False
    (F32, BF16, True, True), (BF16, F32, True, True),          # out_dtype different from the input's
], ids=["w-fp32", "w-bf16", "plain-fp32", "plain-bf16", "fp32-to-bf16", "bf16-to-fp32"])
@pytest.mark.parametrize("shape", [(1, 73, 33, 63), (3, 16, 16, 24)], ids=["odd", "aligned"])
def test_parity_variants(dev, shape, x_dtype, y_dtype, has_w, has_b, fuse):
    _check(dev, shape, x_dtype, y_dtype, fuse, has_w, has_b)


@pytest.mark.parametrize("fuse", [False, True])
def test_parity_bf16_field_fp32_result_production_width(dev, fuse):
    """A bf16 field whose norm returns fp32 (the module's default under autocast) at C = 384: the backward stages x and an fp32
    gy tile, 32 pixels wide so that both fit on chip."""
    _check(dev, (1, 384, 8, 1440), BF16, F32, fuse)


@pytest.mark.parametrize("fuse", [False, True])
def test_single_channel(dev, fuse):
    """C = 1: x - mean is exactly zero, so y is the bias (its GELU when fused) and gx, gw vanish."""
    from makani_amd import ops
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(1, 1, 4, 6, generator=g) * 3 + 5).to(dev).requires_grad_(True)
    w = torch.tensor([1.7], device=dev, requires_grad=True)
    b = torch.tensor([-0.6], device=dev, requires_grad=True)
    gy = torch.randn(1, 1, 4, 6, generator=g).to(dev)
    y = ops.channel_layer_norm(x, w, b, EPS, fuse)
    y.backward(gy)
    want = F.gelu(b.detach().double()) if fuse else b.detach().double()
    assert torch.allclose(y.double(), want.view(1, 1, 1, 1).expand_as(y), rtol=1e-5, atol=1e-6)      # erff is good to a few ulp
    assert torch.allclose(x.grad, torch.zeros_like(x.grad), atol=1e-6)
    assert torch.allclose(w.grad, torch.zeros_like(w.grad), atol=1e-6)
    assert all(torch.isfinite(t).all() for t in (y, x.grad, w.grad, b.grad))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_constant_over_channels(dev, dtype):
    """x[b, :, p] = const: the variance vanishes, values stay finite and y is the bias.  The fp32 sum of 7 equal values c
    carries at most 6 roundings of partial sums <= 7 |c| and the division one more: |x - mean| <= 7 * 2^-24 |c|, which
    rstd <= 1 / sqrt(eps) and |w| amplify; the result is then rounded once to the output dtype."""
    from makani_amd import ops
    C, eps = 7, 1e-5
    g = torch.Generator().manual_seed(11)
    const = (torch.randn(2, 1, 5, 9, generator=g) * 3 + 5).to(dtype)
    x = const.expand(2, C, 5, 9).contiguous().to(dev).requires_grad_(True)
    w, b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    wd, bd = w.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    y = ops.channel_layer_norm(x, wd, bd, eps)
    y.backward(torch.randn(2, C, 5, 9, generator=g).to(dtype).to(dev))
    assert all(torch.isfinite(t).all() for t in (y, x.grad, wd.grad, bd.grad))
    bound = 7 * 2.0 ** -24 * const.abs().max().item() / eps ** 0.5 * w.abs().max().item()
    bound += (2.0 ** -8 if dtype == BF16 else 2.0 ** -23) * (b.abs().max().item() + bound)
    assert (y.float().cpu() - b.view(1, C, 1, 1)).abs().max().item() <= bound


@pytest.mark.parametrize("fuse", [False, True])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 73, 33, 63), (2, 73, 31, 64)], ids=["odd", "aligned-full"])
def test_shards_bit_equal_to_slices(dev, shape, dtype, fuse):
    """The arithmetic of a pixel does not depend on its place: y and gx of a latitude and of a longitude shard are the bits
    of the same slice of the full result, whichever path (vector / single-element) each of them took."""
    from makani_amd import ops
    B, C, H, W = shape
    g = torch.Generator().manual_seed(12)
    x = (torch.randn(B, C, H, W, generator=g) * 3 + 5).to(dtype).to(dev)
    w, b = torch.randn(C, generator=g).to(dev), torch.randn(C, generator=g).to(dev)
    gy = torch.randn(B, C, H, W, generator=g).to(dtype).to(dev)

    def run(sl):
        xs = x[sl].contiguous().requires_grad_(True)
        ws, bs = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        y = ops.channel_layer_norm(xs, ws, bs, EPS, fuse)
        y.backward(gy[sl].contiguous())
        return y.detach(), xs.grad, ws.grad, bs.grad

    full = (slice(None),) * 4
    y, gx, gw, gb = run(full)
    for sl in ((slice(None), slice(None), slice(5, 19), slice(None)), (slice(None), slice(None), slice(None), slice(7, 40))):
        ys, gxs, _, _ = run(sl)
        assert torch.equal(ys, y[sl]) and torch.equal(gxs, gx[sl])
    # the two latitude shards' parameter gradients add up to the full ones
    top = run((slice(None), slice(None), slice(0, 14), slice(None)))
    bot = run((slice(None), slice(None), slice(14, None), slice(None)))
    assert rel(top[2] + bot[2], gw) < 1e-5 and rel(top[3] + bot[3], gb) < 1e-5


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_deterministic(dev, dtype):
    case = _case((1, 8, 91, 180), dtype, dtype, True, True, True)
    a = _run(dev, case, True, dtype)
    b = _run(dev, case, True, dtype)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_graph_capture(dev, dtype):
    """Forward + backward recorded on one stream after a warm-up, replayed on new contents: the eager bits."""
    from makani_amd import ops
    shape = (2, 73, 33, 63)
    g = torch.Generator().manual_seed(13)
    xs = (torch.randn(shape, generator=g) * 3 + 5).to(dtype).to(dev).requires_grad_(True)
    gys = torch.randn(shape, generator=g).to(dtype).to(dev)
    w = torch.randn(shape[1], generator=g).to(dev).requires_grad_(True)
    b = torch.randn(shape[1], generator=g).to(dev).requires_grad_(True)

    def step():
        y = ops.channel_layer_norm(xs, w, b, EPS, True)
        return (y,) + torch.autograd.grad(y, (xs, w, b), gys)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    x2 = (torch.randn(shape, generator=g) * 2 - 3).to(dtype).to(dev)
    gy2 = torch.randn(shape, generator=g).to(dtype).to(dev)
    with torch.no_grad():
        xs.copy_(x2)
        gys.copy_(gy2)
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in out]
    want = step()
    assert all(torch.equal(p, q) for p, q in zip(got, want))


def _count_calls(monkeypatch):
    from makani_amd import ops
    calls = []
    real = ops.channel_layer_norm

    def spy(x, weight, bias, eps=1e-5, fuse_gelu=False, out_dtype=None):
        calls.append(dict(fuse_gelu=bool(fuse_gelu), out_dtype=out_dtype, eps=eps))
        return real(x, weight, bias, eps, fuse_gelu, out_dtype)

    monkeypatch.setattr(ops, "channel_layer_norm", spy)
    return calls


def test_module_runs_on_hip_and_agrees_with_torch(dev, monkeypatch):
    from makani_amd.layer_norm import DistributedLayerNorm
    calls = _count_calls(monkeypatch)
    torch.manual_seed(3)
    m = DistributedLayerNorm(24, eps=1e-6).to(dev)
    with torch.no_grad():
        m.norm.weight.normal_()
        m.norm.bias.normal_()
    x = (torch.randn(2, 24, 9, 13) * 3 + 5).to(dev)
    gy = torch.randn(2, 24, 9, 13).to(dev)
    res = []
    for fn in (lambda t: m(t, fuse_gelu=True), lambda t: F.gelu(m._forward_torch(t))):
        m.zero_grad(set_to_none=True)
        xr = x.clone().requires_grad_(True)
        y = fn(xr)
        y.backward(gy)
        res.append((y.detach(), xr.grad, m.norm.weight.grad.clone(), m.norm.bias.grad.clone()))
    assert len(calls) == 1 and calls[0]["fuse_gelu"] and calls[0]["eps"] == 1e-6
    assert rel(res[0][0], res[1][0]) < 2e-5
    assert all(rel(p, q) < 1e-4 for p, q in zip(res[0][1:], res[1][1:]))
    # the default result dtype is what the torch formulation returns in the same context
    for xin in (x, x.to(BF16)):
        with torch.autocast("cuda", dtype=BF16):
            assert m(xin).dtype == m._forward_torch(xin).dtype
    assert m(x).dtype == m._forward_torch(x).dtype == F32
    assert m(x, out_dtype=BF16).dtype == BF16


@pytest.mark.parametrize("inner_skip", ["none", "linear"])
def test_block_calls(dev, monkeypatch, inner_skip):
    """norm0 (+ GELU, when nothing sits between them) and norm1 of a block are one call each."""
    from functools import partial
    from makani_amd.layer_norm import DistributedLayerNorm
    from makani_amd.sfnonet import FourierNeuralOperatorBlock
    from makani_amd.sht import InverseRealSHT, RealSHT
    calls = _count_calls(monkeypatch)
    torch.manual_seed(4)
    norm = partial(DistributedLayerNorm, normalized_shape=(8), elementwise_affine=True, eps=1e-6)
    blk = FourierNeuralOperatorBlock(RealSHT(33, 64, 16, 17, "equiangular"), InverseRealSHT(33, 64, 16, 17, "equiangular"), 8,
                                     operator_type="dhconv", act_layer=nn.GELU, norm_layer=(norm, norm), inner_skip=inner_skip,
                                     outer_skip="linear", use_mlp=True).to(dev)
    x = torch.randn(2, 8, 33, 64, device=dev)
    y = blk(x)
    assert y.shape == (2, 8, 33, 64) and torch.isfinite(y).all()
    assert [c["fuse_gelu"] for c in calls] == [inner_skip == "none", False]
    assert all(c["out_dtype"] in (None, F32) for c in calls)
    calls.clear()
    with torch.autocast("cuda", dtype=BF16):
        yb = blk(x)
    assert [c["out_dtype"] for c in calls] == [BF16, BF16]
    # the engine step against the fp32 step of the same block, at the bf16 bound of the net tests (with an inner skip norm0's
    # result is rounded to bf16 before the skip add and the activation)
    err = rel(yb.float(), y)
    print(f"chnorm block inner_skip={inner_skip}: bf16 engine step vs fp32 step {err:.2e}")
    assert err < 3e-2


def test_net_bf16_autocast_vs_oracle(dev, monkeypatch):
    """normalization_layer="layer_norm" on a bf16 autocast step: forward and every parameter gradient against the fp32 oracle
    with the bounds and the error measure of test_sfno_bf16_engine_gradients, and eval / no_grad == training forward."""
    from makani_amd.sfnonet import SphericalFourierNeuralOperatorNet
    from oracle import spectral as osp
    calls = _count_calls(monkeypatch)
    torch.manual_seed(9)
    kw = dict(inp_shape=(32, 64), out_shape=(32, 64), scale_factor=2, inp_chans=6, out_chans=5, embed_dim=32, num_layers=3,
              normalization_layer="layer_norm")
    ref = osp.SphericalFourierNeuralOperatorNet(**kw)
    net = SphericalFourierNeuralOperatorNet(**kw).to(dev)
    net.load_state_dict(ref.state_dict(), strict=True)
    x, tar = torch.randn(2, 6, 32, 64), torch.randn(2, 5, 32, 64)
    with torch.autocast("cuda", dtype=BF16):
        y = net(x.to(dev))
    assert len(calls) == 6 and all(c["out_dtype"] == BF16 for c in calls)
    ((y.float() - tar.to(dev)) ** 2).mean().backward()
    yo = ref(x)
    ((yo - tar) ** 2).mean().backward()
    fwd = rel(y.float(), yo)
    po = dict(ref.named_parameters())
    scale = float(np.median([torch.linalg.norm(_f64(p.grad)).item() for p in po.values()]))
    assert all(p.grad is not None for p in net.parameters())
    errs = {n: (torch.linalg.norm(_f64(p.grad) - _f64(po[n].grad))
                / max(torch.linalg.norm(_f64(po[n].grad)).item(), scale)).item() for n, p in net.named_parameters()}
    worst = max(errs, key=errs.get)
    print(f"chnorm net bf16: forward {fwd:.2e}, worst gradient {worst} {errs[worst]:.2e}")
    assert fwd < 3e-2
    assert errs[worst] < 5e-2, (worst, errs[worst])
    net.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=BF16):
        ye = net(x.to(dev))
    assert torch.equal(ye, y)
