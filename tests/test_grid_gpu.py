"""GPU tests of ``grids.GridConverter`` / ``ops.lat_interp`` on the device: nlat = 33, W = 66, a ``[2, 2, 3, H, W]`` batch built from
the recorded input of tests/golden/ref_grids.npz.  Forward against the reference's recorded output within the forward bound of
tests/grid_checks.py, ``.grad`` against the float64 transpose within the backward bound, ``out=`` into a channel slice of a
larger bf16 buffer, graph capture, and ``MK_GRID=torch`` on the same tensors within twice the bound."""
import numpy as np
import pytest
import torch

import grid_checks as gc
from kernel_checks import SENTINEL, node_kinds

pytestmark = pytest.mark.gpu

NLAT, W = 33, 66


@pytest.fixture(scope="module")
def case():
    """(x [2, 2, 3, H, W] fp32 numpy, the reference's output for it, the table)."""
    f = gc.fixture()
    x, y = f["n33_x"], f["n33_y"]
    idx, wgt, hs = gc.converter_table(NLAT)
    x5 = np.stack([x, x[::-1].copy()])
    y5 = np.stack([y, y[::-1].copy()])
    return x5, y5, idx, wgt


@pytest.fixture()
def conv(dev, monkeypatch):
    from makani_amd.grids import GridConverter
    monkeypatch.setenv("MK_GRID", "hip")
    f = gc.fixture()
    lat = torch.from_numpy(f["n33_f32_lat"]).to(dev)
    lon = torch.deg2rad(torch.linspace(0.0, 360.0, W + 1)[:-1]).to(dev)
    c = GridConverter("equiangular", "legendre-gauss", lat, lon)
    assert c.dst_lat.device.type == "cuda" and c.indices.device.type == "cuda" and c.interp_weights.device.type == "cuda"
    assert torch.equal(c.indices.cpu(), torch.from_numpy(f["n33_f32_indices"]))
    assert torch.equal(c.interp_weights.cpu(), torch.from_numpy(f["n33_f32_interp_weights"]))
    return c


def test_forward_against_the_reference_output(dev, conv, case):
    x5, y5, idx, wgt = case
    got = conv(torch.from_numpy(x5).to(dev))
    torch.cuda.synchronize()
    assert got.shape == y5.shape and got.dtype == torch.float32
    ref, bound = gc.forward_reference(x5.reshape(-1, NLAT, W), idx, wgt, False)
    gc.assert_within(got.cpu().reshape(-1, NLAT, W), ref, bound, torch.float32, "against float64")
    # the reference's own fp32 result lies within the same bound of the float64 value: twice the bound between the two
    assert bool((np.abs(got.cpu().numpy().astype(np.float64) - y5.astype(np.float64)).reshape(-1, NLAT, W) <= 2 * bound).all())
    assert conv.tables(dev) is conv.tables(dev)


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "norm"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_gradient_against_the_float64_transpose(dev, conv, case, dtype, norm):
    x5, _, idx, wgt = case
    xv = torch.from_numpy(x5).to(dtype)
    x = xv.to(dev).requires_grad_(True)
    bias, scale = (torch.from_numpy(gc.BIAS).reshape(1, 3, 1, 1).to(dev), torch.from_numpy(gc.SCALE).reshape(1, 3, 1, 1).to(dev)) if norm else (None, None)
    y = conv(x, bias=bias, scale=scale)
    assert "_LatInterpBackward" in node_kinds(y) and y.dtype == dtype
    gy = gc.field(y.shape, 21, bf16=dtype == torch.bfloat16)
    y.backward(torch.from_numpy(gy).to(dev, dtype))
    torch.cuda.synchronize()
    assert x.grad.shape == x.shape and x.grad.dtype == dtype
    ref, bound, _ = gc.backward_reference(gy.reshape(-1, NLAT, W), idx, wgt, NLAT, norm)
    gc.assert_within(x.grad.cpu().reshape(-1, NLAT, W), ref, bound, dtype, f"grad {dtype} norm={norm}")
    fref, fbound = gc.forward_reference(xv.float().numpy().reshape(-1, NLAT, W), idx, wgt, norm)
    gc.assert_within(y.detach().cpu().reshape(-1, NLAT, W), fref, fbound, dtype, f"forward {dtype} norm={norm}")


def test_out_into_a_channel_slice_of_a_larger_bf16_buffer(dev, conv, case):
    x5, _, idx, wgt = case
    bias, scale = torch.from_numpy(gc.BIAS).to(dev), torch.from_numpy(gc.SCALE).to(dev)
    buf = torch.full((2, 2, 6, NLAT, W), SENTINEL, dtype=torch.bfloat16, device=dev)
    before = buf.clone()
    out = buf[:, :, 2:5]
    got = conv(torch.from_numpy(x5).to(dev), bias=bias, scale=scale, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and got.dtype == torch.bfloat16
    for rest in (slice(0, 2), slice(5, 6)):
        assert torch.equal(buf[:, :, rest].contiguous().view(torch.uint8), before[:, :, rest].contiguous().view(torch.uint8))
    ref, bound = gc.forward_reference(x5.reshape(-1, NLAT, W), idx, wgt, True)
    gc.assert_within(out.cpu().reshape(-1, NLAT, W), ref, bound, torch.bfloat16, "out slice")
    same = conv(torch.from_numpy(x5).to(dev), bias=bias, scale=scale, out_dtype=torch.bfloat16)
    assert torch.equal(same.view(torch.uint8), out.contiguous().view(torch.uint8))
    # under autograd the given buffer is the function's (dirty) output
    grads = []
    for given in (None, torch.empty(2, 2, 3, NLAT, W, device=dev)):
        x = torch.from_numpy(x5).to(dev).requires_grad_(True)
        y = conv(x, bias=bias, scale=scale, out=given)
        assert given is None or y.data_ptr() == given.data_ptr()
        (y * y).sum().backward()
        grads.append(x.grad)
    assert torch.equal(grads[0].view(torch.int32), grads[1].view(torch.int32))


def test_capture_and_replay_equal_the_eager_bits(dev, conv, case):
    x5 = case[0]
    x = torch.from_numpy(x5).to(dev)
    bias, scale = torch.from_numpy(gc.BIAS).to(dev), torch.from_numpy(gc.SCALE).to(dev)
    eager = conv(x, bias=bias, scale=scale)
    static_x = torch.zeros_like(x)
    out = torch.empty_like(eager)
    conv.tables(dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        conv(static_x, bias=bias, scale=scale, out=out)
    static_x.copy_(x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), eager.view(torch.int32))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_the_torch_switch_agrees_within_twice_the_bound(dev, conv, case, monkeypatch, dtype):
    x5, _, idx, wgt = case
    xv = torch.from_numpy(x5).to(dtype)
    bias, scale = torch.from_numpy(gc.BIAS).to(dev), torch.from_numpy(gc.SCALE).to(dev)
    hip = conv(xv.to(dev), bias=bias, scale=scale, out_dtype=torch.float32)
    monkeypatch.setenv("MK_GRID", "torch")
    x = xv.to(dev).requires_grad_(True)
    ref = conv(x, bias=bias, scale=scale, out_dtype=torch.float32)
    assert "_LatInterpBackward" not in node_kinds(ref)
    torch.cuda.synchronize()
    _, bound = gc.forward_reference(xv.float().numpy().reshape(-1, NLAT, W), idx, wgt, True)
    diff = (hip.double() - ref.detach().double()).abs().cpu().numpy().reshape(-1, NLAT, W)
    assert bool((diff <= 2 * bound).all()), float((diff / np.maximum(bound, 1e-300)).max())
