"""GPU tests of ``mk_ens_crps_bwd`` (csrc/ens.hip) through the C ABI -- guarded outputs, poisoned inputs, member strides with
gaps on both sides -- of ``ops.ensemble_crps_sums`` under autograd and graph capture, and of the ``crps`` losses of
``LossHandler`` behind a step wrapper.  The gradient is held per element to ``(u + 2^-40) |r|`` against the numpy closed form
of tests/ens_loss_checks.py (u = 2^-24 for an fp32 gradient, 2^-8 for bf16: one rounding of a float64 value whose own error
is a few 2^-53), to exact zeros where the reference is zero and to NaN exactly at all members of the NaN points.  The input
gaps hold NaN (a read there would make a point NaN), the output gaps and bands must keep the sentinel bit for bit."""
import numpy as np
import pytest
import torch

import capi_checks as capi
import ens_checks as ec
import ens_loss_checks as lc
from kernel_checks import SENTINEL, guarded, node_kinds, poisoned
from test_ens_gpu import _device_members
from test_ens_loss_cpu import REFUSED

pytestmark = pytest.mark.gpu

# (B, E, C, H, W): two slabs, the second of one row, rows odd and shorter than a tile; a row longer than a tile; P = 8 with
# pads; P = 16 without; members whose alignments disagree (C H W = 27)
SHAPES = [(2, 2, 2, 9, 37), (1, 3, 1, 3, 300), (2, 5, 2, 8, 8), (1, 16, 1, 9, 37), (4, 4, 1, 3, 9)]
DTYPES = ["float32", "bfloat16"]
ids = lambda s: "x".join(map(str, s))


def launch(dev, ens, tar, wrow, gs, dtype="float32", gap=0):
    """One call of mk_ens_crps_bwd on numpy inputs: the members between NaN bands with ``gap`` NaN elements behind every
    member's block, the gradient into a guarded buffer with the same gaps.  Returns the gradient ``[B, E, C, H, W]`` as a torch
    tensor of the gradient's dtype on the host, after checking the bands and the gaps."""
    from makani_amd import _lib
    lib = _lib.load()
    B, E, C, H, W = ens.shape
    chw = C * H * W
    keep, eptr, bstride, estride = _device_members(ens, dtype, dev, False, gap)
    td = poisoned(torch.from_numpy(np.array(tar)), dev)
    wd = poisoned(torch.from_numpy(np.array(wrow)), dev)
    gd = poisoned(torch.from_numpy(np.array(gs)), dev)
    out, check = guarded((B, E, chw + gap), getattr(torch, dtype), dev)
    rc = lib.mk_ens_crps_bwd(eptr, 0 if dtype == "float32" else 1, bstride, estride, td.data_ptr(), wd.data_ptr(), gd.data_ptr(),
                             out.data_ptr(), E * (chw + gap), chw + gap, B, E, C, H, W, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "mk_ens_crps_bwd")
    torch.cuda.synchronize()
    check("gradient")
    host = out.cpu()
    if gap:
        want = torch.full((B, E, gap), SENTINEL, dtype=host.dtype)
        assert torch.equal(host[:, :, chw:].view(torch.uint8), want.view(torch.uint8)), "a store into the gap behind a member's block"
    return host[:, :, :chw].reshape(B, E, C, H, W)


@pytest.mark.parametrize("gap", [0, 3], ids=["flat", "gaps"])
@pytest.mark.parametrize("kind", ["ties", "nan"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_gradient_per_element(dev, shape, dtype, kind, gap):
    """``gap = 0`` is the ``[B * E, C, H, W]`` view of a model output; ``gap = 3`` is a member stride of ``C H W + 3`` on both sides."""
    ens, tar, wrow, gs = lc.problem(shape, dtype, kind)
    got = launch(dev, ens, tar, wrow, gs, dtype, gap)
    lc.assert_grad(got.float().numpy(), ens, tar, wrow, gs, dtype, f"{ids(shape)} {dtype} {kind} gap {gap}")
    if kind == "nan":
        B, E = shape[:2]
        assert int(torch.isnan(got).sum()) == E * len(set(p for p, _ in lc.nan_points(shape)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_runs_give_the_same_bits(dev, dtype):
    shape = (2, 5, 2, 8, 8)
    ens, tar, wrow, gs = lc.problem(shape, dtype, "nan")
    one, two = (launch(dev, ens, tar, wrow, gs, dtype, 3) for _ in range(2))
    assert torch.equal(one.view(torch.uint8), two.view(torch.uint8))


@pytest.mark.parametrize("cut", [4, 5])
@pytest.mark.parametrize("dtype", DTYPES)
def test_row_shards_are_slices_of_the_whole(dev, dtype, cut):
    shape = (2, 2, 2, 9, 37)
    ens, tar, wrow, gs = lc.problem(shape, dtype, "nan")
    whole = launch(dev, ens, tar, wrow, gs, dtype)
    for rows in (slice(0, cut), slice(cut, shape[3])):
        part = launch(dev, np.ascontiguousarray(ens[..., rows, :]), np.ascontiguousarray(tar[..., rows, :]), wrow[rows], gs, dtype)
        assert torch.equal(part.view(torch.uint8), whole[..., rows, :].contiguous().view(torch.uint8)), (cut, rows)


@pytest.mark.parametrize("case", REFUSED, ids=capi.case_ids(REFUSED))
def test_bad_argument_is_refused_before_any_launch(dev, case):
    capi.assert_refused(*case)


# ---------------------------------------------------------------------------- the op, capture, the handler behind a wrapper
def _on(dev, shape, dtype, kind):
    ens, tar, wrow, gs = lc.problem(shape, dtype, kind)
    return (torch.from_numpy(np.array(ens)).to(dev, getattr(torch, dtype)), torch.from_numpy(np.array(tar)).to(dev),
            torch.from_numpy(np.array(wrow)).to(dev), torch.from_numpy(np.array(gs)).to(dev))


@pytest.mark.parametrize("dtype", DTYPES)
def test_op_under_autograd_against_the_cpu_formulation(dev, monkeypatch, dtype):
    from makani_amd import ops
    shape = (2, 4, 3, 9, 37)
    B, E, C, H, W = shape
    ens, tar, wrow, gs = lc.problem(shape, dtype, "nan")
    # the CPU formulation on float64 members (the values of the rounded members, exactly)
    x64 = torch.from_numpy(np.array(ens)).double().requires_grad_(True)
    ref = ops._ensemble_crps_sums_torch(x64, torch.from_numpy(np.array(tar)), torch.from_numpy(np.array(wrow)))
    (ref[..., :2] * torch.from_numpy(np.array(gs))).sum().backward()
    monkeypatch.setenv("MK_ENS_LOSS", "hip")
    e, t, w, g = _on(dev, shape, dtype, "nan")
    x = e.reshape(B * E, C, H, W).requires_grad_(True)
    s, sums = ops.ensemble_crps_sums(x, t, w, with_sums=True)
    assert "_EnsCrpsSumsBackward" in node_kinds(s) and s.shape == (B, C, 2) and s.dtype == torch.float64
    (s * g).sum().backward()
    torch.cuda.synchronize()
    assert x.grad.shape == x.shape and x.grad.dtype == x.dtype and x.grad.is_contiguous()
    assert torch.equal(sums[..., :2].contiguous().view(torch.int64), s.detach().view(torch.int64)) and not sums.requires_grad
    ec.assert_sums(sums.cpu().numpy(), ens, tar, wrow, f"op {dtype}")
    got = x.grad.float().cpu().reshape(shape).numpy()
    lc.assert_grad(got, ens, tar, wrow, gs, dtype, f"op {dtype}")
    want = x64.grad.numpy()
    ok = ~np.isnan(want)
    assert np.array_equal(np.isnan(got), ~ok)
    assert (np.abs(got - want)[ok] <= (lc.ROUND[dtype] + 2.0 ** -40) * np.abs(want)[ok]).all()
    # the torch formulation on the device takes the other node
    monkeypatch.setenv("MK_ENS_LOSS", "torch")
    assert "_EnsCrpsSumsBackward" not in node_kinds(ops.ensemble_crps_sums(x, t, w))


def test_captured_forward_and_backward_replay_to_the_eager_bits(dev, monkeypatch):
    from makani_amd import ops
    monkeypatch.setenv("MK_ENS_LOSS", "hip")
    shape = (2, 4, 3, 9, 37)
    B, E, C, H, W = shape
    fresh = [_on(dev, shape, "bfloat16", kind) for kind in ("ties", "nan")]
    w, g = fresh[0][2], fresh[0][3]

    def step(x, t):
        s = ops.ensemble_crps_sums(x, t, w)
        (s * g).sum().backward()
        return s.detach()

    eager = []
    for e, t, _, _ in fresh:
        x = e.reshape(B * E, C, H, W).clone().requires_grad_(True)
        eager.append((step(x, t), x.grad.clone()))
    x = torch.zeros(B * E, C, H, W, dtype=torch.bfloat16, device=dev).requires_grad_(True)
    t = torch.zeros(B, C, H, W, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(x, t)                                   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    x.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = step(x, t)
    for (e, tt, _, _), (s_want, g_want) in zip(fresh, eager):
        with torch.no_grad():
            x.copy_(e.reshape(B * E, C, H, W))
            t.copy_(tt)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(s.view(torch.int64), s_want.view(torch.int64))
        assert torch.equal(x.grad.view(torch.int16), g_want.view(torch.int16))


def test_almost_fair_crps_trains_a_one_layer_model_through_the_step_wrapper(dev, monkeypatch):
    """Batch B E = 2 x 3 on 9 x 16: the parameter gradients are finite and equal those of the ``MK_ENS_LOSS=torch`` run within
    1e-5 relative L2 (the fp32 rounding of the per-element gradients, summed by the model's backward)."""
    from makani_amd.ensemble import perturb_members
    from makani_amd.losses import LossHandler
    from makani_amd.stepper import SingleStepWrapper
    from test_lploss_cpu import CHANNELS, make_params as loss_params
    from test_stepper_cpu import make_params, toy_model
    H, W, B, E, C = 9, 16, 2, 3, len(CHANNELS)
    gen = torch.Generator().manual_seed(21)
    wgt, bias = 0.3 * torch.randn(C, C, 1, 1, generator=gen), 0.1 * torch.randn(C, generator=gen)
    inp, tar = torch.randn(B, C, H, W, generator=gen).to(dev), torch.randn(B, C, H, W, generator=gen).to(dev)
    params = loss_params("weighted almost-fair ensemble crps", H, W)
    params.ensemble_size = E
    handler = LossHandler(params).to(dev).train()
    assert handler.loss_obj.alpha == 0.95
    members = perturb_members(inp, E, 0.5, generator=torch.Generator(device=dev).manual_seed(4))
    grads = {}
    for mode in ("hip", "torch"):
        monkeypatch.setenv("MK_ENS_LOSS", mode)
        wrap = SingleStepWrapper(make_params(H, W), lambda: toy_model(wgt, bias)).to(dev).train()
        loss = handler(wrap(members), tar, None)
        assert ("_EnsCrpsSumsBackward" in node_kinds(loss)) == (mode == "hip")
        loss.backward()
        grads[mode] = [p.grad.detach().double().cpu() for p in wrap.parameters()]
        assert len(grads[mode]) == 2 and all(bool(torch.isfinite(gr).all()) and float(gr.abs().max()) > 0 for gr in grads[mode])
    for a, b in zip(grads["hip"], grads["torch"]):
        err = float((a - b).norm() / b.norm())
        print(f"parameter gradient {tuple(a.shape)}: hip against torch, relative L2 {err:.2e}")
        assert err <= 1e-5
