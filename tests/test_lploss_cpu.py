"""CPU tests of the Lp training losses on their two-sum form (ops.geo_lp_sums, GeometricLpLoss, LossHandler).

The yardstick for values is oracle.losses.geometric_lp_loss / quad_weight in float64 on the full field; for gradients it
is the closed form  s0 = sum q |prd - tar|^p,  s1 = sum q |tar|^p,  norm = s0 or s0 / s1, root unless squared,
reduce(chw * norm), differentiated by torch in float64 (``closed_form``).  The helpers here also serve
test_lploss_dist_cpu.py and test_lploss_gpu.py.

Tolerances are the project's for the CPU and gloo paths (test_distributed_cpu._body_loss): loss 2e-6 relative, gradient
1e-6 relative L2.  Inputs are torch.randn fields with a fixed seed; no element of prd - tar is zero (asserted), so the
p = 1 gradient has no tie and every element is compared."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import capi_checks as capi

from oracle import losses as ol

LOSS_TOL, GRAD_TOL = 2e-6, 1e-6
SEED, SHAPE = 12, (2, 6, 33, 61)


def rel(got, want):
    got, want = torch.as_tensor(got).double().reshape(-1), torch.as_tensor(want).double().reshape(-1)
    return float((got - want).norm() / want.norm())


def fields(shape=SHAPE, seed=SEED):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)


def no_ties(prd, tar):
    """No element of prd - tar is zero, in fp32 and with the prediction rounded to bf16."""
    return int(((prd - tar) == 0).sum()) == 0 and int(((prd.bfloat16().float() - tar) == 0).sum()) == 0


def closed_form(prd, tar, q, chw, p, absolute, squared, size_average=False, reduction=True):
    """(loss, d loss / d prd) in float64 by torch autograd on the closed form, on the device of ``prd``; q [H, W], chw
    broadcastable to [B, C]."""
    x = prd.detach().double().clone().requires_grad_(True)
    t, q, chw = tar.detach().double(), torch.as_tensor(q).double().to(prd.device), torch.as_tensor(chw).double().to(prd.device)
    s0 = (q * (x - t).abs() ** p).sum((-2, -1))
    s1 = (q * t.abs() ** p).sum((-2, -1))
    norm = s0 if absolute else s0 / s1
    if not squared:
        norm = norm ** (1.0 / p)
    out = chw * norm
    loss = out if not reduction else (out.mean() if size_average else out.sum())
    loss.sum().backward()
    return loss.detach(), x.grad


def sums64(prd, tar, wrow, p):
    """[B, C, 2] float64 sums on the tensors' device, one sample at a time."""
    w = wrow.double().view(1, -1, 1)
    out = []
    for b in range(prd.shape[0]):
        d, t = prd[b].double() - tar[b].double(), tar[b].double()
        out.append(torch.stack([(w * d.abs() ** p).sum((-2, -1)), (w * t.abs() ** p).sum((-2, -1))], dim=-1))
    return torch.stack(out)


CHANNELS = ["u10m", "sst", "t2m", "z500", "q700", "v10m"]
UNEQUAL = [0.5, 1.0, 2.0, 0.25, 1.5, 3.0]

# spelling -> (p, absolute, squared, pole mask, channel weights before normalisation / None = uniform)
SPECS = {
    "l2": (2, False, False, 0, None),
    "geometric l2": (2, False, False, 0, None),
    "absolute geometric l1": (1, True, False, 0, None),
    "weighted squared geometric l2": (2, False, True, 0, UNEQUAL),
    "weighted pole-masked geometric l2": (2, False, False, 1, [1.0, 0.0, 1.0, 1.0, 1.0, 1.0]),
    "weighted squared temp-std geometric l2": (2, False, True, 0, UNEQUAL),
}


def make_params(spec, H, W, n_future=0, img_shape=None, crop_offset=(0, 0), grid="equiangular", tmp_path=None):
    img = img_shape or (H, W)
    auto = "pole-masked" in spec
    params = SimpleNamespace(loss=spec, n_future=n_future, img_shape_x=img[0], img_shape_y=img[1], img_crop_shape_x=H,
                             img_crop_shape_y=W, img_crop_offset_x=crop_offset[0], img_crop_offset_y=crop_offset[1],
                             N_out_channels=len(CHANNELS), channel_names=CHANNELS,
                             channel_weights="auto" if auto else UNEQUAL, model_grid_type=grid)
    if "temp-std" in spec:
        # statistics of a nine-channel data set of which the model predicts six
        rng = np.random.default_rng(5)
        params.out_channels = [0, 2, 3, 5, 6, 8]
        params.dt = 4
        params.global_stds_path = str(tmp_path / "global_stds.npy")
        params.time_diff_stds_path = str(tmp_path / "time_diff_stds.npy")
        np.save(params.global_stds_path, rng.uniform(0.5, 2.0, (1, 9, 1, 1)))
        np.save(params.time_diff_stds_path, rng.uniform(0.1, 0.5, (1, 9, 1, 1)))
    return params


def expected_chw(params, training):
    """[1, C * steps] float64 channel weights of losses.py:60-90 and 160-163, restated in numpy."""
    _, _, squared, _, weights = SPECS[params.loss]
    chw = np.ones(len(CHANNELS)) if weights is None else np.asarray(weights, np.float64)
    chw = chw / chw.sum()
    if "temp-std" in params.loss:
        gs = np.load(params.global_stds_path).reshape(-1)[params.out_channels]
        ts = math.sqrt(params.dt) * np.load(params.time_diff_stds_path).reshape(-1)[params.out_channels]
        tw = gs / (ts + 1e-6)
        chw = chw * (tw ** 2 if squared else tw)
    if training:
        chw = (np.ones((params.n_future + 1, 1)) / (params.n_future + 1) * chw[None, :]).reshape(-1)
    return chw.reshape(1, -1)


def expected_q(params):
    rule = "legendre-gauss" if params.model_grid_type == "legendre_gauss" else "naive"
    return ol.quad_weight(rule, (params.img_shape_x, params.img_shape_y), (params.img_crop_shape_x, params.img_crop_shape_y),
                          (params.img_crop_offset_x, params.img_crop_offset_y), normalize=True,
                          pole_mask=SPECS[params.loss][3])


def expected_loss(params, prd, tar, training):
    """(oracle value, closed-form gradient) of the handler's loss on the full field."""
    p, absolute, squared, _, _ = SPECS[params.loss]
    q, chw = expected_q(params), expected_chw(params, training)
    want = ol.geometric_lp_loss(prd.double().numpy(), tar.double().numpy(), chw, q, p=p, absolute=absolute, squared=squared)
    loss, grad = closed_form(prd, tar, q, chw, p, absolute, squared)
    assert abs(float(loss) - want) < 1e-12 * abs(want)                # the closed form is the oracle's arithmetic
    return want, grad


# --------------------------------------------------------------------------- the op
@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_geo_lp_sums_cpu(p, dtype):
    from makani_amd import ops
    prd, tar = fields()
    assert no_ties(prd, tar)
    prd = prd.to(dtype)
    wrow = torch.rand(SHAPE[2], generator=torch.Generator().manual_seed(3)).double() + 0.1
    x = prd.clone().requires_grad_(True)
    got = ops.geo_lp_sums(x, tar, wrow, p)
    assert got.dtype == torch.float64 and got.shape == (SHAPE[0], SHAPE[1], 2)
    want = sums64(prd, tar, wrow, p)
    assert float(((got.detach() - want).abs() / want.abs()).max()) < 1e-12
    # differentiable: an arbitrary function of the sums against the same function of the float64 restatement
    coef = torch.rand(SHAPE[0], SHAPE[1], 2, generator=torch.Generator().manual_seed(4)).double() + 0.5
    (coef * got).sum().backward()
    x64 = prd.double().requires_grad_(True)
    w = wrow.view(1, 1, -1, 1)
    (coef[..., 0] * (w * (x64 - tar.double()).abs() ** p).sum((-2, -1))).sum().backward()
    assert x.grad.dtype == dtype
    assert rel(x.grad, x64.grad) < (GRAD_TOL if dtype == torch.float32 else GRAD_TOL + 2.0 ** -9)


def test_geo_lp_sums_target_gradient_and_errors():
    from makani_amd import ops
    prd, tar = fields((1, 2, 9, 7))
    wrow = torch.ones(9)
    t = tar.clone().requires_grad_(True)
    ops.geo_lp_sums(prd, t, wrow, 2).sum().backward()
    want = 2.0 * (tar.double() - prd.double()) + 2.0 * tar.double()
    assert t.grad is not None and rel(t.grad, want) < GRAD_TOL
    with pytest.raises(ValueError, match="p must be 1 or 2"):
        ops.geo_lp_sums(prd, tar, wrow, 3)
    with pytest.raises(ValueError, match="latitude rows"):
        ops.geo_lp_sums(prd, tar, torch.ones(8), 2)
    with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
        ops.geo_lp_sums(prd[0], tar[0], wrow, 2)


# --------------------------------------------------------------------------- the loss object
@pytest.mark.parametrize("rule", ["naive", "clenshaw-curtiss", "legendre-gauss"])
@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("absolute", [False, True])
@pytest.mark.parametrize("squared", [False, True])
def test_geometric_lp_loss_cpu(rule, p, absolute, squared):
    from makani_amd.losses import GeometricLpLoss
    B, C, H, W = SHAPE
    prd, tar = fields()
    chw = torch.rand(1, C, generator=torch.Generator().manual_seed(6)) + 0.1
    kw = dict(img_shape=(H + 2, W + 3), crop_shape=(H, W), crop_offset=(1, 2))
    q = ol.quad_weight(rule, kw["img_shape"], kw["crop_shape"], kw["crop_offset"], normalize=True, pole_mask=2)
    loss = GeometricLpLoss(p=p, absolute=absolute, squared=squared, pole_mask=2, quadrature_rule=rule, **kw)
    x = prd.clone().requires_grad_(True)
    out = loss(x, tar, chw)
    out.backward()
    assert out.dtype == torch.float32 and out.dim() == 0
    want = ol.geometric_lp_loss(prd.numpy(), tar.numpy(), chw.numpy(), q, p=p, absolute=absolute, squared=squared)
    assert abs(float(out.detach()) - want) < LOSS_TOL * abs(want)
    assert rel(x.grad, closed_form(prd, tar, q, chw, p, absolute, squared)[1]) < GRAD_TOL


def test_geometric_lp_loss_reductions_and_other_p():
    from makani_amd.losses import GeometricLpLoss
    B, C, H, W = SHAPE
    prd, tar = fields()
    chw = torch.rand(1, C, generator=torch.Generator().manual_seed(6)) + 0.1
    q = ol.quad_weight("naive", (H, W), (H, W), (0, 0), normalize=True)
    kw = dict(img_shape=(H, W), crop_shape=(H, W), crop_offset=(0, 0))
    per = GeometricLpLoss(p=2, reduction=False, **kw)(prd, tar, chw)
    assert per.shape == (B, C) and per.dtype == torch.float32
    assert rel(per, closed_form(prd, tar, q, chw, 2, False, False, reduction=False)[0]) < LOSS_TOL
    avg = GeometricLpLoss(p=1, size_average=True, absolute=True, **kw)(prd, tar, chw)
    want = ol.geometric_lp_loss(prd.numpy(), tar.numpy(), chw.numpy(), q, p=1, absolute=True, size_average=True)
    assert abs(float(avg) - want) < LOSS_TOL * abs(want)
    # p = 3 has no kernel and keeps the torch formulation
    cube = GeometricLpLoss(p=3, **kw)
    assert not cube.has_sums(prd, tar)
    want = ol.geometric_lp_loss(prd.numpy(), tar.numpy(), chw.numpy(), q, p=3)
    assert abs(float(cube(prd, tar, chw)) - want) < 1e-5 * abs(want)


# --------------------------------------------------------------------------- the handler
@pytest.mark.parametrize("spec", list(SPECS))
@pytest.mark.parametrize("n_future", [0, 1])
@pytest.mark.parametrize("training", [True, False])
def test_loss_handler_cpu(spec, n_future, training, tmp_path):
    from makani_amd.losses import LossHandler
    B, C, H, W = SHAPE
    cropped = spec in ("geometric l2", "weighted squared temp-std geometric l2")
    params = make_params(spec, H, W, n_future=n_future, tmp_path=tmp_path,
                         **(dict(img_shape=(H + 2, W + 3), crop_offset=(1, 2), grid="legendre_gauss") if cropped else {}))
    steps = n_future + 1 if training else 1                # training stacks the steps of a rollout along the channels
    prd, tar = fields((B, C * steps, H, W))
    assert no_ties(prd, tar)
    handler = LossHandler(params)
    handler.train(training)
    x = prd.clone().requires_grad_(True)
    out = handler(x, tar, None)
    out.backward()
    want, gwant = expected_loss(params, prd, tar, training)
    assert out.dtype == torch.float32
    assert abs(float(out.detach()) - want) < LOSS_TOL * abs(want)
    assert rel(x.grad, gwant) < GRAD_TOL


# ---------------------------------------------------------------------------------------------------------------------
# misaligned pointers: refused by the host checks, with the message of the check (tests/capi_checks.py)
# ---------------------------------------------------------------------------------------------------------------------
_A = capi.A
MISALIGNED = [      # entry point, its arguments in front of the stream with one pointer moved off its alignment, the refusal
    ("mk_geo_lp_sums", (_A + 2, 0, _A, _A, _A, _A, 2, 1, 2, 4, 8), "prediction not aligned to its element"),
    ("mk_geo_lp_sums", (_A, 0, _A, _A + 2, _A, _A, 1, 1, 2, 4, 8), "fp32 stream not 4-byte aligned"),
    ("mk_geo_lp_sums", (_A + 2, 1, _A, _A, _A, _A + 4, 2, 1, 2, 4, 8), "fp64 buffer not 8-byte aligned"),
    ("mk_geo_lp_bwd", (_A, 0, _A, _A, _A, _A + 2, 2, 1, 2, 4, 8), "prediction or its gradient not aligned to its element"),
    ("mk_geo_lp_bwd", (_A, 1, _A, _A, _A + 2, _A, 1, 1, 2, 4, 8), "fp32 stream not 4-byte aligned"),
]


@pytest.mark.parametrize("case", MISALIGNED, ids=capi.case_ids(MISALIGNED))
def test_misaligned_pointer_is_refused_before_any_launch(case):
    capi.assert_refused(*case)
