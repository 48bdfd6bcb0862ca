"""CPU tests of the ensemble CRPS training loss: the torch formulation (``ops._ensemble_crps_sums_torch``, the all-pairs
expression under autograd) against the numpy restatement of tests/ens_loss_checks.py, which forms the gradient from counts
and shares no step with autograd or a sort; ``EnsembleCRPSLoss`` and the ``crps`` strings of ``LossHandler``;
``perturb_members``; the C signature and the refusals of ``mk_ens_crps_bwd`` (before any launch: no GPU needed)."""
import ctypes

import numpy as np
import pytest
import torch

import capi_checks as capi
import ens_checks as ec
import ens_loss_checks as lc
from test_lploss_cpu import fields, make_params

MEMBERS = [1, 2, 3, 5, 16, 17]
DTYPES = ["float32", "bfloat16"]
KINDS = ["normal", "ties", "nan"]


def _torch(a, dtype=None):
    t = torch.from_numpy(np.array(a))
    return t if dtype is None else t.to(dtype)


def _run64(ens, tar, wrow, gs):
    """(sums [B, C, 4], gradient [B, E, C, H, W]) of the torch formulation on float64 members, as numpy."""
    from makani_amd import ops
    x = _torch(ens, torch.float64).requires_grad_(True)
    out = ops._ensemble_crps_sums_torch(x, _torch(tar), _torch(wrow))
    assert out.shape == tar.shape[:2] + (4,) and out.dtype == torch.float64
    (out[..., :2] * _torch(gs)).sum().backward()
    return out.detach().numpy(), x.grad.numpy()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("E", MEMBERS)
def test_torch_formulation_meets_the_reference(E, dtype, kind):
    """Members rounded to ``dtype`` and widened (exact): sums within ``ens_checks.bound``, gradient within the float64 bound,
    zero exactly where sgn = 0 and L = G, NaN at every member of a NaN point and nowhere else."""
    shape = (2, E, 2, 9, 37)
    ens, tar, wrow, gs = lc.problem(shape, dtype, kind)
    if kind == "ties":
        tied = (ens[:, :, None] == ens[:, None]).sum(axis=(1, 2)) > E          # a pair of different members is equal
        assert E == 1 or tied.mean() >= 0.2
    sums, grad = _run64(ens, tar, wrow, gs)
    what = f"E={E} {dtype} {kind}"
    ec.assert_sums(sums, ens, tar, wrow, what)
    lc.assert_grad(grad, ens, tar, wrow, gs, lc.float64_bound(ens, wrow, gs), what)
    if kind == "nan":
        for (b, c, h, w), _ in lc.nan_points(shape):
            assert np.isnan(grad[b, :, c, h, w]).all() and np.isnan(sums[b, c]).all()
        assert int(np.isnan(grad).sum()) == 2 * E


@pytest.mark.parametrize("E", [2, 5, 16])
def test_member_gradients_add_up_to_the_sign_term(E):
    """``sum_e (L_e - G_e) = 0`` at every point, so ``sum_e grad_e = w gs0 sum_e sgn(x_e - y) / E``.  The bound: E elements,
    each within ``float64_bound`` = 16 u T of its reference (T = |w| (|gs0| / E + 2 |gs1| / E)), added in float64, which
    costs at most (E - 1) u sum_e |r_e| <= E^2 u T more: (16 E + E^2) u T."""
    ens, tar, wrow, gs = lc.problem((2, E, 2, 9, 37), "float32", "ties")
    _, grad = _run64(ens, tar, wrow, gs)
    L, G = lc.counts(ens)
    assert ((L - G).sum(axis=1) == 0).all()
    w = wrow.astype(np.float64).reshape(1, 1, -1, 1)
    want = w * gs[:, :, None, None, 0] * lc.signs(ens, tar).sum(axis=1) / E
    lim = (16 * E + E * E) / 16 * lc.float64_bound(ens, wrow, gs)[:, 0]
    assert (np.abs(grad.sum(axis=1) - want) <= lim).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_op_on_cpu_tensors_of_the_members_dtype(dtype, monkeypatch):
    """``ops.ensemble_crps_sums`` on a ``[B * E, C, H, W]`` leaf of the members' dtype: the gradient arrives in that dtype,
    rounded once; walking the channels in chunks (with recomputation in the backward) gives the same bits."""
    from makani_amd import ops
    shape = (2, 3, 3, 9, 37)
    B, E, C, H, W = shape
    ens, tar, wrow, gs = lc.problem(shape, dtype, "ties")
    res = []
    for chunk in (ops._ENS_TORCH_CHUNK, B * E * E * H * W):          # all channels at once; one channel per chunk
        monkeypatch.setattr(ops, "_ENS_TORCH_CHUNK", chunk)
        x = _torch(ens, getattr(torch, dtype)).reshape(B * E, C, H, W).requires_grad_(True)
        s, sums = ops.ensemble_crps_sums(x, _torch(tar), _torch(wrow), with_sums=True)
        assert s.shape == (B, C, 2) and sums.shape == (B, C, 4) and not sums.requires_grad
        assert torch.equal(sums[..., :2], s.detach())
        (s * _torch(gs)).sum().backward()
        assert x.grad.dtype == x.dtype and x.grad.shape == x.shape
        lc.assert_grad(x.grad.float().reshape(shape).numpy(), ens, tar, wrow, gs, dtype, f"op {dtype}")
        res.append((s.detach(), x.grad))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_op_refuses_bad_shapes_and_an_unknown_switch(monkeypatch):
    from makani_amd import ops
    ens, tar, wrow = torch.zeros(2, 3, 2, 5, 7), torch.zeros(2, 2, 5, 7), torch.ones(5)
    assert "MK_ENS_LOSS" in ops.KNOBS and ops.ENS_LOSS_DEFAULT in ops.KNOBS["MK_ENS_LOSS"] and ops.ENS_LOSS_MAX_MEMBERS == 16
    with pytest.raises(ValueError, match="must be"):
        ops.ensemble_crps_sums(ens[:, :, :1], tar, wrow)
    with pytest.raises(ValueError, match="latitude rows"):
        ops.ensemble_crps_sums(ens, tar, wrow[:4])
    monkeypatch.setenv("MK_ENS_LOSS", "fast")
    with pytest.raises(ValueError, match="MK_ENS_LOSS"):
        ops.ensemble_crps_sums(ens, tar, wrow)


# ---------------------------------------------------------------------------------------------------------------------
# EnsembleCRPSLoss and LossHandler
# ---------------------------------------------------------------------------------------------------------------------
H, W, B, C = 9, 16, 2, 6
SPELLINGS = {"ensemble crps": 0.0, "fair ensemble crps": 1.0, "almost-fair ensemble crps": 0.95}


def _crps_params(spec, E, n_future=0, **kw):
    params = make_params(spec, H, W, n_future=n_future, **kw)
    params.ensemble_size = E
    return params


def _ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


@pytest.mark.parametrize("n_future", [0, 1])
@pytest.mark.parametrize("spec", list(SPELLINGS))
def test_equal_members_give_the_absolute_geometric_l1_loss(spec, n_future):
    from makani_amd.losses import LossHandler
    E, CC = 3, C * (n_future + 1)
    prd, tar = fields((B, CC, H, W), seed=3)
    for prefix in ("", "weighted "):
        crps = LossHandler(_crps_params(prefix + spec, E, n_future)).train()
        l1 = LossHandler(make_params(prefix + "absolute geometric l1", H, W, n_future=n_future)).train()
        assert crps.loss_obj.members == E and crps.loss_obj.alpha == SPELLINGS[spec]
        assert crps.loss_obj.kappa == 1.0 + SPELLINGS[spec] / (E - 1)
        got = crps(prd.repeat_interleave(E, dim=0), tar, None)
        want = l1(prd, tar, None)
        assert got.dtype == torch.float32 and got.shape == ()
        assert abs(float(got) - float(want)) <= _ulp32(float(want)), (spec, prefix, float(got), float(want))
        assert crps.loss_obj.last_sums.shape == (B, CC, 4)
        assert float(crps.loss_obj.last_sums[..., 1].abs().max()) == 0.0 and float(crps.loss_obj.last_sums[..., 3].abs().max()) == 0.0


@pytest.mark.parametrize("spec", list(SPELLINGS))
def test_handler_loss_and_gradient_against_the_reference(spec):
    """Different members: the loss is ``sum_bc chw_c (S0 - kappa / 2 S1)`` of the numpy all-pairs sums, its gradient the closed
    form with ``gs = chw (1, -kappa / 2)``."""
    from makani_amd.losses import LossHandler
    E = 4
    shape = (B, E, C, H, W)
    ens, tar, _, _ = lc.problem(shape, "float32", "ties")
    params = _crps_params("weighted pole-masked " + spec, E)
    params.crps_alpha = 0.5 if "almost" in spec else 0.9          # read for "almost-fair" only
    handler = LossHandler(params).train()
    kappa = 1.0 + {"ensemble crps": 0.0, "fair ensemble crps": 1.0, "almost-fair ensemble crps": 0.5}[spec] / (E - 1)
    assert handler.loss_obj.kappa == kappa
    x = _torch(ens).reshape(B * E, C, H, W).requires_grad_(True)
    loss = handler(x, _torch(tar), None)
    loss.backward()
    wrow = handler.loss_obj.wrow.numpy()
    assert wrow[0] == 0.0 and wrow[-1] == 0.0 and (wrow[1:-1] > 0).all()            # pole-masked
    chw = (handler.channel_weights * handler.multistep_weight).reshape(-1).double().numpy()
    assert chw[1] == 0.0                                                             # "sst" under automatic weights
    s = ec.sums(ens, tar, wrow)
    want = float((chw * (s[..., 0] - 0.5 * kappa * s[..., 1])).sum())
    assert abs(float(loss.detach()) - want) <= _ulp32(want)          # float64 sums, rounded to fp32 once
    gs = np.broadcast_to(chw[None, :, None] * np.array([1.0, -0.5 * kappa]), (B, C, 2))
    lc.assert_grad(x.grad.reshape(shape).numpy(), ens, tar, wrow, gs, "float32", spec)


def test_handler_value_errors():
    from makani_amd.ensemble import EnsembleCRPSLoss
    from makani_amd.losses import LossHandler
    with pytest.raises(ValueError, match="ensemble_size"):
        LossHandler(make_params("fair ensemble crps", H, W))
    with pytest.raises(ValueError, match="squared"):
        LossHandler(_crps_params("squared ensemble crps", 4))
    with pytest.raises(ValueError, match="2 members"):
        LossHandler(_crps_params("fair ensemble crps", 1))
    assert LossHandler(_crps_params("ensemble crps", 1)).loss_obj.kappa == 1.0
    with pytest.raises(ValueError, match="members of a target"):
        LossHandler(_crps_params("ensemble crps", 4))(torch.zeros(6, C, H, W), torch.zeros(2, C, H, W), None)
    with pytest.raises(ValueError, match="alpha"):
        EnsembleCRPSLoss((H, W), (H, W), (0, 0), 4, alpha=1.5)


def test_perturb_members_is_the_rollouts_perturbation(tmp_path):
    from makani_amd.ensemble import perturb_members
    from makani_amd.inference import EnsembleRollout
    from test_rollout_cpu import build, make_params as rollout_params, make_problem
    Hh, Ww, E, T = 12, 24, 4, 2
    params = rollout_params(Hh, Ww, tmp_path, n_history=T - 1)
    prob = make_problem(2, T, Hh, Ww, 1, seed=1)
    wrap, _, _ = build(params, prob)
    ro = EnsembleRollout(params, wrap, None, E, noise_std=0.25)
    want = ro.perturb(prob.inp, generator=torch.Generator().manual_seed(5))
    flat = wrap.preprocessor.flatten_history(prob.inp)
    got = perturb_members(flat, E, 0.25, generator=torch.Generator().manual_seed(5))
    assert got.shape == (2 * E,) + tuple(flat.shape[1:]) and torch.equal(got, want)
    assert torch.equal(got[0], flat[0]) and torch.equal(got[E], flat[1]) and not torch.equal(got[1], got[0])
    assert torch.equal(perturb_members(flat, E, 0.0), flat.repeat_interleave(E, dim=0))
    assert torch.equal(perturb_members(flat, 1, 0.25), flat)


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_signature_of_the_entry_point():
    from makani_amd import _lib
    p, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert _lib.SIGNATURES["mk_ens_crps_bwd"] == (i, [p, i, ll, ll, p, p, p, p, ll, ll, i, i, i, i, i, p])


_A = capi.A
_OK = dict(ens=_A, dtype=0, bstride=3 * 80, estride=80, tar=_A, wrow=_A, gs=_A, gens=_A, gbstride=3 * 80, gestride=80, B=2, E=3, C=2,
           H=5, W=8)


def _args(**kw):
    return tuple(dict(_OK, **kw).values())


_E_MSG = "E outside 2 ... 16 (all pairs of a point are compared in registers)"
_BLOCK = "a member's [C][H][W] block must be contiguous: strides below C * H * W"
REFUSED = [
    ("mk_ens_crps_bwd", _args(ens=_A + 2), "ensemble or its gradient not aligned to its element"),
    ("mk_ens_crps_bwd", _args(gens=_A + 2), "ensemble or its gradient not aligned to its element"),
    ("mk_ens_crps_bwd", _args(dtype=1, gens=_A + 1), "ensemble or its gradient not aligned to its element"),
    ("mk_ens_crps_bwd", _args(tar=_A + 2), "fp32 stream not 4-byte aligned"),
    ("mk_ens_crps_bwd", _args(wrow=_A + 2), "fp32 stream not 4-byte aligned"),
    ("mk_ens_crps_bwd", _args(gs=_A + 4), "64-bit buffer not 8-byte aligned"),
    ("mk_ens_crps_bwd", _args(gs=None), "null pointer"),
    ("mk_ens_crps_bwd", _args(gens=None), "null pointer"),
    ("mk_ens_crps_bwd", _args(dtype=2), "dtype must be 0 (fp32) or 1 (bf16)"),
    ("mk_ens_crps_bwd", _args(E=1), _E_MSG),
    ("mk_ens_crps_bwd", _args(E=17, bstride=17 * 80, gbstride=17 * 80), _E_MSG),
    ("mk_ens_crps_bwd", _args(estride=79), _BLOCK),
    ("mk_ens_crps_bwd", _args(gestride=79), _BLOCK),
    ("mk_ens_crps_bwd", _args(gbstride=1 << 44), "stride too large"),
    ("mk_ens_crps_bwd", _args(bstride=239), "members of different samples overlap: need bstride >= E * estride or estride >= B * bstride"),
    ("mk_ens_crps_bwd", _args(gbstride=239),
     "gradients of different samples overlap: need gbstride >= E * gestride or gestride >= B * gbstride"),
    ("mk_ens_crps_bwd", _args(W=0), "bad sizes"),
    ("mk_ens_crps_bwd", _args(B=65536), "B or C beyond the grid range"),
]


@pytest.mark.parametrize("case", REFUSED, ids=capi.case_ids(REFUSED))
def test_bad_argument_is_refused_before_any_launch(case):
    capi.assert_refused(*case)
