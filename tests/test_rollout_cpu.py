"""CPU tests of the autoregressive rollout (makani_amd/inference.py on ops.rollout_tail's torch formulation).

The yardstick is the loop of the reference's ``inferencer.py:167-206`` written out here with this package's
``SingleStepWrapper``, ``LossHandler``, ``MetricsHandler.update``, ``(pred - targ) ** 2`` and ``append_history`` -- with
the two documented deviations: the error map and the curve take every sample (in ascending ``b``), and the held
channels are a parameter.  Both sides are the same torch operations in the same order, so predictions, the handler's
buffers and the map must be equal bit for bit; ``RMSE_over_time`` comes from float64 sums and is held to 1e-6 of the
float64 restatement."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import capi_checks as capi

from test_stepper_cpu import make_params as stepper_params, toy_model

NAMES = ["u10m", "t2m", "z500"]
C, CU, CS = 3, 1, 3
TIME_TOL = 1e-6


def make_params(H, W, tmp_path, steps=3, **kw):
    """The trainer's parameter object as the wrappers, the metrics handler, the loss handler and the rollout read it:
    C = 3 predicted channels, one unpredicted, three static (linear grid + orography)."""
    oro = tmp_path / f"oro_{H}x{W}.npy"
    if not oro.exists():
        np.save(oro, (3000.0 * torch.rand(H, W, generator=torch.Generator().manual_seed(H * W))).numpy())
    p = stepper_params(H, W, add_grid=True, gridtype="linear", add_orography=True, orography_path=str(oro), **kw)
    p.__dict__.update(log_to_screen=False, log_to_wandb=False, channel_names=list(NAMES), dt=1, dhours=6,
                      split_data_channels=False, valid_autoreg_steps=steps - 1, N_out_channels=C, img_crop_shape_x=H,
                      img_crop_shape_y=W, img_crop_offset_x=0, img_crop_offset_y=0, loss="geometric l2", channel_weights="auto")
    return p


def make_problem(B, T, H, W, steps, seed):
    g = torch.Generator().manual_seed(seed)
    cin = T * (C + CU) + CS
    return SimpleNamespace(
        w=torch.randn(C, cin, 1, 1, generator=g) / cin ** 0.5, b=0.1 * torch.randn(C, generator=g),
        inp=torch.randn(B, T, C, H, W, generator=g), tar=torch.randn(B, steps, C, H, W, generator=g),
        xz=torch.randn(B, T, CU, H, W, generator=g), yz=torch.randn(B, steps, CU, H, W, generator=g),
        clim=0.5 * torch.randn(C, H, W, generator=g), mult=1.0 + torch.rand(C, generator=g))


def build(params, prob, device="cpu", shard=None, model=None):
    """(wrapper, metrics handler, loss handler) on ``device``; ``shard`` cuts this rank's piece of a full field."""
    from makani_amd.losses import LossHandler
    from makani_amd.metric import MetricsHandler
    from makani_amd.stepper import SingleStepWrapper
    shard = shard or (lambda x: x)
    torch.manual_seed(1234)                  # a model handle that draws its weights draws the same ones every time
    wrap = SingleStepWrapper(params, model or (lambda: toy_model(prob.w, prob.b))).to(device)
    wrap.eval()
    wrap.preprocessor.cache_unpredicted_features(None, None, shard(prob.xz).clone().to(device), shard(prob.yz).clone().to(device))
    h = MetricsHandler(params, prob.mult, prob.clim, torch.device(device))
    h.initialize_buffers()
    h.zero_buffers()
    loss = LossHandler(params).to(device)
    loss.eval()
    return wrap, h, loss


def handwritten(wrap, h, loss, inp, tar, held=()):
    """inferencer.py:167-206 (scored) with this package's modules; every sample adds to the map and the curve."""
    pp = wrap.preprocessor
    B, steps, Cn, H, W = tar.shape
    space = torch.zeros(Cn, H, W, dtype=torch.float32, device=tar.device)
    time64 = torch.zeros(steps, Cn, dtype=torch.float64, device=tar.device)
    preds = []
    inpt = pp.flatten_history(inp)
    for idt in range(steps):
        targ = tar[:, idt]
        pred = wrap(inpt)
        if held:
            pred = pred.float().clone()
            pred[:, list(held)] = pp.expand_history(inpt, pp.n_history + 1)[:, -1][:, list(held)]
        lval = loss(pred, targ, inpt)
        h.update(pred, targ, lval, idt)
        sqdif = (pred - targ) ** 2
        for b in range(B):
            space += sqdif[b]
        time64[idt] += ((pred.double() - targ.double()) ** 2).mean(dim=(-1, -2)).sum(0)
        preds.append(pred.float())
        inpt = pp.append_history(inpt, pred, idt)
    return torch.stack(preds), space, time64


def check_scored(params, prob, device="cpu", held=(), model=None, capture=False, autocast=False, exact_curves=True):
    """Rollout against the hand-written loop on ``device``; returns the Rollout and the predictions."""
    from makani_amd.inference import Rollout
    steps, B = prob.tar.shape[1], prob.tar.shape[0]
    inp, tar = prob.inp.to(device), prob.tar.to(device)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        wrap, h0, loss = build(params, prob, device, model=model)
        want, space, time64 = handwritten(wrap, h0, loss, inp, tar, held)
        wrap, h1, loss = build(params, prob, device, model=model)
        ro = Rollout(params, wrap, metrics=h1, loss=loss, capture=capture)
        got = ro.run(inp, tar, output_channels=list(range(C)))
    assert got.shape == (steps, B, C) + tuple(tar.shape[-2:]) and got.dtype == torch.float32 and got.device.type == "cpu"
    assert torch.equal(got, want.cpu())
    assert not torch.equal(got[0], got[1])
    for name in ("acc_curve", "rmse_curve", "valid_buffer", "acc_counter"):
        a, b = getattr(h1, name), getattr(h0, name)
        if exact_curves:
            assert torch.equal(a, b), name
        else:
            # the handler's own pass and the rollout's sum in another order: 1e-6 of the value, for the ACC (a sum over the
            # samples of correlation coefficients, each at most 1, which may be near 0) 1e-6 of that range
            floor = float(B) if name == "acc_curve" else 0.0
            assert ((a - b).abs() <= 1e-6 * b.abs().clamp_min(floor)).all(), name
    assert float(h1.acc_counter.sum()) == steps and float(h1.valid_buffer[2]) == 1.0
    assert torch.equal(ro.RMSE_over_space, space)
    assert ((ro.RMSE_over_time - time64).abs() <= TIME_TOL * time64).all()
    curve, rmap = ro.finalize()
    assert curve.shape == (steps, C) and curve.dtype == torch.float32 and rmap.shape == space.shape
    assert ((curve.double() - (time64 / B).sqrt()).abs() <= TIME_TOL * (time64 / B).sqrt()).all()
    assert torch.equal(rmap, torch.sqrt(ro.RMSE_over_space / float(steps) / float(B)))
    return ro, got


CASES = [dict(history_normalization_mode="none"), dict(history_normalization_mode="none", masked_channels=[1]),
         dict(history_normalization_mode="exponential"), dict(history_normalization_mode="exponential", masked_channels=[1]),
         dict(history_normalization_mode="none", target="residual", masked_channels=[2])]


@pytest.mark.parametrize("nh", [0, 1])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_rollout_equals_the_handwritten_loop_bit_for_bit(tmp_path, nh, case):
    H, W, B, steps = 12, 24, 2, 3
    params = make_params(H, W, tmp_path, steps=steps, n_history=nh, **CASES[case])
    prob = make_problem(B, nh + 1, H, W, steps, seed=10 * case + nh)
    ro, _ = check_scored(params, prob)
    # stds scale both scores; zero_buffers starts over
    stds = torch.tensor([2.0, 0.5, 3.0])
    curve, rmap = ro.finalize()
    c2, m2 = ro.finalize(stds=stds)
    assert torch.equal(c2, curve * stds[None, :]) and torch.equal(m2, rmap * stds[:, None, None])
    ro.zero_buffers()
    assert float(ro.RMSE_over_time.abs().sum()) == 0.0 and float(ro.RMSE_over_space.abs().sum()) == 0.0 and ro.n_samples == 0


def test_scored_rollout_holds_channels_too(tmp_path):
    H, W, B, steps = 12, 24, 2, 3
    params = make_params(H, W, tmp_path, steps=steps, n_history=1, held_channels=[0])
    check_scored(params, make_problem(B, 2, H, W, steps, seed=77), held=(0,))


def test_lite_rollout_holds_channels_and_emits(tmp_path):
    from makani_amd.inference import Rollout
    H, W, B, steps, nh = 12, 24, 2, 3, 1
    params = make_params(H, W, tmp_path, steps=steps, n_history=nh, history_normalization_mode="exponential",
                         masked_channels=[2], held_channels=[1])
    prob = make_problem(B, nh + 1, H, W, steps, seed=5)

    def rollout(**kw):
        wrap, _, _ = build(params, prob)
        return Rollout(params, wrap).run(prob.inp, **kw)

    plain = rollout(output_channels=[0, 1, 2])
    assert plain.shape == (steps, B, C, H, W)                    # steps defaults to valid_autoreg_steps + 1
    for idt in range(steps):
        assert torch.equal(plain[idt, :, 1], prob.inp[:, -1, 1])
    assert not torch.equal(plain[0, :, 0], plain[1, :, 0])
    # without the held channel the forecast moves there as well
    free = make_params(H, W, tmp_path, steps=steps, n_history=nh, history_normalization_mode="exponential", masked_channels=[2])
    wrap, _, _ = build(free, prob)
    moving = Rollout(free, wrap).run(prob.inp, steps=2, output_channels=[1])
    assert moving.shape == (2, B, 1, H, W) and not torch.equal(moving[0, :, 0], prob.inp[:, -1, 1])
    # a repeated and a reordered channel, de-normalised inside the pass
    oc, means, stds = [2, 0, 2], np.array([1.5, -2.0, 0.25], np.float32), np.array([3.0, 0.5, 7.0], np.float32)
    got = rollout(output_channels=oc, output_stats=(means, stds))
    want = plain[:, :, oc] * torch.from_numpy(stds).reshape(1, 1, 3, 1, 1) + torch.from_numpy(means).reshape(1, 1, 3, 1, 1)
    assert torch.equal(got, want)
    assert rollout() is None
    with pytest.raises(ValueError, match="output_stats"):
        rollout(output_stats=(means, stds))
    with pytest.raises(ValueError, match="out of range"):
        rollout(output_channels=[3])
    with pytest.raises(ValueError, match="held_channels"):
        Rollout(make_params(H, W, tmp_path, held_channels=[3]), build(params, prob)[0])


def test_times_feed_the_zenith_channel(tmp_path):
    """inp_times / tar_times go through cache_unpredicted_times: the rollout equals one on the same fields cached by hand."""
    from makani_amd import zenith
    from makani_amd.inference import Rollout
    H, W, B, steps = 12, 24, 2, 3
    lat, lon = np.linspace(90, -90, H), np.linspace(0, 360, W, endpoint=False)
    params = make_params(H, W, tmp_path, steps=steps, lat=lat, lon=lon)
    prob = make_problem(B, 1, H, W, steps, seed=9)
    t0 = np.datetime64("2021-03-04T06:00")
    inp_times = np.array([[t0], [t0 + np.timedelta64(30, "D")]])
    tar_times = np.stack([inp_times[:, 0] + np.timedelta64(6 * (k + 1), "h") for k in range(steps)], axis=1)
    wrap, _, _ = build(params, prob)
    got = Rollout(params, wrap).run(prob.inp, steps=steps, inp_times=inp_times, tar_times=tar_times, output_channels=[0, 1, 2])
    wrap2, _, _ = build(params, prob)
    cosz = zenith.CosZenith.from_params(params)
    field = lambda t: cosz(torch.from_numpy(zenith.solar_ephemeris(t)))
    wrap2.preprocessor.cache_unpredicted_features(None, None, field(inp_times), field(tar_times))
    want = Rollout(params, wrap2).run(prob.inp, steps=steps, output_channels=[0, 1, 2])
    assert torch.equal(got, want)
    assert torch.equal(wrap.preprocessor.unpredicted_inp_eval, field(tar_times)[:, -1:])


def _tail_inputs(B=2, H=5, W=8):
    g = torch.Generator().manual_seed(1)
    return dict(yn=torch.randn(B, C, H, W, generator=g), x=torch.randn(B, C, H, W, generator=g),
                tar=torch.randn(B, C, H, W, generator=g), wrow=torch.rand(H, generator=g), mask=torch.rand(H, W, generator=g))


def test_rollout_tail_rejects_bad_arguments():
    from makani_amd import ops
    t = _tail_inputs()
    B, _, H, W = t["yn"].shape
    for kw, needle in ((dict(mean=torch.zeros(B, C)), "mean and std"), (dict(mean=torch.zeros(B, C), std=torch.ones(B, C + 1)), "mean and std"),
                       (dict(mask_chans=[1]), "mask"), (dict(mask_chans=[1], mask=t["mask"][:, :-1]), "mask"),
                       (dict(mask_chans=[3], mask=t["mask"]), "out of range"), (dict(mask_chans=[1, 1], mask=t["mask"]), "repeats"),
                       (dict(residual=True), "x_last"), (dict(hold_chans=[0], x_last=t["x"][:, :2]), r"x_last \(2, 3, 5, 8\), got \(2, 2, 5, 8\)"),
                       (dict(scale=torch.ones(C), x_last=t["x"]), "scale"), (dict(clim=torch.zeros(C, H, W)), "need a target"),
                       (dict(tar=t["tar"][:, :, :-1], wrow=t["wrow"]), r"target \(2, 3, 4, 8\)"), (dict(tar=t["tar"]), "wrow"),
                       (dict(tar=t["tar"], wrow=t["wrow"][:-1]), "4 weights for 5"),
                       (dict(tar=t["tar"], wrow=t["wrow"], clim=torch.zeros(C, H, W + 1)), "climatology"),
                       (dict(tar=t["tar"], wrow=t["wrow"], err_map=torch.zeros(C, H, W, dtype=torch.float64)), "err_map"),
                       (dict(emit_scale=torch.ones(2)), "emit_scale"), (dict(emit_chans=[0, 1], emit_shift=torch.ones(3)), "emit_shift"),
                       (dict(emit_chans=torch.tensor([0, 1])), "int32")):
        with pytest.raises(ValueError, match=needle):
            ops.rollout_tail(t["yn"], **kw)
    with pytest.raises(ValueError, match="must be"):
        ops.rollout_tail(t["yn"][0])


def test_rollout_tail_cpu_path_and_knob(monkeypatch):
    from makani_amd import ops
    t = _tail_inputs()
    err = torch.full((C,) + tuple(t["yn"].shape[-2:]), 0.5)
    pred, sums, emit = ops.rollout_tail(t["yn"], tar=t["tar"], wrow=t["wrow"], err_map=err, emit_chans=[2, 2])
    assert torch.equal(pred, t["yn"]) and pred.data_ptr() != t["yn"].data_ptr()
    assert sums.shape == (2, C, 6) and sums.dtype == torch.float64 and len(ops.ROLLOUT_SUMS) == 6
    assert torch.equal(sums[..., :5], ops.geo_metric_sums(pred, t["tar"], None, t["wrow"]))
    d = pred - t["tar"]
    assert torch.equal(sums[..., 5], d.double().square().sum((-2, -1)))
    assert torch.equal(err, (torch.full_like(err, 0.5) + d[0] * d[0]) + d[1] * d[1])
    assert torch.equal(emit, pred[:, [2, 2]])
    assert ops.rollout_tail(t["yn"])[1:] == (None, None)
    for mode in ("hip", "torch"):                               # CPU tensors take the torch formulation under either
        monkeypatch.setenv("MK_ROLLOUT", mode)
        assert torch.equal(ops.rollout_tail(t["yn"], x_last=t["x"], residual=True)[0], t["x"] + t["yn"])
    monkeypatch.setenv("MK_ROLLOUT", "fast")
    with pytest.raises(ValueError, match="MK_ROLLOUT"):
        ops.rollout_tail(t["yn"])


def test_matmul_parallel_raises(monkeypatch, tmp_path):
    from makani_amd import comm
    from makani_amd.inference import Rollout
    params = make_params(12, 24, tmp_path)
    wrap, _, _ = build(params, make_problem(1, 1, 12, 24, 3, seed=0))
    monkeypatch.setattr(comm, "get_size", lambda name: 2 if name == "matmul" else 1)
    with pytest.raises(NotImplementedError):
        Rollout(params, wrap)


# ---------------------------------------------------------------------------------------------------------------------
# misaligned pointers: refused by the host checks, with the message of the check (tests/capi_checks.py)
# ---------------------------------------------------------------------------------------------------------------------
_A = capi.A
MISALIGNED = [      # entry point, its arguments in front of the stream with one pointer moved off its alignment, the refusal
    ("mk_rollout_tail", (_A + 2, 0) + (None,) * 4 + (0, None, 0, 0, None, None, 0, _A) + (None,) * 10 + (0, 1, 2, 4, 8),
     "model output not aligned to its element"),
    ("mk_rollout_tail", (_A, 1) + (None,) * 4 + (0, None, 0, 0, None, None, 0, _A + 2) + (None,) * 10 + (0, 1, 2, 4, 8),
     "fp32 / int32 stream not 4-byte aligned"),
    ("mk_rollout_tail", (_A, 0) + (None,) * 4 + (0, None, 0, 0, None, None, 0, _A, _A, None, _A, _A + 4, _A) + (None,) * 5 + (0, 1, 2, 4, 8),
     "fp64 buffer not 8-byte aligned"),
]


@pytest.mark.parametrize("case", MISALIGNED, ids=capi.case_ids(MISALIGNED))
def test_misaligned_pointer_is_refused_before_any_launch(case):
    capi.assert_refused(*case)
