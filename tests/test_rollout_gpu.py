"""GPU tests of the rollout tail (csrc/rollout.hip through the C ABI and ops.rollout_tail) and of Rollout on the device.

The kernel's field arithmetic is one fp32 rounding per operation, as torch's one-kernel-per-operation formulation
(``ops._rollout_tail_torch``) on the same device tensors: ``pred``, the error map and the emitted fields must be equal
bit for bit, outputs between guard bands, inputs between NaN bands.  The sums are fp32 row partials folded in fp64: held
to the measure and bound of test_metrics_gpu.py, ``max |got - want| / |want| < 1e-6`` over all ``[B, C, 6]`` against torch
float64 of the written ``pred``; the inputs are that file's ``_fields`` (prediction correlated with the target, so the one
signed sum does not cancel), and the extra streams keep that correlation: the last input step is ``0.5 tar + noise``, the
statistics, the mask and the residual scale stay near (1, 0), 1 and 1."""
import pytest
import torch

from kernel_checks import SENTINEL, guarded, poisoned
from test_metrics_gpu import _fields, _rel_each, _sums64
from test_rollout_cpu import C as CR, check_scored, make_params, make_problem
from test_stepper_gpu import _sfno

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3, 7, 60), (2, 3, 7, 61), (3, 3, 9, 61), (1, 2, 5, 1440)]
OPTIONS = ["denorm", "all", "all_repeat", "no_clim", "no_map", "no_target"]


def _inputs(dev, shape, dtype, seed):
    """Everything a launch can read, as plain device tensors (fp32 unless said)."""
    B, C, H, W = shape
    yn, tar, clim, wrow = _fields(dev, B, C, H, W, dtype=dtype, seed=seed)
    g = torch.Generator(device=dev).manual_seed(1000 + seed)
    r = lambda *s: torch.rand(*s, device=dev, generator=g)
    return dict(yn=yn, tar=tar, clim=clim, wrow=wrow, mean=0.1 * r(B, C) - 0.05, std=0.9 + 0.2 * r(B, C), mask=0.9 + 0.1 * r(H, W),
                x_last=0.5 * tar + 0.1 * torch.randn(B, C, H, W, device=dev, generator=g), scale=0.9 + 0.2 * r(C),
                err0=r(C, H, W) + 0.5, escale=1.0 + r(2), eshift=r(2) - 0.5)


def _option(t, opt, C, dev):
    """The arguments of ``ops._rollout_tail_torch`` (in its order) for an option set."""
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    none = dict(yn=t["yn"], mean=None, std=None, mask=None, mask_chans=None, x_last=None, residual=False, scale=None, hold_chans=None,
                tar=None, clim=None, wrow=None, err_map=None, emit_chans=None, emit_scale=None, emit_shift=None)
    score = dict(tar=t["tar"], wrow=t["wrow"])
    if opt == "denorm":
        return dict(none, mean=t["mean"], std=t["std"])
    if opt in ("all", "all_repeat"):
        chans = [C - 1, 0] if opt == "all" else [C - 1, C - 1]
        return dict(none, mean=t["mean"], std=t["std"], mask=t["mask"], mask_chans=i32([1]), x_last=t["x_last"], residual=True,
                    scale=t["scale"], hold_chans=i32([0]), clim=t["clim"], err_map=t["err0"], emit_chans=i32(chans),
                    emit_scale=t["escale"], emit_shift=t["eshift"], **score)
    if opt == "no_clim":
        return dict(none, mean=t["mean"], std=t["std"], err_map=t["err0"], **score)
    if opt == "no_map":
        return dict(none, clim=t["clim"], x_last=t["x_last"], hold_chans=i32([C - 1]), **score)
    assert opt == "no_target"
    return dict(none, mask=t["mask"], mask_chans=i32([0]), x_last=t["x_last"], residual=True, emit_chans=i32([0, C - 1]))


def _shifted_in(t, off):
    """A bit-equal copy of ``t`` between NaN bands, its first element ``off`` elements past a 16-byte boundary."""
    if t is None:
        return None
    if off == 0 or not t.is_floating_point():
        return poisoned(t) if t.is_floating_point() else t
    flat = torch.cat([torch.full((off,), float("nan"), dtype=t.dtype, device=t.device), t.reshape(-1)])
    return poisoned(flat)[off:].view(t.shape)


def _guarded_out(shape, dev, off):
    """(view, check): an fp32 output between guard bands, ``off`` elements past a 16-byte boundary; the check covers the
    bands and the ``off`` elements in front."""
    n = 1
    for s in shape:
        n *= s
    flat, check = guarded((n + off,), torch.float32, dev)

    def check_all(what=""):
        check(what)
        assert bool((flat[:off] == SENTINEL).all()), f"{what}: the elements in front of the output were written"

    return flat[off:].view(shape), check_all


def _launch(lib, dev, shape, a, off=0):
    """One launch through the C ABI on banded copies of the arguments ``a``; returns (pred, sums, err_map, emit)."""
    B, C, H, W = shape
    p = lambda x: x.data_ptr() if x is not None else None
    f = {k: _shifted_in(a[k], off) for k in ("yn", "mean", "std", "mask", "x_last", "scale", "tar", "clim", "wrow", "emit_scale", "emit_shift")}
    pred, check_pred = _guarded_out(shape, dev, off)
    err = check_err = emit = check_emit = ws = sums = None
    if a["err_map"] is not None:
        err, check_err = _guarded_out((C, H, W), dev, off)
        err.copy_(a["err_map"])
    K = a["emit_chans"].numel() if a["emit_chans"] is not None else 0
    if K:
        emit, check_emit = _guarded_out((B, K, H, W), dev, off)
    if a["tar"] is not None:
        ws = torch.empty(lib.mk_rollout_tail_workspace(B, C, H), dtype=torch.float64, device=dev)
        sums = torch.full((B, C, 6), -1.0, dtype=torch.float64, device=dev)
    bstride = f["x_last"].stride(0) if f["x_last"] is not None else 0
    rc = lib.mk_rollout_tail(p(f["yn"]), 0 if f["yn"].dtype == torch.float32 else 1, p(f["mean"]), p(f["std"]), p(f["mask"]),
                             p(a["mask_chans"]), a["mask_chans"].numel() if a["mask_chans"] is not None else 0, p(f["x_last"]),
                             bstride, int(a["residual"]), p(f["scale"]), p(a["hold_chans"]),
                             a["hold_chans"].numel() if a["hold_chans"] is not None else 0, p(pred), p(f["tar"]), p(f["clim"]),
                             p(f["wrow"]), p(ws), p(sums), p(err), p(emit), p(a["emit_chans"]), p(f["emit_scale"]),
                             p(f["emit_shift"]), K, B, C, H, W, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mk_last_error()
    torch.cuda.synchronize()
    for chk, name in ((check_pred, "pred"), (check_err, "err_map"), (check_emit, "emit")):
        if chk is not None:
            chk(name)
    return pred, sums, err, emit


def _reference(a):
    """``ops._rollout_tail_torch`` on the plain tensors, the map on a copy of its start."""
    from makani_amd import ops
    err = a["err_map"].clone() if a["err_map"] is not None else None
    a = dict(a, err_map=err)
    pred, sums, emit = ops._rollout_tail_torch(**a)
    return pred, sums, err, emit


def _want_sums(pred, a):
    """torch float64 of the written pred: the five sums of test_metrics_gpu.py and the unweighted sum of fp32 d squared."""
    d = pred - a["tar"]
    return torch.cat([_sums64(pred, a["tar"], a["clim"], a["wrow"]), d.double().square().sum((-2, -1)).unsqueeze(-1)], dim=-1)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_equals_the_torch_formulation(dev, shape, dtype, off):
    from makani_amd import _lib
    lib = _lib.load()
    B, C, H, W = shape
    t = _inputs(dev, shape, dtype, seed=W + B)
    for opt in OPTIONS:
        a = _option(t, opt, C, dev)
        pred, sums, err, emit = _launch(lib, dev, shape, a, off)
        rpred, rsums, rerr, remit = _reference(a)
        what = (shape, dtype, off, opt)
        assert torch.equal(pred, rpred), what
        assert bool(torch.isfinite(pred).all()), what
        assert not torch.equal(pred, t["yn"].float()), what
        assert (err is None) == (rerr is None) and (emit is None) == (remit is None) and (sums is None) == (rsums is None), what
        if err is not None:
            assert torch.equal(err, rerr) and not torch.equal(err, t["err0"]), what
        if emit is not None:
            assert torch.equal(emit, remit), what
        if sums is not None:
            want = _want_sums(pred, a)
            e = _rel_each(sums, want)
            print(f"{what}: sums rel err {e:.2e} (kernel), {_rel_each(rsums, want):.2e} (torch formulation); bound 1e-6")
            assert e < 1e-6, what
            # the same bits every run
            again = _launch(lib, dev, shape, a, off)
            assert torch.equal(again[1], sums) and torch.equal(again[0], pred), what
    # the everything-on set does what it says: channel 0 is held, channel 1 masked
    a = _option(t, "all", C, dev)
    pred = _launch(lib, dev, shape, a, off)[0]
    assert torch.equal(pred[:, 0], t["x_last"][:, 0])
    a2 = dict(a, mask_chans=None, mask=None)
    pred2 = _launch(lib, dev, shape, a2, off)[0]
    assert not torch.equal(pred2[:, 1], pred[:, 1]) and torch.equal(pred2[:, C - 1:], pred[:, C - 1:]) == (C > 2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", SHAPES)
def test_row_slices_give_the_slices(dev, shape, dtype):
    from makani_amd import _lib
    lib = _lib.load()
    B, C, H, W = shape
    t = _inputs(dev, shape, dtype, seed=3 * W + B)
    a = _option(t, "all", C, dev)
    pred, sums, err, emit = _launch(lib, dev, shape, a)
    total = torch.zeros_like(sums)
    for h0, h1 in ((0, 3), (3, H)):
        cut = lambda x: x[..., h0:h1, :].contiguous()
        s = dict(a, yn=cut(a["yn"]), mask=cut(a["mask"]), x_last=cut(a["x_last"]), tar=cut(a["tar"]), clim=cut(a["clim"]),
                 wrow=a["wrow"][h0:h1].contiguous(), err_map=cut(a["err_map"]))
        sp, ss, se, sm = _launch(lib, dev, (B, C, h1 - h0, W), s)
        assert torch.equal(sp, pred[..., h0:h1, :]) and torch.equal(se, err[..., h0:h1, :]) and torch.equal(sm, emit[..., h0:h1, :])
        total += ss
    # the sums add up as in test_metrics_gpu.py's test_shard_sums_add_up: a row of a slice starts at another address, its fp32
    # partials are summed by other lanes
    assert _rel_each(total, sums) < 1e-6


def test_ops_rollout_tail_on_the_device(dev, monkeypatch):
    """The operator: HIP against the torch formulation under the knob, the last history step read in place."""
    from makani_amd import ops
    B, C, H, W, T = 2, 3, 7, 61, 2
    t = _inputs(dev, (B, C, H, W), torch.bfloat16, seed=5)
    hist = torch.randn(B, T * C, H, W, device=dev)
    hist.view(B, T, C, H, W)[:, -1] = t["x_last"]
    x_last = hist.view(B, T, C, H, W)[:, -1]
    assert not x_last.is_contiguous()
    out = {}
    for mode in ("hip", "torch"):
        monkeypatch.setenv("MK_ROLLOUT", mode)
        err = t["err0"].clone()
        out[mode] = ops.rollout_tail(t["yn"], mean=t["mean"].view(B, C, 1, 1), std=t["std"].view(B, C, 1, 1), mask=t["mask"],
                                     mask_chans=[1], x_last=x_last, residual=True, scale=t["scale"].view(1, C, 1, 1),
                                     hold_chans=[0], tar=t["tar"], clim=t["clim"], wrow=t["wrow"], err_map=err,
                                     emit_chans=[2, 0, 2], emit_scale=torch.ones(3, device=dev) * 2, emit_shift=None) + (err,)
    for a, b in zip(out["hip"], out["torch"]):
        if a.dtype == torch.float64:
            assert _rel_each(a, b) < 1e-6
        else:
            assert torch.equal(a, b)
    assert out["hip"][0].dtype == torch.float32 and out["hip"][2].shape == (B, 3, H, W)


def test_c_abi_rejects_bad_arguments(dev):
    from makani_amd import _lib
    lib = _lib.load()
    shape = (1, 2, 4, 8)
    B, C, H, W = shape
    t = _inputs(dev, shape, torch.float32, seed=1)
    pred = torch.full(shape, 3.0, device=dev)
    ws = torch.zeros(lib.mk_rollout_tail_workspace(B, C, H), dtype=torch.float64, device=dev)
    sums = torch.full((B, C, 6), -1.0, dtype=torch.float64, device=dev)
    one = torch.tensor([1], dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    base = dict(yn=t["yn"].data_ptr(), dtype=0, mean=None, std=None, mask=None, mask_chans=None, n_mask=0, x_last=None, bstride=0,
                residual=0, scale=None, hold=None, n_hold=0, pred=pred.data_ptr(), tar=None, clim=None, wrow=None, ws=None, sums=None,
                err=None, emit=None, echans=None, escale=None, eshift=None, K=0, B=B, C=C, H=H, W=W)

    def call(**kw):
        return lib.mk_rollout_tail(*dict(base, **kw).values(), st)

    for kw, needle in ((dict(yn=None), b"null pointer"), (dict(pred=None), b"null pointer"), (dict(dtype=2), b"dtype"),
                       (dict(mean=t["mean"].data_ptr()), b"mean and std"), (dict(n_mask=1, mask_chans=one.data_ptr()), b"masked channels"),
                       (dict(n_mask=-1), b"masked channels"), (dict(n_hold=1, hold=one.data_ptr()), b"x_last"),
                       (dict(residual=1), b"x_last"), (dict(residual=2), b"residual"),
                       (dict(residual=1, x_last=t["x_last"].data_ptr(), bstride=1), b"batch stride"),
                       (dict(scale=t["scale"].data_ptr()), b"scale without"), (dict(clim=t["clim"].data_ptr()), b"need a target"),
                       (dict(tar=t["tar"].data_ptr()), b"a target needs"), (dict(K=1), b"emitted channels"),
                       (dict(escale=t["escale"].data_ptr()), b"without emitted"), (dict(K=2000), b"emitted channels"),
                       (dict(W=0), b"bad sizes"), (dict(yn=t["yn"].data_ptr() + 2), b"aligned")):
        assert call(**kw) != 0, kw
        assert needle in lib.mk_last_error(), (needle, lib.mk_last_error())
    assert lib.mk_rollout_tail_workspace(0, C, H) == 0
    torch.cuda.synchronize()
    assert bool((pred == 3.0).all()) and bool((sums == -1.0).all())          # nothing was launched
    assert call() == 0 and call(tar=t["tar"].data_ptr(), wrow=t["wrow"].data_ptr(), ws=ws.data_ptr(), sums=sums.data_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(pred, t["yn"]) and bool((sums[..., 1] > 0).all())


# ---------------------------------------------------------------------------- Rollout on the device
def test_captured_rollout_equals_eager_bitwise(dev, tmp_path, monkeypatch):
    """capture=True with the toy model: three steps bit-equal to the eager run.  The tail is part of the graph: the library
    entry point is called while the step is captured and never again while the graph is replayed.  (``_graph_names`` of
    test_lploss_gpu.py walks autograd nodes; a rollout runs under ``no_grad`` and has none, so the launches are counted.)"""
    from makani_amd import _lib
    monkeypatch.setenv("MK_ROLLOUT", "hip")
    H, W, B, steps = 12, 24, 2, 3
    params = make_params(H, W, tmp_path, steps=steps, n_history=1, masked_channels=[1], held_channels=[2])
    prob = make_problem(B, 2, H, W, steps, seed=12)
    eager, want = check_scored(params, prob, dev, held=(2,), exact_curves=False)
    lib = _lib.load()
    calls = []
    real = lib.mk_rollout_tail

    class Counted:
        def __getattr__(self, name):
            if name == "mk_rollout_tail":
                return lambda *a: calls.append(torch.cuda.is_current_stream_capturing()) or real(*a)
            return getattr(lib, name)

    monkeypatch.setattr(_lib, "load", lambda: Counted())
    captured, got = check_scored(params, prob, dev, held=(2,), capture=True, exact_curves=False)
    assert calls == [False, True], calls            # the warm-up step and the capture; three replays launch from the graph
    assert torch.equal(got, want)
    assert torch.equal(captured.RMSE_over_space, eager.RMSE_over_space)
    assert torch.equal(captured.RMSE_over_time, eager.RMSE_over_time)
    for name in ("acc_curve", "rmse_curve", "valid_buffer"):
        assert torch.equal(getattr(captured.metrics, name), getattr(eager.metrics, name)), name


def test_rollout_of_the_package_sfno(dev, tmp_path, monkeypatch):
    """Two steps of a small package SFNO under bf16 autocast against the hand-written loop on the same device."""
    monkeypatch.setenv("MK_ROLLOUT", "hip")
    H, W, B, steps, T = 64, 128, 2, 2, 2
    params = make_params(H, W, tmp_path, steps=steps, n_history=T - 1, masked_channels=[1])
    prob = make_problem(B, T, H, W, steps, seed=4)
    check_scored(params, prob, dev, model=_sfno(dev, T * (CR + 1) + 3, CR, H, W), autocast=True, exact_curves=False)
