"""CPU tests of the validation metrics (makani_amd.metrics, makani_amd.metric.MetricsHandler, the CPU path of
ops.geo_metric_sums) against a float64 restatement of the reference's arithmetic (makani/utils/metrics/functions.py,
makani/utils/metric.py:186-306).  The restatement lives here; test_metrics_dist_cpu.py and test_metrics_gpu.py import it."""
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import capi_checks as capi

from oracle.losses import quad_weight

TOL = 1e-5
REDUCTIONS = ["mean", "sum", "none"]


# ------------------------------------------------------------------ float64 restatement of the reference
def reduce64(v, channel_reduction, batch_reduction):
    if channel_reduction == "mean":
        v = v.mean(axis=1)
    elif channel_reduction == "sum":
        v = v.sum(axis=1)
    if batch_reduction == "mean":
        v = v.mean(axis=0)
    elif batch_reduction == "sum":
        v = v.sum(axis=0)
    return v


def quad64(x, q):
    """GridQuadrature.forward: sum over the last two axes with the [H, W] weights."""
    return (np.asarray(x, np.float64) * q).sum(axis=(-2, -1))


def l1_64(x, y, q):
    return quad64(np.abs(np.asarray(x, np.float64) - np.asarray(y, np.float64)), q)


def msq_64(x, y, q):
    return quad64((np.asarray(x, np.float64) - np.asarray(y, np.float64)) ** 2, q)


def acc_64(x, y, q, eps=1e-8):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return quad64(x * y, q) / (np.sqrt(quad64(x * x, q) * quad64(y * y, q)) + eps)


def sums_64(p, t, c, wrow):
    """The five integrals of ops.geo_metric_sums, [B, C, 5]."""
    p, t = np.asarray(p, np.float64), np.asarray(t, np.float64)
    c = np.zeros(()) if c is None else np.asarray(c, np.float64)[None]
    w = np.asarray(wrow, np.float64)[None, None, :, None]
    d, pa, ta = p - t, p - c, t - c
    return np.stack([(w * np.abs(d)).sum((-2, -1)), (w * d * d).sum((-2, -1)), (w * pa * ta).sum((-2, -1)),
                     (w * pa * pa).sum((-2, -1)), (w * ta * ta).sum((-2, -1))], axis=-1)


def auc_weights64(n_intervals):
    """functions.py:110-167: Simpson 1/3 for an even number of intervals, else trapezoid; width 1 / (n + 1)."""
    h = 1.0 / (n_intervals + 1)
    if n_intervals % 2 == 0:
        w = np.ones(n_intervals + 1)
        w[1:-1:2] = 4.0
        w[2:-1:2] = 2.0
        return w * h / 3.0
    w = np.full(n_intervals + 1, h)
    w[0] = w[-1] = 0.5 * h
    return w


def handler64(batches, clim, q, mult, n_steps, eps=1e-8):
    """metric.py:186-306 in float64 over the full field: batches = [(preds[idt], tars[idt], losses[idt]) ...]."""
    C = clim.shape[0]
    acc = np.zeros((C, n_steps + 1))
    rmse = np.zeros((C, n_steps + 1))
    counter = np.zeros(n_steps + 1)
    loss = l1 = steps = 0.0
    for preds, tars, losses in batches:
        for idt, (p, t) in enumerate(zip(preds, tars)):
            acc[:, idt] += acc_64(np.asarray(p, np.float64) - clim, np.asarray(t, np.float64) - clim, q, eps).sum(axis=0)
            rmse[:, idt] += mult * np.sqrt(msq_64(p, t, q)).sum(axis=0)
            counter[idt] += 1
            if idt == 0:
                steps += 1
                loss += float(losses[idt])
                l1 += l1_64(p, t, q).mean(axis=1).sum(axis=0)
    acc, rmse = acc / counter, rmse / counter
    return dict(loss=loss / steps, l1=l1 / steps, acc=acc, rmse=rmse, auc=(acc * auc_weights64(n_steps)).sum(axis=1))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ------------------------------------------------------------------ fixtures of a small validation problem
CHANNELS = ["u10m", "t2m", "z500", "sst"]


def make_params(H, W, crop=None, offset=(0, 0), grid="equiangular", steps=2, split_data_channels=False):
    crop = crop or (H, W)
    return SimpleNamespace(log_to_screen=False, log_to_wandb=False, channel_names=list(CHANNELS), dt=1, dhours=6,
                           split_data_channels=split_data_channels, valid_autoreg_steps=steps, N_out_channels=len(CHANNELS),
                           img_shape_x=H, img_shape_y=W, img_crop_shape_x=crop[0], img_crop_shape_y=crop[1],
                           img_crop_offset_x=offset[0], img_crop_offset_y=offset[1], model_grid_type=grid)


def make_rollout(B, C, H, W, steps, seed, n_batches=1, dtype=torch.float32):
    """Correlated prediction / target pairs (the ACC is well away from 0), a climatology and the output scale."""
    g = torch.Generator().manual_seed(seed)
    clim = 0.5 * torch.randn(C, H, W, generator=g)
    mult = 1.0 + torch.rand(C, generator=g)
    batches = []
    for _ in range(n_batches):
        preds, tars, losses = [], [], []
        for _ in range(steps + 1):
            t = clim + torch.randn(B, C, H, W, generator=g)
            p = 0.8 * t + 0.4 * torch.randn(B, C, H, W, generator=g) + 0.1
            preds.append(p.to(dtype))
            tars.append(t)
            losses.append(torch.rand((), generator=g))
        batches.append((preds, tars, losses))
    return clim, mult, batches


def run_handler(params, mult, clim, batches, device="cpu", shard=None):
    """Drive MetricsHandler like Trainer.validate_one_epoch; shard(x) cuts this rank's piece of a full field."""
    from makani_amd.metric import MetricsHandler
    shard = shard or (lambda x: x)
    h = MetricsHandler(params, mult, clim, torch.device(device))
    h.initialize_buffers()
    h.zero_buffers()
    with torch.inference_mode():
        for preds, tars, losses in batches:
            for idt, (p, t) in enumerate(zip(preds, tars)):
                h.update(shard(p).to(device), shard(t).to(device), losses[idt].to(device), idt)
        logs, acc, rmse = h.finalize(final_inference=True)
    return h, logs, acc, rmse


def check_handler(params, mult, clim, batches, logs, acc, rmse, tol=TOL):
    H, W = params.img_shape_x, params.img_shape_y
    crop = (params.img_crop_shape_x, params.img_crop_shape_y)
    off = (params.img_crop_offset_x, params.img_crop_offset_y)
    rule = "legendre-gauss" if params.model_grid_type == "legendre_gauss" else "naive"
    q = quad_weight(rule, (H, W), crop, off, normalize=True)
    full = [([p.double().numpy() for p in ps], [t.double().numpy() for t in ts], ls) for ps, ts, ls in batches]
    want = handler64(full, clim.double().numpy(), q, mult.double().numpy(), params.valid_autoreg_steps)
    assert rel(acc.cpu(), want["acc"]) < tol
    assert rel(rmse.cpu(), want["rmse"]) < tol
    assert abs(logs["base"]["validation loss"] - want["loss"]) < tol * abs(want["loss"])
    assert abs(logs["base"]["validation L1"] - want["l1"]) < tol * abs(want["l1"])
    for name in ("u10m", "t2m", "z500"):
        c = CHANNELS.index(name)
        assert abs(logs["metrics"]["validation " + name] - want["rmse"][c, 0]) < tol * want["rmse"][c, 0]
        assert abs(logs["metrics"]["ACC AUC " + name] - want["auc"][c]) < tol * abs(want["auc"][c])
    return want


# ------------------------------------------------------------------ metric classes
@pytest.mark.parametrize("channel_reduction", REDUCTIONS)
@pytest.mark.parametrize("batch_reduction", REDUCTIONS)
@pytest.mark.parametrize("grid,img,crop,offset", [("naive", (33, 48), (30, 40), (2, 5)),
                                                  ("legendre-gauss", (32, 64), (31, 64), (1, 0))])
def test_metric_classes_match_float64(channel_reduction, batch_reduction, grid, img, crop, offset):
    from makani_amd.metrics import GeometricACC, GeometricL1, GeometricRMSE
    g = torch.Generator().manual_seed(5)
    y = torch.randn(3, 4, *crop, generator=g)
    x = 0.7 * y + 0.5 * torch.randn(3, 4, *crop, generator=g)
    q = quad_weight(grid, img, crop, offset, normalize=True)
    kw = dict(img_shape=img, crop_shape=crop, crop_offset=offset, normalize=True, channel_reduction=channel_reduction,
              batch_reduction=batch_reduction)
    xd, yd = x.double().numpy(), y.double().numpy()
    cases = [(GeometricL1(grid, **kw), reduce64(l1_64(xd, yd, q), channel_reduction, batch_reduction)),
             (GeometricRMSE(grid, **kw), np.sqrt(reduce64(msq_64(xd, yd, q), channel_reduction, batch_reduction))),
             (GeometricACC(grid, **kw), reduce64(acc_64(xd, yd, q), channel_reduction, batch_reduction))]
    for metric, want in cases:
        got = metric(x, y)
        assert got.dtype == metric.quadrature.quad_weight.dtype and tuple(got.shape) == np.shape(want)
        assert rel(got, want) < 1e-6, type(metric).__name__


def test_metric_classes_stay_differentiable():
    from makani_amd.metrics import GeometricRMSE
    x = torch.randn(2, 3, 17, 24, requires_grad=True)
    y = torch.randn(2, 3, 17, 24)
    GeometricRMSE("naive", (17, 24), normalize=True)(x, y).backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()


def test_geo_metric_sums_cpu_path():
    from makani_amd import ops
    g = torch.Generator().manual_seed(2)
    p, t, c = torch.randn(2, 3, 9, 13, generator=g), torch.randn(2, 3, 9, 13, generator=g), torch.randn(3, 9, 13, generator=g)
    w = torch.rand(9, generator=g)
    for clim in (c, None):
        got = ops.geo_metric_sums(p, t, clim, w)
        assert got.dtype == torch.float64 and got.shape == (2, 3, 5)
        assert rel(got, sums_64(p.numpy(), t.numpy(), None if clim is None else clim.numpy(), w.numpy())) < 1e-12
    with pytest.raises(ValueError):
        ops.geo_metric_sums(p, t, c, torch.rand(8))


# ------------------------------------------------------------------ rollout quadratures
def test_simpson_weights_by_hand():
    from makani_amd.metrics import Quadrature, SimpsonQuadrature
    s = SimpsonQuadrature(4, 0.3, "cpu")
    assert torch.allclose(s.weights, torch.tensor([1, 4, 2, 4, 1], dtype=torch.float32) * 0.1)
    assert torch.allclose(SimpsonQuadrature(2, 1.0 / 3.0, "cpu").weights, torch.tensor([1.0, 4.0, 1.0]) / 9.0)
    q = Quadrature(4, 0.3, "cpu")
    x = torch.arange(10, dtype=torch.float32).reshape(2, 5)
    assert torch.allclose(q(x, dim=1), torch.tensor([0.1 * (0 + 4 + 4 + 12 + 4), 0.1 * (5 + 24 + 14 + 32 + 9)]))
    with pytest.raises(NotImplementedError):
        SimpsonQuadrature(3, 0.25, "cpu")


def test_trapezoid_weights_by_hand():
    from makani_amd.metrics import Quadrature, TrapezoidQuadrature
    assert torch.allclose(TrapezoidQuadrature(3, 0.25, "cpu").weights, torch.tensor([0.125, 0.25, 0.25, 0.125]))
    assert torch.allclose(TrapezoidQuadrature(4, 0.2, "cpu").weights, torch.tensor([0.1, 0.2, 0.2, 0.2, 0.1]))
    q = Quadrature(3, 0.25, "cpu")
    assert isinstance(q.quad, TrapezoidQuadrature)
    assert torch.allclose(q(torch.tensor([[1.0, 2.0, 3.0, 4.0]]), dim=1), torch.tensor([0.125 + 0.5 + 0.75 + 0.5]))
    for n in (1, 2, 3, 6, 7):
        w = (Quadrature(n, 1.0 / (n + 1), "cpu").quad.weights).double().numpy()
        assert np.abs(w - auc_weights64(n)).max() < 1e-7


# ------------------------------------------------------------------ MetricsHandler
@pytest.mark.parametrize("grid,crop,offset,steps", [("equiangular", None, (0, 0), 2), ("legendre_gauss", (20, 28), (3, 2), 2),
                                                    ("equiangular", (21, 30), (1, 0), 3)])
def test_metrics_handler_matches_float64(grid, crop, offset, steps):
    H, W = 24, 32
    params = make_params(H, W, crop, offset, grid, steps)
    Hc, Wc = crop or (H, W)
    clim, mult, batches = make_rollout(2, len(CHANNELS), Hc, Wc, steps, seed=17, n_batches=2)
    h, logs, acc, rmse = run_handler(params, mult, clim, batches)
    check_handler(params, mult, clim, batches, logs, acc, rmse)
    assert logs["base"]["validation steps"] == 2
    assert acc.shape == rmse.shape == (len(CHANNELS), steps + 1) and acc.dtype == torch.float32
    assert set(logs["metrics"]) == {"validation u10m", "validation t2m", "validation z500", "ACC AUC u10m", "ACC AUC t2m",
                                    "ACC AUC z500", "rollouts"}


def test_rollouts_without_wandb(monkeypatch):
    monkeypatch.setitem(sys.modules, "wandb", None)           # `import wandb` raises ImportError
    params = make_params(16, 24, steps=2)
    clim, mult, batches = make_rollout(1, len(CHANNELS), 16, 24, 2, seed=3)
    h, logs, acc, rmse = run_handler(params, mult, clim, batches)
    table = logs["metrics"]["rollouts"]
    assert table["columns"] == ["metric type", "variable name", "time [h]", "value"]
    assert len(table["data"]) == 2 * 3 * 3                     # (ACC, RMSE) x 3 variables x 3 lead times
    first = table["data"][0]
    assert first[:3] == ["ACC", "u10m", 6] and abs(first[3] - float(acc[0, 0])) < 1e-7
    rm = [r for r in table["data"] if r[0] == "RMSE" and r[1] == "z500"]
    assert [r[2] for r in rm] == [6, 12, 18]
    assert abs(rm[2][3] - float(rmse[CHANNELS.index("z500"), 2])) < 1e-6 * float(rmse[CHANNELS.index("z500"), 2])


def test_matmul_parallel_raises(monkeypatch):
    from makani_amd import comm
    from makani_amd.metric import MetricsHandler
    real = comm.get_size
    monkeypatch.setattr(comm, "get_size", lambda name: 2 if name == "matmul" else real(name))
    params = make_params(16, 24, split_data_channels=True)
    with pytest.raises(NotImplementedError):
        MetricsHandler(params, torch.ones(len(CHANNELS)), torch.zeros(len(CHANNELS), 16, 24), torch.device("cpu"))
    MetricsHandler(make_params(16, 24), torch.ones(len(CHANNELS)), torch.zeros(len(CHANNELS), 16, 24), torch.device("cpu"))


# ---------------------------------------------------------------------------------------------------------------------
# misaligned pointers: refused by the host checks, with the message of the check (tests/capi_checks.py)
# ---------------------------------------------------------------------------------------------------------------------
_A = capi.A
MISALIGNED = [      # entry point, its arguments in front of the stream with one pointer moved off its alignment, the refusal
    ("mk_geo_metric_sums", (_A + 2, 0, _A, None, _A, _A, _A, 1, 2, 4, 8), "prediction not aligned to its element"),
    ("mk_geo_metric_sums", (_A + 1, 1, _A, None, _A, _A, _A, 1, 2, 4, 8), "prediction not aligned to its element"),
    ("mk_geo_metric_sums", (_A, 0, _A + 2, None, _A, _A, _A, 1, 2, 4, 8), "fp32 stream not 4-byte aligned"),
    ("mk_geo_metric_sums", (_A, 1, _A, _A + 2, _A, _A, _A, 1, 2, 4, 8), "fp32 stream not 4-byte aligned"),
]


@pytest.mark.parametrize("case", MISALIGNED, ids=capi.case_ids(MISALIGNED))
def test_misaligned_pointer_is_refused_before_any_launch(case):
    capi.assert_refused(*case)
