"""Validation metrics on the sphere: ``makani/utils/metrics/functions.py`` (``GeometricL1``, ``GeometricRMSE``,
``GeometricACC`` and the rollout quadratures ``SimpsonQuadrature``, ``TrapezoidQuadrature``, ``Quadrature``) with the
same constructor arguments, defaults and ``forward`` results.

The three field metrics are ratios or roots of latitude-weighted integrals per (sample, channel).  On CUDA tensors with
nothing to differentiate they come from one streaming HIP pass (``ops.geo_metric_sums``), followed by the reductions on
``[B, C]``; otherwise (CPU tensors, or inputs that need a gradient) they run the reference's torch formulation, so the
results stay differentiable.  The quadrature weights are those of ``losses.GridQuadrature`` (grids.py:63-115); they
depend on the latitude only, so the kernel reads one weight per row.
"""
import torch

from . import ops
from .losses import GridQuadrature


def _reduce(v, channel_reduction, batch_reduction):
    if channel_reduction == "mean":
        v = torch.mean(v, dim=1)
    elif channel_reduction == "sum":
        v = torch.sum(v, dim=1)
    if batch_reduction == "mean":
        v = torch.mean(v, dim=0)
    elif batch_reduction == "sum":
        v = torch.sum(v, dim=0)
    return v


class _GeometricMetric(torch.nn.Module):
    def __init__(self, grid_type, img_shape, crop_shape=None, crop_offset=(0, 0), normalize=False, channel_reduction="mean",
                 batch_reduction="mean"):
        super().__init__()
        self.quadrature = GridQuadrature(grid_type, img_shape=img_shape, crop_shape=crop_shape, crop_offset=crop_offset,
                                         normalize=normalize)
        self.channel_reduction = channel_reduction
        self.batch_reduction = batch_reduction

    def _use_kernel(self, x, y):
        need_grad = torch.is_grad_enabled() and (x.requires_grad or y.requires_grad)
        return x.is_cuda and y.is_cuda and x.dim() == 4 and not need_grad

    def _sums(self, x, y):
        return ops.geo_metric_sums(x, y, None, self.quadrature.row_weights)

    def _out_dtype(self, x, y):
        return torch.promote_types(torch.promote_types(x.dtype, y.dtype), self.quadrature.quad_weight.dtype)


class GeometricL1(_GeometricMetric):
    """functions.py:20-45: quadrature of |x - y| per (sample, channel), then the reductions."""

    def forward(self, x, y):
        if self._use_kernel(x, y):
            diff = self._sums(x, y)[..., 0]
            return _reduce(diff, self.channel_reduction, self.batch_reduction).to(self._out_dtype(x, y))
        diff = self.quadrature(torch.abs(x - y))
        return _reduce(diff, self.channel_reduction, self.batch_reduction)


class GeometricRMSE(_GeometricMetric):
    """functions.py:48-76: the square root of the reduced quadrature of (x - y)^2."""

    def forward(self, x, y):
        if self._use_kernel(x, y):
            diff = self._sums(x, y)[..., 1]
            return torch.sqrt(_reduce(diff, self.channel_reduction, self.batch_reduction)).to(self._out_dtype(x, y))
        diff = self.quadrature(torch.square(x - y))
        return torch.sqrt(_reduce(diff, self.channel_reduction, self.batch_reduction))


class GeometricACC(_GeometricMetric):
    """functions.py:79-107: cov(x, y) / (sqrt(var(x) var(y)) + eps) per (sample, channel), then the reductions.  x and y
    are the anomalies (the caller subtracts the climatology)."""

    def __init__(self, grid_type, img_shape, crop_shape=None, crop_offset=(0, 0), normalize=False, channel_reduction="mean",
                 batch_reduction="mean", eps=1e-8):
        super().__init__(grid_type, img_shape, crop_shape=crop_shape, crop_offset=crop_offset, normalize=normalize,
                         channel_reduction=channel_reduction, batch_reduction=batch_reduction)
        self.eps = eps

    def forward(self, x, y):
        if self._use_kernel(x, y):
            s = self._sums(x, y)
            acc = s[..., 2] / (torch.sqrt(s[..., 3] * s[..., 4]) + self.eps)
            return _reduce(acc, self.channel_reduction, self.batch_reduction).to(self._out_dtype(x, y))
        cov_xy = self.quadrature(x * y)
        var_x = self.quadrature(torch.square(x))
        var_y = self.quadrature(torch.square(y))
        acc = cov_xy / (torch.sqrt(var_x * var_y) + self.eps)
        return _reduce(acc, self.channel_reduction, self.batch_reduction)


class SimpsonQuadrature(torch.nn.Module):
    """functions.py:110-136: composite Simpson 1/3 weights over an even number of intervals."""

    def __init__(self, num_intervals, interval_width, device):
        super().__init__()
        if num_intervals % 2 != 0:
            raise NotImplementedError("Error, please specify an even number of intervals")
        weights = [0.0 for _ in range(num_intervals + 1)]
        for j in range(1, num_intervals // 2 + 1):
            weights[2 * j - 2] += 1.0
            weights[2 * j - 1] += 4.0
            weights[2 * j] += 1.0
        self.weights = torch.tensor(weights, dtype=torch.float32, device=device)
        self.weights *= interval_width / 3.0

    def forward(self, x, dim=1):
        shape = [1 for _ in range(x.dim())]
        shape[dim] = -1
        return torch.sum(x * torch.reshape(self.weights, shape), dim=dim)


class TrapezoidQuadrature(torch.nn.Module):
    """functions.py:139-155: trapezoid weights."""

    def __init__(self, num_intervals, interval_width, device):
        super().__init__()
        weights = [interval_width for _ in range(num_intervals + 1)]
        weights[0] *= 0.5
        weights[-1] *= 0.5
        self.weights = torch.tensor(weights, dtype=torch.float32, device=device)

    def forward(self, x, dim=1):
        shape = [1 for _ in range(x.dim())]
        shape[dim] = -1
        return torch.sum(x * torch.reshape(self.weights, shape), dim=dim)


class Quadrature(torch.nn.Module):
    """functions.py:158-167: Simpson's rule for an even number of intervals, the trapezoid rule for an odd one."""

    def __init__(self, num_intervals, interval_width, device):
        super().__init__()
        if num_intervals % 2 == 0:
            self.quad = SimpsonQuadrature(num_intervals, interval_width, device)
        else:
            self.quad = TrapezoidQuadrature(num_intervals, interval_width, device)

    def forward(self, x, dim=1):
        return self.quad(x, dim)
