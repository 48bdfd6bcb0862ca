"""Dataset statistics: the seven files of ``data_process/get_stats.py`` (``global_means.npy``, ``global_stds.npy``,
``mins.npy``, ``maxs.npy``, ``time_means.npy``, ``time_diff_means.npy``, ``time_diff_stds.npy``) from one pass per batch.

``DatasetStats.update`` hands a batch ``[T, C, H, W]`` of consecutive samples to ``ops.field_stats`` (one HIP pass on a
device tensor, ``MK_STATS=hip``; float64 torch ops on CPU tensors and with ``MK_STATS=torch``) and keeps raw float64 sums
about a per-channel pivot, which is fixed at the first update from that batch (the unweighted mean of its first sample,
rounded to fp32): with ``d = x - pivot`` the sums ``sum w d`` and ``sum w d^2`` lose nothing to cancellation for a channel
whose offset is large against its spread, later batches simply add, and mean and variance follow at the end,

    mean = (sum w x) / n,                 sum w x = sum w d + pivot * sum w,
    var  = (sum w d^2 - 2 (mean - pivot) sum w d + (mean - pivot)^2 sum w) / n,

with ``n`` the number of samples and ``w`` the row weights of ``GridQuadrature(rule, img_shape, normalize=True)``, which
is what the reference's per-batch means and its Welford combination add up to.  Two accumulators with different pivots
``p`` and ``q`` combine exactly: ``d_q = d_p + (p - q)``, so ``sum w d_q = sum w d_p + (p - q) sum w`` and
``sum w d_q^2 = sum w d_p^2 + 2 (p - q) sum w d_p + (p - q)^2 sum w`` (``merge``).

Deviations from the reference script (``finalize`` otherwise returns its shapes and dtypes, float64 ``[1, C, 1, 1]`` and
``[1, C, H, W]``):

1. Time-difference variance.  The reference multiplies the per-batch variance of ``e = x[t] - x[t - 1]`` by ``4 pi`` and
   keeps a count of ``(T - 1) H W`` points for it (get_stats.py:187-189), so for one batch its ``time_diff_stds`` is the
   weighted standard deviation times ``sqrt(4 pi / (H W))`` (``reference_time_diff_factor``).  Across batches its Welford
   step adds the spread of the batch means of ``e`` with the point counts as weights, i.e. WITHOUT that factor:
   ``ref^2 = (4 pi / (H W)) within / m + between / m`` for ``m`` differences, so the reference's file depends on the batch
   size.  This module returns the standard deviation itself, ``sqrt((within + between) / m)``; multiply by the factor for
   the reference's scale (exact for one batch, and up to the small between-batch term otherwise).
2. Wind variance.  The reference adds up only the within-batch variances of the wind magnitude and stores a mean of zero
   (get_stats.py:194-198).  This module returns the standard deviation of ``sqrt(u^2 + v^2)`` over the whole dataset,
   unweighted as in the reference, in ``global_stds`` of both channels of a pair, with their ``global_means`` set to zero.
3. Climatology.  ``time_means`` is one float64 running sum per point divided by the number of samples, not a mean of
   fp32 batch means.
4. ``mins`` / ``maxs`` are those of the data; the reference's start values of zero (get_stats.py:359-360) clamp its files
   to ``min <= 0 <= max``.
5. The reference joins batches as if the quadrature weights of a sample added up to exactly one.  The fp32 weights add
   up to ``sw = 1 + O(1e-7)``; here ``mean = (sum w x) / n`` as in the reference, and the variance is
   ``sum w (x - mean)^2 / n`` over the whole dataset, which differs from the reference's by at most
   ``|sw - 1| sum_b t_b (2 |mu_b - mu| |mu_b| + (mu_b - mu)^2) / n`` (``mu_b`` the mean of batch b of ``t_b`` samples): nothing
   for one batch, 3e-4 of the variance for a channel whose offset is 3e4 times its spread.
6. ``carry=False`` drops the difference across a batch boundary, as the reference does (get_stats.py:168);
   ``carry=True`` keeps the last sample of a batch on the device and hands it to the next call, and the result then does
   not depend on the batch size.  Without any difference (one sample) ``time_diff_means`` is 0 and ``time_diff_stds``
   NaN.
"""
import math
import os

import numpy as np
import torch
import torch.distributed as dist

from . import comm, ops
from .distributed import shard_span
from .losses import GridQuadrature

FILES = ("global_means", "global_stds", "mins", "maxs", "time_means", "time_diff_means", "time_diff_stds")


def reference_time_diff_factor(img_shape):
    """``sqrt(4 pi / (H W))``: the reference's ``time_diff_stds`` of one batch over this module's (deviation 1)."""
    return math.sqrt(4.0 * math.pi / (img_shape[0] * img_shape[1]))


def get_wind_channels(channel_names):
    """``(u channels, v channels)``: every name ``u<level>`` that has a partner ``v<level>`` (get_stats.py:207-222)."""
    index = {name: i for i, name in enumerate(channel_names)}
    pairs = [(i, index["v" + name[1:]]) for name, i in index.items() if name[:1] == "u" and "v" + name[1:] in index]
    return [u for u, _ in pairs], [v for _, v in pairs]


def _shift(sums, delta, wtot):
    """The sums about pivot ``p`` as sums about ``q``, ``delta = p - q`` (float64 ``[C]``), ``wtot = sum w``."""
    out = sums.clone()
    out[:, 0] = sums[:, 0] + delta * wtot
    out[:, 1] = sums[:, 1] + 2.0 * delta * sums[:, 0] + delta * delta * wtot
    return out


class DatasetStats:
    """Running statistics of a dataset of ``[C, H, W]`` samples; see the module docstring.

    ``wind_pairs``: ``(u channels, v channels)`` as ``get_wind_channels`` returns them, or None.  Under spatial model
    parallelism (``comm.get_size("spatial") > 1``) ``img_shape`` is the global grid, ``update`` takes this rank's rows and
    columns, and ``shard_reduce`` combines the shards."""

    def __init__(self, num_channels, img_shape, quadrature_rule="naive", wind_pairs=None, carry=False):
        self.C = int(num_channels)
        self.img_shape = (int(img_shape[0]), int(img_shape[1]))
        self.carry = bool(carry)
        (h0, self.H), (_, self.W) = shard_span(self.img_shape[0], "h"), shard_span(self.img_shape[1], "w")
        wrow = GridQuadrature(quadrature_rule, self.img_shape, normalize=True).row_weights
        self.wrow = wrow[h0:h0 + self.H].float().contiguous()
        self.sw = float(self.wrow.double().sum()) * self.W            # sum of the weights over one sample (this shard)
        self.wind_pairs = None
        if wind_pairs is not None and len(wind_pairs[0]) > 0:
            u, v = [int(i) for i in wind_pairs[0]], [int(i) for i in wind_pairs[1]]
            if len(u) != len(v) or len(set(u)) != len(u) or min(u + v) < 0 or max(u + v) >= self.C:
                raise ValueError(f"DatasetStats: wind pairs {u} / {v} must be as many distinct u as v channels below {self.C}")
            self.wind_pairs = (u, v)
        self.device = None
        self.n_time = 0             # samples
        self.n_diff = 0             # time differences
        self.wtot = 0.0             # sum of w over everything that went into sums[:, :2]
        self.wtot_diff = 0.0        # ... into sums[:, 2:]
        self.npts = 0               # points (samples x H x W) behind the wind sums

    # -- state -------------------------------------------------------------------------------------------------------------
    def _alloc(self, device):
        self.device = torch.device(device)
        kw = dict(dtype=torch.float64, device=self.device)
        self.wrow = self.wrow.to(self.device)
        self.pivot = torch.zeros(self.C, dtype=torch.float32, device=self.device)
        self.sums = torch.zeros(self.C, 4, **kw)
        self.mins = torch.full((self.C,), float("inf"), dtype=torch.float32, device=self.device)
        self.maxs = torch.full((self.C,), float("-inf"), dtype=torch.float32, device=self.device)
        self.tsum = torch.zeros(self.C, self.H, self.W, **kw)
        self.wind_u = self.wind_v = self.wsums = None
        if self.wind_pairs is not None:
            self.wind_u = torch.tensor(self.wind_pairs[0], dtype=torch.int32, device=self.device)
            self.wind_v = torch.tensor(self.wind_pairs[1], dtype=torch.int32, device=self.device)
            self.wsums = torch.zeros(len(self.wind_pairs[0]), 2, **kw)
        self.last = torch.zeros(self.C, self.H, self.W, dtype=torch.float32, device=self.device) if self.carry else None
        self.have_last = False

    @torch.no_grad()
    def update(self, batch):
        """Add a batch ``[T, C, H, W]`` of samples that are consecutive in time (fp32; on the device the sums should live on).
        No host synchronisation; after the first call the launches are the same every time, so a call can be captured.
        The numbers of samples and differences are kept on the host: capturing a call counts it once, for its first
        replay; every further replay of the graph needs ``count(T)``, or ``finalize`` divides by too little."""
        if batch.dim() != 4 or tuple(batch.shape[1:]) != (self.C, self.H, self.W) or batch.shape[0] < 1:
            raise ValueError(f"DatasetStats.update: batch {tuple(batch.shape)} is not [T, {self.C}, {self.H}, {self.W}]")
        batch = batch.float()
        if self.device is None:
            self._alloc(batch.device)
        elif batch.device != self.device:
            raise ValueError(f"DatasetStats.update: batch on {batch.device}, the sums on {self.device}")
        T = batch.shape[0]
        if self.n_time == 0:
            self.pivot.copy_(batch[0].mean((-2, -1)))        # any value near the data serves; it only has to stay fixed
        prev = self.last if (self.carry and self.have_last) else None
        sums, minmax, wsums = ops.field_stats(batch, self.wrow, self.tsum, prev=prev, pivot=self.pivot, wind_u=self.wind_u,
                                              wind_v=self.wind_v)
        self.sums += sums
        torch.minimum(self.mins, minmax[:, 0], out=self.mins)         # minimum / maximum keep a NaN
        torch.maximum(self.maxs, minmax[:, 1], out=self.maxs)
        if wsums is not None:
            self.wsums += wsums
        self.count(T, prev is not None)
        if self.carry:
            self.last.copy_(batch[-1])
            self.have_last = True
        return self

    def count(self, T, with_prev=None):
        """The host side of one ``update`` of ``T`` samples: the numbers of samples, differences and points and the weight
        totals.  ``update`` calls it; a caller that replays a captured ``update`` calls it once per replay after the
        first.  ``with_prev``: whether the call had the carried sample (default: what the next ``update`` would have)."""
        if with_prev is None:
            with_prev = self.carry and self.have_last
        nd = T - 1 + (1 if with_prev else 0)
        self.n_time += T
        self.n_diff += nd
        self.wtot += T * self.sw
        self.wtot_diff += nd * self.sw
        self.npts += T * self.H * self.W
        return self

    def _add(self, pivot, sums, mins, maxs, wsums, n_time, n_diff, wtot, wtot_diff, npts):
        """Fold another accumulator's small state (tensors on this device) into this one; ``tsum`` is the caller's."""
        if n_time == 0:
            return
        if self.n_time == 0:
            self.pivot.copy_(pivot)
        delta = pivot.double() - self.pivot.double()
        self.sums += _shift(sums, delta, wtot)
        torch.minimum(self.mins, mins.float(), out=self.mins)
        torch.maximum(self.maxs, maxs.float(), out=self.maxs)
        if self.wsums is not None:
            self.wsums += wsums
        self.n_time += n_time
        self.n_diff += n_diff
        self.wtot += wtot
        self.wtot_diff += wtot_diff
        self.npts += npts

    @torch.no_grad()
    def merge(self, other):
        """Fold ``other`` (same channels, grid and wind pairs; any pivot; later in time) into this accumulator."""
        if (other.C, other.H, other.W, other.wind_pairs) != (self.C, self.H, self.W, self.wind_pairs):
            raise ValueError("DatasetStats.merge: the accumulators differ in channels, grid or wind pairs")
        if other.n_time == 0:
            return self
        if self.device is None:
            self._alloc(other.device)
        dev = self.device
        self._add(other.pivot.to(dev), other.sums.to(dev), other.mins.to(dev), other.maxs.to(dev),
                  other.wsums.to(dev) if other.wsums is not None else None, other.n_time, other.n_diff, other.wtot,
                  other.wtot_diff, other.npts)
        self.tsum += other.tsum.to(dev)
        if self.carry and other.carry and other.have_last:
            self.last.copy_(other.last.to(dev))
            self.have_last = True
        return self

    # -- collectives ---------------------------------------------------------------------------------------------------
    def _default_device(self):
        return torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")

    def _pack(self):
        nw = 0 if self.wsums is None else self.wsums.numel()
        counts = torch.tensor([self.n_time, self.n_diff, self.wtot, self.wtot_diff, self.npts], dtype=torch.float64, device=self.device)
        parts = [self.pivot.double(), self.sums.flatten(), self.mins.double(), self.maxs.double()]
        if nw:
            parts.append(self.wsums.flatten())
        return torch.cat(parts + [counts])

    def _unpack(self, vec):
        C = self.C
        nw = 0 if self.wsums is None else self.wsums.numel()
        pivot, sums, mins, maxs = vec[:C].float(), vec[C:5 * C].reshape(C, 4), vec[5 * C:6 * C], vec[6 * C:7 * C]
        wsums = vec[7 * C:7 * C + nw].reshape(-1, 2) if nw else None
        n_time, n_diff, wtot, wtot_diff, npts = vec[7 * C + nw:].tolist()
        return pivot, sums, mins, maxs, wsums, int(n_time), int(n_diff), wtot, wtot_diff, int(npts)

    def _reset_small(self):
        self.sums.zero_()
        self.mins.fill_(float("inf"))
        self.maxs.fill_(float("-inf"))
        if self.wsums is not None:
            self.wsums.zero_()
        self.n_time = self.n_diff = self.npts = 0
        self.wtot = self.wtot_diff = 0.0

    @torch.no_grad()
    def all_reduce(self, group=None):
        """Combine sample-parallel ranks (each saw its own samples of the full grid): the small sums are all-gathered and
        merged in rank order, so every rank ends with the same bits; the time sums are all-reduced.  The difference
        between the last sample of a rank and the first of the next is not formed.  Collective; a rank without samples
        takes part."""
        if not dist.is_initialized() or dist.get_world_size(group) == 1:
            return self
        if self.device is None:
            self._alloc(self._default_device())
        vec = self._pack()
        gathered = [torch.empty_like(vec) for _ in range(dist.get_world_size(group))]
        dist.all_gather(gathered, vec, group=group)
        dist.all_reduce(self.tsum, op=dist.ReduceOp.SUM, group=group)
        self._reset_small()
        for v in gathered:
            self._add(*self._unpack(v))
        return self

    @torch.no_grad()
    def shard_reduce(self):
        """Combine the spatial shards of one model-parallel instance (each saw its own rows and columns of the same
        samples): every shard moves its sums to the pivot of the group's first rank, then the ``[C, 4]`` sums, the wind sums
        and min / max are all-reduced once over ``"spatial"``, as ``MetricsHandler`` does with its sums.  The time sums stay
        local: ``finalize`` returns this rank's shard of the climatology.  Collective."""
        if comm.get_size("spatial") == 1:
            return self
        if self.device is None:
            self._alloc(self._default_device())
        grp = comm.get_group("spatial")
        pivot = self.pivot.clone()
        dist.broadcast(pivot, src=comm.get_root("spatial"), group=grp)
        self.sums.copy_(_shift(self.sums, self.pivot.double() - pivot.double(), self.wtot))
        self.pivot.copy_(pivot)
        counts = torch.tensor([self.wtot, self.wtot_diff, self.npts], dtype=torch.float64, device=self.device)
        dist.all_reduce(self.sums, op=dist.ReduceOp.SUM, group=grp)
        dist.all_reduce(counts, op=dist.ReduceOp.SUM, group=grp)
        dist.all_reduce(self.mins, op=dist.ReduceOp.MIN, group=grp)
        dist.all_reduce(self.maxs, op=dist.ReduceOp.MAX, group=grp)
        if self.wsums is not None:
            dist.all_reduce(self.wsums, op=dist.ReduceOp.SUM, group=grp)
        self.wtot, self.wtot_diff, npts = counts.tolist()
        self.npts = int(npts)
        return self

    # -- results -----------------------------------------------------------------------------------------------------------
    def finalize(self):
        """The seven arrays under the reference's file names (float64 numpy; ``time_means`` ``[1, C, H, W]``, the others
        ``[1, C, 1, 1]``)."""
        if self.n_time == 0:
            raise RuntimeError("DatasetStats.finalize: no sample was added")
        n, m = float(self.n_time), float(self.n_diff)
        s = self.sums.cpu().numpy()
        p = self.pivot.double().cpu().numpy()
        mean = (s[:, 0] + p * self.wtot) / n
        dm = mean - p
        var = (s[:, 1] - 2.0 * dm * s[:, 0] + dm * dm * self.wtot) / n
        if self.n_diff > 0:
            dmean = s[:, 2] / m
            dvar = (s[:, 3] - 2.0 * dmean * s[:, 2] + dmean * dmean * self.wtot_diff) / m
        else:
            dmean, dvar = np.zeros(self.C), np.full(self.C, np.nan)
        std = np.sqrt(np.maximum(var, 0.0))
        if self.wind_pairs is not None:
            w = self.wsums.cpu().numpy()
            wmean = w[:, 0] / self.npts
            wstd = np.sqrt(np.maximum(w[:, 1] / self.npts - wmean * wmean, 0.0))
            for chans in self.wind_pairs:
                mean[chans] = 0.0
                std[chans] = wstd

        def col(v):
            return np.asarray(v, dtype=np.float64).reshape(1, self.C, 1, 1)

        # the time sum is divided on the host: a true division whatever device holds the sums (torch multiplies by 1 / n there)
        return {"global_means": col(mean), "global_stds": col(std), "mins": col(self.mins.cpu().numpy()),
                "maxs": col(self.maxs.cpu().numpy()), "time_means": self.tsum.cpu().numpy()[None] / n,
                "time_diff_means": col(dmean), "time_diff_stds": col(np.sqrt(np.maximum(dvar, 0.0)))}

    def save(self, output_dir):
        """Write the seven ``.npy`` files of ``finalize`` into ``output_dir``; returns the arrays."""
        out = self.finalize()
        os.makedirs(output_dir, exist_ok=True)
        for name in FILES:
            np.save(os.path.join(output_dir, name + ".npy"), out[name])
        return out
