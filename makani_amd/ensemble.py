"""``EnsembleScores``: probabilistic scores of an ensemble forecast per lead time, the counterpart of ``MetricsHandler``
(``metric.py``) for E perturbed members -- the runs the reference configures with ``n_initial_conditions``, ``noise_std`` and
``perturb`` (``inferencer.py``) and scores only member by member.  Per autoregressive step and output channel it keeps

* the CRPS of the ensemble's empirical distribution, ``A - G / 2`` with ``A = E|X - y|`` and ``G = E|X - X'|`` over the members,
  and its fair (unbiased in E) form ``A - G E / (2 (E - 1))``;
* the RMSE of the ensemble mean and the spread (root of the unbiased member variance), both as the mean over samples of the
  root of the latitude-weighted integral, which is ``MetricsHandler``'s convention for the RMSE, and their ratio with the
  finite-ensemble factor ``sqrt((E + 1) / E)`` (1 for a statistically consistent ensemble);
* the rank histogram of the target among the members, as integer counts, and the number of points skipped for a NaN.

Built from the same ``params`` as ``MetricsHandler`` (grid, crop, ``valid_autoreg_steps``, ``N_out_channels``) with the same
normalised latitude weights, cut to this rank's shard.  ``update`` is one ``ops.ensemble_sums`` pass (``csrc/ens.hip`` on CUDA
tensors with ``MK_ENSEMBLE=hip``) and an epilogue on ``[B, C]`` that stays on the device: no host synchronisation, capturable.
Under spatial parallelism the ``[B, C, 4]`` float64 sums are all-reduced over ``"spatial"`` per update (the roots come after
the reduction); the rank counts add up over shards and are reduced once, in ``finalize``.  All scores are linear in a
channel's scale, so scoring runs on normalised fields and ``finalize(stds)`` scales the curves.

``EnsembleCRPSLoss`` is the same score as a training loss (``ops.ensemble_crps_sums``: the forward pass above, and one HIP pass
for the gradient with respect to the members), selected by the ``crps`` strings of ``losses.LossHandler``; ``perturb_members``
makes the E members of a training step the way ``EnsembleRollout`` makes those of a rollout.

``EnsembleProducts`` turns the members into the planes a forecast is delivered as -- ensemble mean, spread, quantiles, the
probability of crossing a threshold -- in one ``ops.ensemble_products`` pass (``csrc/ens_products.hip`` with
``MK_ENS_PRODUCTS=hip``), so that ``EnsembleRollout.run(products=...)`` copies K planes per lead time to the host, not E fields.

``EnsembleSpectralCRPSLoss`` is the CRPS of the members' spherical-harmonic coefficients (``ops.spectral_crps_sums`` on the
transform's packed spectra, one HIP pass each way), selected by the words ``spectral`` and ``combined`` of the ``crps`` strings.
"""
import math

import torch
import torch.distributed as dist
from torch import nn

from . import comm, ops
from .distributed import all_reduce_spatial, real_sht, shard_span
from .losses import GridQuadrature


class EnsembleScores:
    """Buffers and arithmetic of the ensemble scores (see the module docstring).  ``members``: E >= 1, fixed."""

    def __init__(self, params, members, device):
        self.device = torch.device(device)
        self.members = int(members)
        if self.members < 1:
            raise ValueError(f"EnsembleScores: members must be at least 1, got {members}")
        if getattr(params, "split_data_channels", False) and comm.get_size("matmul") > 1:
            raise NotImplementedError("EnsembleScores: channel (matmul) parallelism is not supported")
        self.steps = int(params.valid_autoreg_steps) + 1
        self.N_out_channels = int(params.N_out_channels)
        self.img_shape = (params.img_shape_x, params.img_shape_y)
        self.crop_shape = (params.img_crop_shape_x, params.img_crop_shape_y)
        self.crop_offset = (params.img_crop_offset_x, params.img_crop_offset_y)
        rule = "legendre-gauss" if params.model_grid_type == "legendre_gauss" else "naive"
        quad = GridQuadrature(rule, img_shape=self.img_shape, crop_shape=self.crop_shape, crop_offset=self.crop_offset, normalize=True)
        h0, hs = shard_span(self.crop_shape[0], "h")
        self.wrow = quad.row_weights[h0:h0 + hs].float().contiguous().to(self.device)
        C, E = self.N_out_channels, self.members
        self.sums = torch.zeros(self.steps, C, 4, dtype=torch.float64, device=self.device)      # over samples: A, G, sqrt Q, sqrt V
        self.counter = torch.zeros(self.steps, dtype=torch.float64, device=self.device)          # samples per lead time
        self.rank_histogram = torch.zeros(self.steps, C, E + 1, dtype=torch.int64, device=self.device)
        self.skipped = torch.zeros(self.steps, C, dtype=torch.int64, device=self.device)
        self.last_sums = None

    def zero_buffers(self):
        """set buffers to zero"""
        with torch.no_grad():
            for t in (self.sums, self.counter, self.rank_histogram, self.skipped):
                t.fill_(0)

    def update(self, ens, tar, idt):
        """accumulate one lead time: ``ens`` ``[B, E, C, H, W]`` or ``[B * E, C, H, W]`` (member fastest), ``tar``
        ``[B, C, H, W]``, both this rank's shard; no host synchronisation"""
        with torch.no_grad():
            B = tar.shape[0]
            if ens.numel() != self.members * tar.numel():
                raise ValueError(f"EnsembleScores.update: ensemble {tuple(ens.shape)} is not {self.members} members of a target "
                                 f"{tuple(tar.shape)}")
            s = all_reduce_spatial(ops.ensemble_sums(ens, tar, self.wrow, self.rank_histogram[idt], self.skipped[idt]))
            self.sums[idt, :, :2] += s[..., :2].sum(dim=0)
            self.sums[idt, :, 2:] += torch.sqrt(s[..., 2:]).sum(dim=0)
            self.counter[idt] += B
            self.last_sums = s              # [B, C, 4] float64 of the whole field (ops.ENSEMBLE_SUMS), this update's

    def finalize(self, stds=None):
        """Reduce over the ranks and return the curves, ``[steps, C]`` float64 on the device, averaged over samples:
        ``crps``, ``fair_crps``, ``ens_mean_rmse``, ``spread`` (times ``stds`` ``[C]`` where given), ``spread_skill``, and the
        counts ``rank_histogram`` ``[steps, C, E + 1]`` and ``skipped`` ``[steps, C]`` (int64).  A lead time without an update
        is NaN.  The accumulators are left as they are."""
        E = self.members
        with torch.no_grad():
            sums, n = self.sums.clone(), self.counter.clone()
            ranks, skipped = self.rank_histogram.clone(), self.skipped.clone()
            for t in (ranks, skipped):          # every spatial rank counted its own shard; the sums are whole already
                all_reduce_spatial(t)
            if dist.is_initialized() and comm.get_size("data") > 1:
                for t in (sums, n, ranks, skipped):
                    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=comm.get_group("data"))
            mean = sums / n.reshape(-1, 1, 1)
            A, G, rmse, spread = mean.unbind(dim=-1)
            nan = torch.full_like(A, float("nan"))
            out = {"crps": A - 0.5 * G, "fair_crps": A - G * (E / (2.0 * (E - 1))) if E > 1 else nan,
                   "ens_mean_rmse": rmse, "spread": spread}
            if stds is not None:
                stds = torch.as_tensor(stds, dtype=torch.float64).reshape(1, -1).to(self.device)
                out = {k: v * stds for k, v in out.items()}
            out["spread_skill"] = math.sqrt((E + 1) / E) * out["spread"] / out["ens_mean_rmse"]
            out["rank_histogram"], out["skipped"] = ranks, skipped
        return out


class EnsembleProducts:
    """The forecast products of an ensemble of ``members`` members, per point: ``__call__(ens)`` with ``ens`` ``[B, E, C, H, W]``
    (or the model's ``[B * E, C, H, W]``, member fastest, which is viewed) returns ``[B, K, Cs, H, W]`` of ``out_dtype`` from one
    ``ops.ensemble_products`` pass.

    ``products`` is a list of K specs (at most ``ops.ENS_PRODUCTS_MAX`` on the HIP pass):

    * ``"mean"``, ``"std"`` (the spread: root of the unbiased member variance), ``"min"``, ``"max"``, ``"median"``;
    * ``("quantile", q)``: numpy's ``linear`` quantile of the members, ``0 <= q <= 1`` (``ops.quantile_position``);
    * ``("above", thr)``, ``("below", thr)``: the fraction of members strictly above / below a threshold.  ``thr`` is a float,
      for all selected channels, or ``{channel index: value}`` by the members' channel index; a selected channel without a value
      gets a NaN threshold and so a NaN plane.

    ``channels`` selects and orders the member channels (repeats allowed; None: all).  ``stats = (means, stds)``, one value per
    selected channel in the order of ``channels`` as ``Rollout.run``'s ``output_stats``, de-normalises inside the pass: mean and
    order statistics come out as ``v * std + mean``, the spread as ``v * std``, the fractions as they are; ``stds`` must be positive.
    ``thresholds_in="output"`` (the default): thresholds are in the units of the result, physical ones with ``stats``, and are
    converted once on the host in float64, ``(thr - mean) / std``, rounded to fp32; the event is defined on the members as they
    are, the normalised ones.  ``thresholds_in="members"``: thresholds are in the members' units and taken as they are.

    ``names`` are K strings, ``table`` the ``(kinds, orders, fracs)`` of ``ops.ensemble_products``.  The device tables (channel
    list, thresholds, statistics) are uploaded once per device and channel count: a captured caller keeps reading the same tensors."""

    def __init__(self, members, products, channels=None, stats=None, thresholds_in="output", out_dtype=torch.float32):
        self.members = E = int(members)
        if E < 1:
            raise ValueError(f"EnsembleProducts: members must be at least 1, got {members}")
        if thresholds_in not in ("output", "members"):
            raise ValueError(f"EnsembleProducts: thresholds_in must be 'output' or 'members', got {thresholds_in!r}")
        self.thresholds_in, self.out_dtype = thresholds_in, out_dtype
        self.channels = None if channels is None else [int(c) for c in channels]
        if self.channels is not None and (not self.channels or min(self.channels) < 0):
            raise ValueError(f"EnsembleProducts: channels {self.channels} must be a non-empty list of channel indices")
        self.means = self.stds = None
        if stats is not None:
            self.means, self.stds = (torch.as_tensor(t, dtype=torch.float64).reshape(-1).cpu() for t in stats)
            if self.means.numel() != self.stds.numel() or (self.channels is not None and self.means.numel() != len(self.channels)):
                raise ValueError(f"EnsembleProducts: stats have {self.means.numel()} means and {self.stds.numel()} stds for "
                                 f"{'all' if self.channels is None else len(self.channels)} selected channels")
            if not bool((self.stds > 0).all()):
                raise ValueError("EnsembleProducts: stds must be positive")
        kinds, orders, fracs, self.names, self._thr = [], [], [], [], []
        fixed = {"mean": (0, 0, 0.0), "std": (1, 0, 0.0), "min": (2, 0, 0.0), "max": (2, E - 1, 0.0),
                 "median": (2,) + ops.quantile_position(0.5, E)}
        for spec in products:
            thr = None
            if isinstance(spec, str) and spec in fixed:
                row, name = fixed[spec], spec
            elif isinstance(spec, (tuple, list)) and len(spec) == 2 and spec[0] == "quantile":
                row, name = (2,) + ops.quantile_position(spec[1], E), f"q{float(spec[1]):g}"
            elif isinstance(spec, (tuple, list)) and len(spec) == 2 and spec[0] in ("above", "below"):
                thr = {int(c): float(v) for c, v in spec[1].items()} if isinstance(spec[1], dict) else float(spec[1])
                row, name = (3 if spec[0] == "above" else 4, 0, 0.0), spec[0] if isinstance(thr, dict) else f"{spec[0]}_{thr:g}"
            else:
                raise ValueError(f"EnsembleProducts: unknown product {spec!r} (mean, std, min, max, median, ('quantile', q), "
                                 "('above', thr), ('below', thr))")
            kinds.append(row[0]), orders.append(row[1]), fracs.append(row[2]), self.names.append(name), self._thr.append(thr)
        if not kinds:
            raise ValueError("EnsembleProducts: no products")
        self.table = (kinds, orders, fracs)
        self._tables = {}

    def thresholds(self, C):
        """``[K, Cs]`` fp32 on the host, as the pass compares them with the members of ``C`` channels (NaN where a product has no
        threshold or a channel no value), or None without a count product."""
        if all(t is None for t in self._thr):
            return None
        chans = list(range(C)) if self.channels is None else self.channels
        out = torch.full((len(self._thr), len(chans)), float("nan"), dtype=torch.float64)
        for i, thr in enumerate(self._thr):
            if thr is not None:
                for j, c in enumerate(chans):
                    if not isinstance(thr, dict) or c in thr:
                        out[i, j] = thr[c] if isinstance(thr, dict) else thr
        if self.means is not None and self.thresholds_in == "output":
            out = (out - self.means.reshape(1, -1)) / self.stds.reshape(1, -1)
        return out.float()

    def _device_tables(self, device, C):
        key = (str(device), C)
        if key not in self._tables:
            if self.channels is not None and max(self.channels) >= C:
                raise ValueError(f"EnsembleProducts: channels {self.channels} out of range for {C} channels")
            Cs = C if self.channels is None else len(self.channels)
            if self.means is not None and self.means.numel() != Cs:
                raise ValueError(f"EnsembleProducts: stats have {self.means.numel()} values for {Cs} selected channels")
            thr = self.thresholds(C)
            self._tables[key] = (None if self.channels is None else torch.tensor(self.channels, dtype=torch.int32, device=device),
                                 None if thr is None else thr.to(device),
                                 None if self.stds is None else self.stds.float().to(device),
                                 None if self.means is None else self.means.float().to(device))
        return self._tables[key]

    def __call__(self, ens, out=None):
        E = self.members
        if ens.dim() == 4 and ens.shape[0] % E == 0:
            shape = (ens.shape[0] // E, E) + tuple(ens.shape[1:])
            ens = ens.view(shape) if ens.is_contiguous() else ens.reshape(shape)
        if ens.dim() != 5 or ens.shape[1] != E:
            raise ValueError(f"EnsembleProducts: ensemble {tuple(ens.shape)} must be [B, {E}, C, H, W] or [B * {E}, C, H, W]")
        chans, thr, scale, shift = self._device_tables(ens.device, ens.shape[2])
        return ops.ensemble_products(ens, *self.table, chans=chans, thr=thr, scale=scale, shift=shift, out=out, out_dtype=self.out_dtype)


def member_noise(noise, shape, members, dtype):
    """``[B, E - 1, ...]`` fields of ``noise`` (a ``noise.SphericalNoise``) for members 1 ... E - 1 of ``shape`` = ``[B, ..., H, W]``: one
    call of ``noise.sample`` with ``B (E - 1) prod(...)`` rows, ordered (sample, member - 1, the remaining leading dims)."""
    B, lead = shape[0], tuple(shape[1:-2])
    rows = B * (int(members) - 1) * math.prod(lead)
    z = noise.sample(rows, batch=B * (int(members) - 1))
    if tuple(z.shape[-2:]) != tuple(shape[-2:]):
        raise ValueError(f"perturb_members: the noise is on a {tuple(z.shape[-2:])} grid, the fields on {tuple(shape[-2:])}")
    return z.view((B, int(members) - 1) + lead + tuple(z.shape[-2:])).to(dtype)


def perturb_members(x, members, noise_std, generator=None, noise=None):
    """``[B * E, ...]`` from ``x`` ``[B, ...]``: each sample E = ``members`` times (member fastest), ``noise_std * N(0, 1)``
    (``torch.randn`` with ``generator``) added to members 1 ... E - 1; member 0 is the unperturbed control.  A new tensor.  A
    training step of an ensemble is ``perturb_members`` -> the stepper at batch ``B * E`` -> ``LossHandler`` with a ``crps`` loss.

    With ``noise`` (a ``noise.SphericalNoise`` on the grid of ``x`` ``[B, ..., H, W]``) the perturbation is ``noise_std`` times one
    ``noise.sample`` of ``B (E - 1) prod(x.shape[1:-2])`` rows instead: row ``(b (E - 1) + (e - 1)) prod(...) + j`` is the field added
    to member e of sample b at flat index j of the remaining leading dims (sample, member - 1, leading dims: C order).
    ``generator`` is then unused."""
    B, E = x.shape[0], int(members)
    out = x.repeat_interleave(E, dim=0)
    if E > 1 and noise_std != 0.0:
        if noise is not None:
            out.view((B, E) + tuple(x.shape[1:]))[:, 1:] += noise_std * member_noise(noise, x.shape, E, x.dtype)
            return out
        noise = torch.randn((B, E - 1) + tuple(x.shape[1:]), generator=generator, device=x.device, dtype=x.dtype)
        out.view((B, E) + tuple(x.shape[1:]))[:, 1:] += noise_std * noise
    return out


class _EnsembleCRPSBase(nn.Module):
    """What the two CRPS losses share: the checks on ``members`` and ``alpha``, ``kappa = 1 + alpha / (E - 1)``, and the loss
    ``sum_bc chw_c (S0 - kappa / 2 S1)`` in fp32 from the ``[B, C, 2]`` float64 sums of the subclass's ``sums``."""

    def __init__(self, members, alpha):
        super().__init__()
        name = type(self).__name__
        self.members, self.alpha = int(members), float(alpha)
        if self.members < 1:
            raise ValueError(f"{name}: members must be at least 1, got {members}")
        if not 0.0 <= self.alpha <= 1.0:
            raise ValueError(f"{name}: alpha must lie in [0, 1], got {alpha}")
        if self.members == 1 and self.alpha != 0.0:
            raise ValueError(f"{name}: the fair forms need at least 2 members")
        self.kappa = 1.0 + (self.alpha / (self.members - 1) if self.members > 1 else 0.0)

    def from_sums(self, sums, chw):
        """The loss (fp32) from the sums of the whole field (of the whole spectrum)."""
        s0, s1 = sums.unbind(-1)
        return torch.sum(chw * (s0 - (0.5 * self.kappa) * s1)).float()

    def forward(self, prd, tar, chw):
        return self.from_sums(self.sums(prd, tar), chw)


class EnsembleCRPSLoss(_EnsembleCRPSBase):
    """The CRPS of the members' empirical distribution as a training loss: per point ``a - (kappa / 2) g`` with
    ``a = mean_e |x_e - y|``, ``g = mean_ef |x_e - x_f|`` and ``kappa = 1 + alpha / (E - 1)`` -- ``alpha = 0`` the CRPS, ``alpha = 1``
    the fair CRPS (unbiased in E), in between the almost-fair CRPS -- integrated with the latitude weights ``GeometricLpLoss``
    uses (normalised, ``pole_mask`` rows zero) and reduced as its absolute, not squared ``p = 1`` form: ``forward(prd, tar, chw)``
    is ``sum_bc chw_c (S0 - kappa / 2 S1)`` in fp32, so E equal members give the ``absolute geometric l1`` loss of the same fields.

    ``prd`` is ``[B * E, C, H, W]`` (member fastest) or ``[B, E, C, H, W]``, ``tar`` ``[B, C, H, W]``.  The two integrals come from
    ``ops.ensemble_crps_sums`` (``MK_ENS_LOSS=hip``: one HIP pass each way); they add up over spatial shards (``sums`` with
    ``rows``), so a sharded caller all-reduces ``[B, C, 2]`` and calls ``from_sums``.  ``last_sums`` is the detached ``[B, C, 4]``
    (``ops.ENSEMBLE_SUMS``) of the latest call over the rows it was given: spread and ensemble-mean error for a log."""

    def __init__(self, img_shape, crop_shape, crop_offset, members, alpha=0.0, pole_mask=0, quadrature_rule="naive"):
        super().__init__(members, alpha)
        self.quadrature = GridQuadrature(quadrature_rule, img_shape=img_shape, crop_shape=crop_shape, crop_offset=crop_offset,
                                         normalize=True, pole_mask=pole_mask)
        wrow = self.quadrature.row_weights.contiguous()
        self.register_buffer("wrow", wrow, persistent=False)
        self.register_buffer("wrow32", wrow.float(), persistent=False)
        self.last_sums = None

    def sums(self, prd, tar, rows=None):
        """``[B, C, 2]`` float64 integrals of ``a`` and ``g`` over the fields' latitude rows ``rows`` (a slice of the cropped
        grid's rows; all of them by default) -- they add up over spatial shards."""
        if prd.numel() != self.members * tar.numel():
            raise ValueError(f"EnsembleCRPSLoss: prediction {tuple(prd.shape)} is not {self.members} members of a target "
                             f"{tuple(tar.shape)}")
        wrow = self.wrow32 if prd.is_cuda else self.wrow
        s, self.last_sums = ops.ensemble_crps_sums(prd, tar, wrow if rows is None else wrow[rows], with_sums=True)
        return s


class EnsembleSpectralCRPSLoss(_EnsembleCRPSBase):
    """The CRPS of the members' spherical-harmonic coefficients as a training loss.  A CRPS per grid point says nothing about
    how the members' variance is spread over scales; this term does.  For every coefficient, its real and imaginary part each
    taken as a real number, ``a = mean_e |x_e - y|`` and ``g = mean_ef |x_e - x_f|``; they are summed over the orders with the
    weight of every spectral norm here (``m > 0`` twice), over the degrees with ``degree_weights`` ``[lmax]`` (ones by default)
    and multiplied by ``scale``:

        ``forward(prd, tar, chw) = sum_bc chw_c (S0 - kappa / 2 S1)`` in fp32,   ``kappa = 1 + alpha / (E - 1)`` as in ``EnsembleCRPSLoss``.

    ``scale`` defaults to ``1 / sqrt(4 pi)``: the harmonics are orthonormal, a spatially constant field ``v`` has the one
    coefficient ``c_00 = sqrt(4 pi) v``, so a constant error costs here what it costs in the grid-space loss.

    ``prd`` is ``[B * E, C, H, W]`` (member fastest) or ``[B, E, C, H, W]``, ``tar`` ``[B, C, H, W]``, fp32 or bf16, on the whole
    sphere ``img_shape``.  The transform is ``RealSHT`` -- ``DistributedRealSHT`` when ``comm.get_size("spatial") > 1``, fed with
    the rank's own shard -- and its packed spectra go straight into ``ops.spectral_crps_sums`` (``MK_SPEC_CRPS=hip``: one HIP pass
    each way); the degree weights act in torch on the small per-degree tensor.  Sharded, ``sums`` returns the partial sums of
    the rank's degrees and orders: they add up, so the caller all-reduces ``[B, C, 2]`` over ``"spatial"`` and calls
    ``from_sums``.  ``last_degree_sums`` is the detached ``[B, C, L, 2]`` of the latest call, scaled by ``scale`` but not by the
    degree weights: ``[..., 0] - kappa / 2 [..., 1]`` is the CRPS per degree, for a log."""

    def __init__(self, img_shape, members, alpha=0.0, grid="equiangular", degree_weights=None, scale=None):
        super().__init__(members, alpha)
        self.sharded = comm.get_size("spatial") > 1
        self.sht = real_sht(img_shape, grid)
        if degree_weights is None:
            degree_weights = torch.ones(self.sht.lmax, dtype=torch.float64)
        degree_weights = torch.as_tensor(degree_weights, dtype=torch.float64).reshape(-1)
        if degree_weights.numel() != self.sht.lmax:
            raise ValueError(f"EnsembleSpectralCRPSLoss: {degree_weights.numel()} degree weights for lmax = {self.sht.lmax}")
        self.register_buffer("degree_weights", degree_weights, persistent=False)
        self.scale = 1.0 / math.sqrt(4.0 * math.pi) if scale is None else float(scale)
        self.last_degree_sums = None

    def sums_from_spectrum(self, cp, ct, batch, l_off=0, m_off=0):
        """``[batch, C, 2]`` float64 from packed spectra ``cp`` ``[L_loc, M_loc, batch * E * C]`` and ``ct`` ``[L_loc, M_loc, batch * C]`` of the
        degrees from ``l_off`` and the orders from ``m_off`` on.  They add up over the shards of a spectrum."""
        s = ops.spectral_crps_sums(cp, ct, self.members, l_off, m_off, batch) * self.scale        # [batch * C, L_loc, 2]
        nl = s.shape[1]
        self.last_degree_sums = s.detach().reshape(batch, -1, nl, 2)
        wl = self.degree_weights[l_off:l_off + nl].reshape(1, nl, 1)                              # of the GLOBAL degree
        return (s * wl).sum(dim=1).reshape(batch, -1, 2)

    def sums(self, prd, tar):
        """``[B, C, 2]`` float64 of the fields (this rank's shard of them under spatial parallelism, where the sums are those of
        the rank's degrees and orders)."""
        if tar.dim() != 4 or prd.numel() != self.members * tar.numel() or tuple(prd.shape[-3:]) != tuple(tar.shape[-3:]):
            raise ValueError(f"EnsembleSpectralCRPSLoss: prediction {tuple(prd.shape)} is not {self.members} members of a target "
                             f"{tuple(tar.shape)}")
        B, C, H, W = tar.shape
        want = (self.sht.nlat_local, self.sht.nlon_local) if self.sharded else (self.sht.nlat, self.sht.nlon)
        if (H, W) != want:
            raise ValueError(f"EnsembleSpectralCRPSLoss: expected [..., {want[0]}, {want[1]}], got {tuple(tar.shape)}")
        cp = self.sht.forward_packed_fields(ops._lowp(prd).reshape(B * self.members, C, H, W))[0]
        ct, l_off, m_off = self.sht.forward_packed_fields(ops._lowp(tar))
        return self.sums_from_spectrum(cp, ct, B, l_off, m_off)
