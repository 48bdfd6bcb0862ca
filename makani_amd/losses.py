"""Training losses of the Makani trainer for the hot path: quadrature-weighted Lp norms on the sphere.

Interface and arithmetic of ``makani/utils/grids.py:63-115`` (``GridQuadrature``) and ``makani/utils/losses.py:33-271``
(``LossHandler``, ``GeometricLpLoss``): per-sample, per-channel integrals of ``|prd - tar| ** p`` with the latitude
quadrature of the model grid, relative or absolute, optionally squared, channel-weighted, summed.

The quadrature weights depend on the latitude only, so for p = 1 and p = 2 every spelling is a function of two sums per
(sample, channel), ``sum w |prd - tar| ** p`` and ``sum w |tar| ** p``: one streaming HIP pass over prediction and target
forward and one backward (``ops.geo_lp_sums`` / ``mk_geo_lp_sums``, ``mk_geo_lp_bwd``; torch float64 on CPU tensors),
followed by the ratio, the root, the channel weights and the reduction on ``[B, C]`` tensors.  The absolute squared L2
norm with uniform channel weights -- the loss the bench harness trains with -- keeps its own single pass
(``ops.weighted_mse`` / ``mk_wmse_fwd``, ``mk_wmse_bwd``).  Other ``p`` run on torch ops.

Under spatial model parallelism the reference gathers prediction and target over ``h`` then ``w`` (``losses.py:149-157``)
and every rank integrates both full fields.  The integrals add up across shards, so here a rank integrates its own shard
with its slice of the latitude weights and the ``[B, C, 2]`` float64 sums are all-reduced over the ``"spatial"`` group;
the gradient of the all-reduce is the identity, which leaves every rank with its shard of the global gradient.

The H1 loss (``GeometricH1Loss``) is a function of the per-degree power of the spherical-harmonic coefficients of the
error and of the target: the transform's packed spectrum ``[L, M, BC]`` is summed over the orders by one HIP pass into
float64 (``ops.degree_power`` / ``mk_degree_power``, ``mk_degree_power_bwd``), whose gradient the transform's backward
takes in the same layout.  The degree sums add up over ``m`` shards and concatenate over ``l`` shards, so under spatial
parallelism a rank transforms its own shard with ``DistributedRealSHT`` and the per-sample ``[B, 2]`` float64 sums are
all-reduced over the ``"spatial"`` group: no loss gathers CUDA fields.  (CPU tensors are still gathered first, as the
reference does; the transform has no CPU path.)
"""
import math

import numpy as np
import torch
from torch import nn

from . import comm, ops
from .distributed import compute_split_shapes, real_sht, shard_span
from .mappings import gather_from_parallel_region, reduce_from_parallel_region


def _latitude_weights(rule, nlat):
    """Quadrature weights over cos(theta) in [-1, 1] for the rules of torch_harmonics.quadrature."""
    if rule == "legendre-gauss":
        return torch.from_numpy(ops.quadrature("legendre-gauss", nlat)[1])
    if rule == "clenshaw-curtiss":
        return torch.from_numpy(ops.quadrature("equiangular", nlat)[1])
    raise ValueError(f"Unknown quadrature rule {rule}")


class GridQuadrature(nn.Module):
    """``sum(x * quad_weight, dim=(-2, -1))`` with the weights of grids.py:63-115.

    (``pole_mask > 0`` raises ``NameError`` in the reference, grids.py:98 uses an undefined ``sizes``; here it masks the
    first / last ``pole_mask`` latitude rows, which is what the line above it does for the northern rows.)"""

    def __init__(self, quadrature_rule, img_shape, crop_shape=None, crop_offset=(0, 0), normalize=False, pole_mask=None):
        super().__init__()
        nlat, nlon = img_shape
        if quadrature_rule == "naive":
            jacobian = torch.clamp(torch.sin(torch.linspace(0, torch.pi, nlat)), min=0.0)
            quad_weight = (2 * torch.pi / nlon) * (torch.pi / nlat) * jacobian.unsqueeze(1)
            quad_weight = quad_weight.tile(1, nlon)
            quad_weight = quad_weight * (4.0 * torch.pi) / torch.sum(quad_weight)
        elif quadrature_rule in ("clenshaw-curtiss", "legendre-gauss"):
            w = _latitude_weights(quadrature_rule, nlat)
            quad_weight = ((2 * torch.pi / nlon) * w.unsqueeze(1)).tile(1, nlon)
        else:
            raise ValueError(f"Unknown quadrature rule {quadrature_rule}")
        if normalize:
            quad_weight = quad_weight / (4.0 * torch.pi)
        if (pole_mask is not None) and (pole_mask > 0):
            quad_weight[:pole_mask, :] = 0.0
            quad_weight[nlat - pole_mask:, :] = 0.0
        if crop_shape is not None:
            quad_weight = quad_weight[crop_offset[0]:crop_offset[0] + crop_shape[0], crop_offset[1]:crop_offset[1] + crop_shape[1]]
        quad_weight = quad_weight.contiguous()
        H, W = quad_weight.shape
        self.register_buffer("quad_weight", quad_weight.reshape(1, 1, H, W))

    @property
    def row_weights(self):
        """``[H]``: the weight of each latitude row.  Every rule tiles one column over the longitudes, so the weights do not vary
        along a row and the streaming passes read one per row (a view of ``quad_weight``: nothing is derived again)."""
        return self.quad_weight[0, 0, :, 0]

    def forward(self, x):
        return torch.sum(x * self.quad_weight, dim=(-2, -1))


class GeometricLpLoss(nn.Module):
    """Lp loss on the sphere, losses.py:174-271 (same constructor arguments, same ``forward(prd, tar, chw)``)."""

    def __init__(self, img_shape, crop_shape, crop_offset, p=2.0, size_average=False, reduction=True, absolute=False,
                 squared=False, pole_mask=0, jacobian="s2", quadrature_rule="naive"):
        super().__init__()
        self.p = p
        self.img_shape, self.crop_shape, self.crop_offset = img_shape, crop_shape, crop_offset
        self.reduction, self.size_average = reduction, size_average
        self.absolute, self.squared, self.pole_mask = absolute, squared, pole_mask
        self.quadrature = GridQuadrature(quadrature_rule, img_shape=img_shape, crop_shape=crop_shape, crop_offset=crop_offset,
                                         normalize=True, pole_mask=pole_mask)
        self.uniform_chw = None     # set by the owner of the channel weights when they are all equal (see _fused_abs_sq_l2)
        # one weight per row, as built (CPU float64 path) and in fp32 (kernels)
        wrow = self.quadrature.row_weights.contiguous()
        self.register_buffer("wrow", wrow, persistent=False)
        self.register_buffer("wrow32", wrow.float(), persistent=False)

    def _reduce(self, v):
        if not self.reduction:
            return v
        return torch.mean(v) if self.size_average else torch.sum(v)

    def _fused_abs_sq_l2(self, prd, tar, chw):
        """Absolute squared L2 with one weight for all channels: a single streaming pass (None if it does not apply)."""
        if not (self.p == 2 and self.squared and self.reduction and not self.size_average and prd.is_cuda):
            return None
        if not (prd.dim() == 4 and prd.is_contiguous() and tar.is_contiguous() and tar.dtype == torch.float32
                and prd.dtype in (torch.float32, torch.bfloat16) and prd.shape[-1] % 8 == 0 and chw.numel() > 0):
            return None
        # one weight for all channels?  Known on the host by whoever built the weights (LossHandler sets ``uniform_chw``);
        # never read back from a device tensor here (that would be a synchronisation per step)
        value = self.uniform_chw
        if value is None and not chw.is_cuda:
            c0 = chw.detach().reshape(-1)
            if c0.numel() == prd.shape[1] and bool((c0 == c0[0]).all()):
                value = float(c0[0])
        if value is None:
            return None
        return ops.weighted_mse(prd, tar, self.wrow32, value)

    def has_sums(self, prd, tar):
        """True when the loss is formed from ``sums`` (p = 1 or 2 on [B, C, H, W] fields)."""
        return self.p in (1, 2) and prd.dim() == 4 and tar.shape == prd.shape

    def sums(self, prd, tar, rows=None):
        """``[B, C, 2]`` float64 integrals of ``|prd - tar| ** p`` and ``|tar| ** p`` over the fields' latitude rows
        ``rows`` (a slice of the cropped grid's rows; all of them by default) -- they add up over spatial shards."""
        wrow = self.wrow32 if prd.is_cuda else self.wrow
        return ops.geo_lp_sums(prd, tar, wrow if rows is None else wrow[rows], int(self.p))

    def from_sums(self, sums, chw):
        """The loss (fp32) from the integrals of the whole field: ratio, root, channel weights, reduction."""
        s0, s1 = sums.unbind(-1)
        norms = s0 if self.absolute else s0 / s1
        if not self.squared:
            norms = norms ** (1.0 / self.p)
        return self._reduce(chw * norms).float()

    def abs(self, prd, tar, chw):
        fused = self._fused_abs_sq_l2(prd, tar, chw)
        if fused is not None:
            return fused
        if self.has_sums(prd, tar):
            return self.from_sums(self.sums(prd, tar), chw)
        num_examples = prd.size()[0]
        all_norms = self.quadrature(torch.abs(prd - tar) ** self.p).reshape(num_examples, -1)
        if not self.squared:
            all_norms = all_norms ** (1.0 / self.p)
        return self._reduce(chw * all_norms)

    def rel(self, prd, tar, chw):
        if self.has_sums(prd, tar):
            return self.from_sums(self.sums(prd, tar), chw)
        num_examples = prd.size()[0]
        diff_norms = self.quadrature(torch.abs(prd - tar) ** self.p).reshape(num_examples, -1)
        tar_norms = self.quadrature(torch.abs(tar) ** self.p).reshape(num_examples, -1)
        frac_norms = diff_norms / tar_norms
        if not self.squared:
            frac_norms = frac_norms ** (1.0 / self.p)
        return self._reduce(chw * frac_norms)

    def forward(self, prd, tar, chw):
        return self.abs(prd, tar, chw) if self.absolute else self.rel(prd, tar, chw)


class GeometricH1Loss(nn.Module):
    """Weighted H1 loss on the sphere, losses.py:275-370: L2 and l (l + 1)-weighted norms of the spherical-harmonic
    coefficients of the error (``alpha`` balances the two), relative to the target's or absolute.  The transform is this
    package's HIP ``RealSHT``; its packed spectrum ``[L, M, BC]`` goes straight into one HIP pass that forms the per-degree
    sums in float64 (``ops.degree_power``), and the two weighted sums over channels and degrees are taken on that small
    ``[B, C, L]`` tensor.  The error ``prd - tar`` is formed in grid space: subtracting two spectra would cancel the
    error's leading digits once the prediction is close to the target.

    Under spatial parallelism (``comm.get_size("spatial") > 1``) the transform is a ``DistributedRealSHT``, ``forward``
    takes the ranks' own shards ``[B, C, H_loc, W_loc]`` and the per-sample ``[B, 2]`` partial sums of the rank's degrees and
    orders are all-reduced over the ``"spatial"`` group once per norm; the gradient of the all-reduce is the identity.

    As in the reference the third argument of ``forward`` is a per-(sample, channel) mask of the relative form --
    ``LossHandler`` passes its channel weights there (losses.py:168 with 364-368), which weights the relative norms."""

    def __init__(self, img_shape, p=2.0, size_average=False, reduction=True, absolute=False, squared=False, alpha=0.5):
        super().__init__()
        self.reduction, self.size_average = reduction, size_average
        self.absolute, self.squared, self.alpha = absolute, squared, alpha
        self.sharded = comm.get_size("spatial") > 1
        self.sht = real_sht(img_shape, "equiangular")
        h1_weights = torch.arange(self.sht.lmax).float()
        self.register_buffer("h1_weights", h1_weights * (h1_weights + 1))

    def norms_from_spectrum(self, c_packed, batch, l_off=0, m_off=0):
        """``[batch, 2]`` float64 (L2 norm squared, H1 seminorm squared) of the packed spectrum ``[L_loc, M_loc, batch * C]``
        of the degrees from ``l_off`` and the orders from ``m_off`` on: sums over channels, degrees and orders (m > 0
        twice).  They add up over the shards of a spectrum."""
        power = ops.degree_power(c_packed, l_off, m_off)                  # [batch * C, L_loc] float64
        nl = power.shape[1]
        power = power.reshape(batch, -1, nl)
        wl = self.h1_weights[l_off:l_off + nl].to(torch.float64)         # l (l + 1) of the GLOBAL degree, exact in fp32
        return torch.stack([power.sum(dim=(1, 2)), (power * wl).sum(dim=(1, 2))], dim=-1)

    def _norms(self, x):
        """(L2 norm squared, H1 seminorm squared) per sample: sums over channels, degrees and orders (m > 0 twice)."""
        n = x.size()[0]
        if x.is_cuda:
            x = ops._lowp(x)
            if not self.sharded and tuple(x.shape[-2:]) != (self.sht.nlat, self.sht.nlon):
                raise ValueError(f"expected [..., {self.sht.nlat}, {self.sht.nlon}], got {tuple(x.shape)}")
            c, l_off, m_off = self.sht.forward_packed_fields(x.reshape(n, -1, *x.shape[-2:]))
            sums = self.norms_from_spectrum(c, n, l_off, m_off)
            if self.sharded:
                sums = reduce_from_parallel_region(sums, "spatial")
            return sums[:, 0], sums[:, 1]
        c = torch.view_as_real(self.sht(x))
        c = c[..., 0] ** 2 + c[..., 1] ** 2
        norm2 = c[..., :, 0] + 2 * torch.sum(c[..., :, 1:], dim=-1)
        return norm2.reshape(n, -1).sum(dim=-1), (norm2 * self.h1_weights).reshape(n, -1).sum(dim=-1)

    def _combine(self, l2, h1):
        if self.squared:
            return self.alpha * l2 + (1 - self.alpha) * h1
        return self.alpha * torch.sqrt(l2) + (1 - self.alpha) * torch.sqrt(h1)

    def abs(self, prd, tar):
        all_norms = self._combine(*self._norms(prd - tar))
        if self.reduction:
            return torch.mean(all_norms) if self.size_average else torch.sum(all_norms)
        return all_norms

    def rel(self, prd, tar, mask=None):
        retval = self._combine(*self._norms(prd - tar)) / self._combine(*self._norms(tar))
        if mask is not None:
            retval = retval * mask
        if self.reduction:
            if self.size_average:
                return torch.mean(retval) if mask is None else torch.sum(retval) / torch.sum(mask)
            return torch.sum(retval)
        return retval

    def forward(self, prd, tar, mask=None):
        out = self.abs(prd, tar) if self.absolute else self.rel(prd, tar, mask)
        return out.float() if out.dtype == torch.float64 else out      # the degree sums are float64, the loss is fp32


class LossHandler(nn.Module):
    """losses.py:33-172 for the Lp family: parses ``params.loss`` ("l2", "geometric l2", "absolute squared geometric l2",
    "weighted ...", "pole-masked ...", "l1" ...), builds channel / multistep weights and calls the loss object.  Under
    spatial parallelism both families all-reduce their per-shard sums (CPU tensors of the H1 loss are gathered).  ``params`` is
    the trainer's parameter object (attribute access).

    A loss string with the word ``crps`` ("ensemble crps", "fair ensemble crps", "almost-fair ensemble crps"; not in the
    reference) selects ``ensemble.EnsembleCRPSLoss`` with ``params.ensemble_size`` members: ``prd`` is then ``[B * E, C', H, W]``
    (member fastest) for a ``tar`` ``[B, C', H, W]``.  "fair" is ``alpha = 1``, "almost-fair" ``alpha = params.crps_alpha`` (0.95);
    "weighted", "temp-std" and "pole-masked" act as for "l1"; "squared" is an error.  Sharded, the ``[B, C', 2]`` sums are all-reduced.
    With ``crps``, the word ``spectral`` selects ``ensemble.EnsembleSpectralCRPSLoss`` (the CRPS of the members' spherical-harmonic
    coefficients) alone and ``combined`` the sum ``EnsembleCRPSLoss + params.crps_spectral_weight * EnsembleSpectralCRPSLoss``.  The
    spectral term needs the whole sphere: a crop is an error, and so is "pole-masked" with "spectral" (with "combined" it acts on
    the grid-space term only).  Sharded, its ``[B, C', 2]`` sums are all-reduced over ``"spatial"`` once."""

    def __init__(self, params):
        super().__init__()
        self.rank = comm.get_rank("matmul")
        self.n_future = params.n_future
        self.img_shape = (params.img_shape_x, params.img_shape_y)
        self.crop_shape = (params.img_crop_shape_x, params.img_crop_shape_y)
        self.crop_offset = (params.img_crop_offset_x, params.img_crop_offset_y)
        self.loss_type = params.loss
        loss_type = set(self.loss_type.split())
        pole_mask = 1 if "pole-masked" in loss_type else 0
        if "weighted" in loss_type:
            if params.channel_weights == "auto":
                channel_weights = torch.ones(params.N_out_channels, dtype=torch.float32)
                for c, chn in enumerate(params.channel_names):
                    channel_weights[c] = 0.0 if chn in ["sst"] else 1.0
            else:
                channel_weights = torch.Tensor(params.channel_weights).float()
        else:
            channel_weights = torch.ones(params.N_out_channels, dtype=torch.float32)
        channel_weights = channel_weights.reshape(1, -1, 1, 1)
        channel_weights = channel_weights / torch.sum(channel_weights)
        absolute, squared = "absolute" in loss_type, "squared" in loss_type
        if "temp-std" in loss_type:
            eps = 1e-6
            global_stds = torch.from_numpy(np.load(params.global_stds_path)).reshape(1, -1, 1, 1)[:, params.out_channels]
            time_diff_stds = math.sqrt(params.dt) * torch.from_numpy(np.load(params.time_diff_stds_path)).reshape(1, -1, 1, 1)[:, params.out_channels]
            time_var_weights = global_stds / (time_diff_stds + eps)
            if squared:
                time_var_weights = time_var_weights ** 2
            channel_weights = channel_weights * time_var_weights
        self.register_buffer("channel_weights", channel_weights)
        rule = "legendre-gauss" if params.model_grid_type == "legendre_gauss" else "naive"
        common = dict(absolute=absolute, pole_mask=pole_mask)
        self.crps = "crps" in loss_type
        if self.crps:
            # the one loss with E predictions per target: prd [B * E, C', H, W] (member fastest) against tar [B, C', H, W]
            from .ensemble import EnsembleCRPSLoss          # ensemble.py imports this module
            if squared:
                raise ValueError(f"Unknown loss function: {self.loss_type} (the CRPS has no squared form)")
            members = getattr(params, "ensemble_size", None)
            if members is None:
                raise ValueError(f"loss {self.loss_type!r} needs params.ensemble_size, the number of members per target")
            alpha = float(getattr(params, "crps_alpha", 0.95)) if "almost-fair" in loss_type else 1.0 if "fair" in loss_type else 0.0
            # "spectral": the CRPS of the spherical-harmonic coefficients alone; "combined": the grid-space CRPS plus
            # params.crps_spectral_weight times the spectral one
            self.crps_spectral, self.crps_combined = "spectral" in loss_type, "combined" in loss_type
            self.spectral_obj = None
            if self.crps_spectral and self.crps_combined:
                raise ValueError(f"loss {self.loss_type!r}: 'spectral' and 'combined' exclude each other")
            if self.crps_spectral or self.crps_combined:
                from .ensemble import EnsembleSpectralCRPSLoss
                if tuple(self.crop_shape) != tuple(self.img_shape) or tuple(self.crop_offset) != (0, 0):
                    raise ValueError(f"loss {self.loss_type!r}: the spectral CRPS needs the whole sphere {self.img_shape}, got the crop "
                                     f"{self.crop_shape} at {self.crop_offset}")
                if self.crps_spectral and pole_mask:
                    raise ValueError(f"loss {self.loss_type!r}: 'pole-masked' has no meaning for the spectral CRPS")
                if self.crps_combined:
                    weight = getattr(params, "crps_spectral_weight", None)
                    if weight is None:
                        raise ValueError(f"loss {self.loss_type!r} needs params.crps_spectral_weight, the weight of the spectral term")
                    self.crps_spectral_weight = float(weight)
                self.spectral_obj = EnsembleSpectralCRPSLoss(self.img_shape, members, alpha=alpha,
                                                             grid="legendre-gauss" if rule == "legendre-gauss" else "equiangular")
            if self.crps_spectral:
                self.loss_obj = self.spectral_obj
            else:
                self.loss_obj = EnsembleCRPSLoss(self.img_shape, self.crop_shape, self.crop_offset, members, alpha=alpha,
                                                 pole_mask=pole_mask, quadrature_rule=rule)
        elif "l2" in loss_type:
            if "geometric" in loss_type:
                self.loss_obj = GeometricLpLoss(self.img_shape, self.crop_shape, self.crop_offset, p=2, squared=squared,
                                                quadrature_rule=rule, **common)
            else:
                self.loss_obj = GeometricLpLoss(self.img_shape, self.crop_shape, self.crop_offset, p=2, jacobian="flat", **common)
        elif "l1" in loss_type:
            if "geometric" in loss_type:
                self.loss_obj = GeometricLpLoss(self.img_shape, self.crop_shape, self.crop_offset, p=1, quadrature_rule=rule, **common)
            else:
                self.loss_obj = GeometricLpLoss(self.img_shape, self.crop_shape, self.crop_offset, p=1, jacobian="flat", **common)
        # losses.py:129-130 tests the two-word string against the SET of words, so the reference never reaches this branch
        # (it raises "Unknown loss function"); the evident intent is kept: "geometric h1" selects the H1 loss
        elif "geometric h1" in self.loss_type:
            self.loss_obj = GeometricH1Loss(self.img_shape, absolute=absolute, squared=squared)
        else:
            raise ValueError(f"Unknown loss function: {self.loss_type}")
        multistep_weight = torch.ones(self.n_future + 1, dtype=torch.float32) / float(self.n_future + 1)
        self.register_buffer("multistep_weight", multistep_weight.reshape(-1, 1, 1, 1))
        # host-side knowledge for the fused pass: the value of the channel weights if they are all equal (training / eval)
        cw_train = (channel_weights * self.multistep_weight).reshape(-1)
        cw_eval = channel_weights.reshape(-1)
        self._uniform = {True: float(cw_train[0]) if bool((cw_train == cw_train[0]).all()) else None,
                         False: float(cw_eval[0]) if bool((cw_eval == cw_eval[0]).all()) else None}
        # the Lp and CRPS terms are formed from sums that add up over shards; the H1 loss transforms and reduces by itself
        self.h1 = isinstance(self.loss_obj, GeometricH1Loss)
        self.do_gather_input = comm.get_size("spatial") > 1
        if self.do_gather_input:
            self.gather_shapes_h = compute_split_shapes(self.crop_shape[0], comm.get_size("h"))
            self.gather_shapes_w = compute_split_shapes(self.crop_shape[1], comm.get_size("w"))
        # this rank's latitude rows of the cropped grid (a w shard holds whole rows' weights: nothing to slice)
        h0, hs = shard_span(self.crop_shape[0], "h")
        self.shard_rows = slice(h0, h0 + hs)

    def _gather_input(self, x):
        xh = gather_from_parallel_region(x, -2, self.gather_shapes_h, "h")
        return gather_from_parallel_region(xh, -1, self.gather_shapes_w, "w")

    def is_distributed(self):
        return False

    def _from_shard(self, obj, prd, tar, chw, *rows):
        """``obj``'s term from this rank's shard: its sums (over ``rows`` of the latitude weights, where it takes them), which add
        up over shards, ONE all-reduce of them over ``"spatial"`` (its gradient is the identity), the loss.  Nothing is gathered."""
        sums = obj.sums(prd, tar, *rows)
        if self.do_gather_input:
            sums = reduce_from_parallel_region(sums, "spatial")
        return obj.from_sums(sums, chw)

    def forward(self, prd, tar, inp=None):
        chw = self.channel_weights
        chw = (chw * self.multistep_weight).reshape(1, -1) if self.training else chw.reshape(1, -1)
        if self.crps:
            if self.crps_spectral:
                return self._from_shard(self.spectral_obj, prd, tar, chw)
            loss = self._from_shard(self.loss_obj, prd, tar, chw, self.shard_rows)
            if self.crps_combined:
                loss = loss + self.crps_spectral_weight * self._from_shard(self.spectral_obj, prd, tar, chw)
            return loss
        if self.h1:
            # the H1 loss reduces over channels itself ([B] norms): its ``mask`` is per SAMPLE, the per-channel weights of
            # the Lp family do not apply (losses.py:331-345); passing them broadcast only for B == 1 or B == C.  Sharded, it
            # transforms its own shard and all-reduces [B, 2] sums; the transform has no CPU path, so CPU shards are gathered
            if self.do_gather_input and not (prd.is_cuda and tar.is_cuda):
                prd, tar = self._gather_input(prd), self._gather_input(tar)
            return self.loss_obj(prd, tar)
        if self.do_gather_input:
            if self.loss_obj.has_sums(prd, tar):
                return self._from_shard(self.loss_obj, prd, tar, chw, self.shard_rows)
            prd, tar = self._gather_input(prd), self._gather_input(tar)
        # unsharded, the loss object's own forward: the fused single pass where it applies (other bits than ``from_sums``)
        self.loss_obj.uniform_chw = self._uniform[bool(self.training)]
        return self.loss_obj(prd, tar, chw)
