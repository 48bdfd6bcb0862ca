"""SFNO blocks and network on MI355X -- the model seam.

Public interface of ``makani/models/networks/sfnonet.py``: ``SpectralFilterLayer`` (51-116),
``FourierNeuralOperatorBlock`` (119-267), ``SphericalFourierNeuralOperatorNet`` (270-640) and the
``FourierNeuralOperatorNet`` subclass (657-659) with the same constructor keywords and defaults (extra
keywords tolerated, line 311), the same ``state_dict`` keys and parameter annotations
(``is_shared_mp`` / ``sharded_dims_mp``), so the class is usable as a Makani ``nettype``
(``"makani_amd/sfnonet.py:SphericalFourierNeuralOperatorNet"``, model_registry.py:63-79) and reference
checkpoints load.  The bodies are this package's own: the block is assembled from a small table of
skip / activation choices and runs its tail through the fused HIP nodes (norm + GELU, the MLP on the
pixel-column engine, the skip convolution with the norm output as its epilogue addend).

Spatial model parallelism (``comm.get_size("spatial") > 1``) selects the distributed transforms and
``DistributedInstanceNorm2d`` where the reference does (sfnonet.py:375-377, 528-533).  Channel
("matmul") parallelism is outside the built hot path and raises; ``layer_norm`` runs on torch ops; the non-linear (attention)
filter runs on the HIP transforms with the ``mk_spec_cmlp_*`` channel MLP in between (``spectral_convolution.SpectralAttention``).
"""
import math
from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.utils.checkpoint import checkpoint

from . import comm, ops
from .distributed import DistributedInverseRealFFT2, DistributedInverseRealSHT, DistributedRealFFT2, DistributedRealSHT
from .layer_norm import DistributedInstanceNorm2d, DistributedLayerNorm
from .layers import (Conv1x1, DropPath, EncoderDecoder, InstanceNorm2d, InverseRealFFT2, MLP, RealFFT2, _engine_field,
                     _is_exact_gelu, _is_noop, conv_plus_instance_norm, encoder_head, spectral_skip_plus_instance_norm,
                     spectral_skip_supported)
from .sht import InverseRealSHT, RealSHT
from .spectral_convolution import FactorizedSpectralConv, SpectralAttention, SpectralConv

_ACTIVATIONS = {"relu": nn.ReLU, "gelu": nn.GELU, "silu": nn.SiLU}


def _local_shape(transform):
    """(latitudes, longitudes) this rank holds of a transform's grid."""
    if comm.get_size("spatial") > 1:
        return transform.lat_shapes[comm.get_rank("h")], transform.lon_shapes[comm.get_rank("w")]
    return transform.nlat, transform.nlon


def _make_skip(kind, embed_dim, gain):
    """Skip connection of the given kind -> (module or None, gain left for the main path).  A skip halves the gain of
    the path it is added to; the linear one is initialised with the halved gain (sfnonet.py:186-200, 223-234)."""
    if kind in ("none", None):
        return None, gain
    if kind == "identity":
        return nn.Identity(), gain / 2.0
    if kind == "linear":
        conv = Conv1x1(embed_dim, embed_dim, bias=False)
        nn.init.normal_(conv.weight, std=math.sqrt(gain / 2.0 / embed_dim))
        return conv, gain / 2.0
    raise ValueError(f"Unknown skip connection type {kind}")


class SpectralFilterLayer(nn.Module):
    def __init__(self, forward_transform, inverse_transform, embed_dim, filter_type="linear", operator_type="diagonal",
                 hidden_size_factor=1, factorization=None, rank=1.0, separable=False, complex_activation="real",
                 spectral_layers=1, bias=False, drop_rate=0.0, gain=1.0):
        super().__init__()
        common = dict(operator_type=operator_type, separable=separable, bias=bias, gain=gain)
        if filter_type == "non-linear":
            self.filter = SpectralAttention(forward_transform, inverse_transform, embed_dim, embed_dim, operator_type=operator_type,
                                            hidden_size_factor=hidden_size_factor, complex_activation=complex_activation,
                                            spectral_layers=spectral_layers, drop_rate=drop_rate, bias=bias, gain=gain)
        elif filter_type != "linear":
            raise NotImplementedError
        elif factorization is None:
            self.filter = SpectralConv(forward_transform, inverse_transform, embed_dim, embed_dim, **common)
        else:
            self.filter = FactorizedSpectralConv(forward_transform, inverse_transform, embed_dim, embed_dim, rank=rank,
                                                 factorization=factorization, **common)

    def forward(self, x, want_row_sums=False, **spectral):
        """``spectral``: ``premix`` / ``spectrum_residual`` of ``SpectralConv.forward``, for a filter that ``takes_spectral_mix()``."""
        spectral = {k: v for k, v in spectral.items() if v}
        if spectral:
            out = self.filter(x, want_row_sums=want_row_sums, **spectral)
            return out
        if want_row_sums and isinstance(self.filter, SpectralConv) and type(self.filter).forward is SpectralConv.forward:
            return self.filter(x, want_row_sums=True)
        if want_row_sums and isinstance(self.filter, SpectralAttention) and type(self.filter).forward is SpectralAttention.forward:
            return self.filter(x, want_row_sums=True)     # its fused path has the inverse FFT's statistics, the other None
        out = self.filter(x)
        return (out[0], out[1], None) if want_row_sums else out

    def takes_spectral_mix(self):
        return isinstance(self.filter, SpectralConv) and self.filter.takes_spectral_mix()


class FourierNeuralOperatorBlock(nn.Module):
    """filter -> norm0 (+ inner skip) -> activation -> MLP -> norm1 -> drop path (+ outer skip) (-> activation)."""

    def __init__(self, forward_transform, inverse_transform, embed_dim, filter_type="linear", operator_type="diagonal",
                 mlp_ratio=2.0, mlp_drop_rate=0.0, path_drop_rate=0.0, act_layer=nn.GELU,
                 norm_layer=(nn.Identity, nn.Identity), rank=1.0, factorization=None, separable=False,
                 inner_skip="linear", outer_skip=None, use_mlp=False, comm_feature_inp_name=None,
                 comm_feature_hidden_name=None, complex_activation="real", spectral_layers=1, bias=False,
                 final_activation=False, checkpointing=0):
        super().__init__()
        self.input_shape_loc = _local_shape(forward_transform)
        self.output_shape_loc = _local_shape(inverse_transform)
        has_act = act_layer != nn.Identity

        # registration order = the reference's (state_dict order): norm0, inner_skip, filter, norm1, outer_skip, mlp
        self.norm0 = norm_layer[0]()
        skip, filter_gain = _make_skip(inner_skip, embed_dim, 2.0 if has_act else 1.0)
        if skip is not None:
            self.inner_skip = skip
        self.filter = SpectralFilterLayer(forward_transform, inverse_transform, embed_dim, filter_type, operator_type,
                                          hidden_size_factor=mlp_ratio, factorization=factorization, rank=rank,
                                          separable=separable, complex_activation=complex_activation,
                                          spectral_layers=spectral_layers, bias=bias, drop_rate=path_drop_rate,
                                          gain=filter_gain)
        self.act_layer0 = act_layer()
        self.norm1 = norm_layer[1]()
        skip, mlp_gain = _make_skip(outer_skip, embed_dim, 2.0 if (final_activation and has_act) else 1.0)
        if skip is not None:
            self.outer_skip = skip
        if use_mlp == True:  # noqa: E712  (1.0 selects the MLP, a non-empty string does not: as upstream)
            self.mlp = MLP(in_features=embed_dim, hidden_features=int(embed_dim * mlp_ratio), act_layer=act_layer,
                           drop_rate=mlp_drop_rate, drop_type="features", comm_inp_name=comm_feature_inp_name,
                           comm_hidden_name=comm_feature_hidden_name, checkpointing=checkpointing, gain=mlp_gain)
        self.drop_path = DropPath(path_drop_rate) if path_drop_rate > 0.0 else nn.Identity()
        if final_activation:
            self.act_layer1 = act_layer()

    @staticmethod
    def _removes_channel_constants(norm):
        """An instance norm on the field's own statistics removes any per-channel constant added in front of it."""
        return (isinstance(norm, (nn.InstanceNorm2d, DistributedInstanceNorm2d))
                and not getattr(norm, "track_running_stats", False))

    def _spectral_outer_skip(self, x):
        """The outer skip convolution may run as a channel mix of the block's input spectrum: its input is a synthesis of that
        spectrum onto a LARGER grid (on a smaller one the convolution on the grid is the cheaper side) and the block's tail is
        the one ``conv_plus_instance_norm`` fuses."""
        outer = getattr(self, "outer_skip", None)
        return (outer is not None and hasattr(self, "mlp") and not hasattr(self, "inner_skip")
                and isinstance(self.filter, SpectralFilterLayer) and self.filter.takes_spectral_mix()
                and self.filter.filter.scale_residual
                and self.output_shape_loc[0] * self.output_shape_loc[1] > self.input_shape_loc[0] * self.input_shape_loc[1]
                and isinstance(self.norm1, (InstanceNorm2d, DistributedInstanceNorm2d))
                and isinstance(self.drop_path, nn.Identity) and not hasattr(self, "act_layer1")
                and getattr(self.mlp, "checkpointing", 0) < 2 and spectral_skip_supported(outer, x))

    def forward(self, x, premix=None):
        """``premix``: a bias-free ``Conv1x1`` the caller left out in front of the block (the encoder's last); the filter applies
        it to the spectrum.  Only for a block whose filter ``takes_spectral_mix()`` and whose residual is a scaled one."""
        inner = getattr(self, "inner_skip", None)
        hip_norm0 = isinstance(self.norm0, (InstanceNorm2d, DistributedInstanceNorm2d)) \
            and not getattr(self.norm0, "track_running_stats", False)
        sums0 = None
        batch, in_dtype = x.shape[0], x.dtype
        spec_skip = self._spectral_outer_skip(x)
        if hip_norm0 and isinstance(self.filter, SpectralFilterLayer):
            # norm0's statistics come out of the inverse FFT
            x, residual, sums0 = self.filter(x, want_row_sums=True, premix=premix, spectrum_residual=spec_skip)
        elif premix is not None or spec_skip:
            x, residual = self.filter(x, premix=premix, spectrum_residual=spec_skip)
        else:
            x, residual = self.filter(x)
        ln_dtype = None
        if x.is_cuda and (x.dtype == torch.bfloat16 or (torch.is_autocast_enabled()
                                                        and torch.get_autocast_dtype("cuda") == torch.bfloat16)):
            ln_dtype = torch.bfloat16     # bf16-engine step: the layer norms hand the MLP / skip convolution the engine's field
        if isinstance(self.norm0, DistributedLayerNorm):
            # channel layer norm (+ GELU) on one HIP pass.  Fused, the result is rounded once to the dtype the convolution behind
            # it takes; with an inner skip in between, an engine step rounds the norm's result to bf16 BEFORE the skip add and
            # the activation (one bf16 rounding more than autocast makes there, which keeps both in fp32)
            fuse = inner is None and _is_exact_gelu(self.act_layer0)
            x = self.norm0(x, fuse_gelu=fuse, out_dtype=ln_dtype)
            if not fuse:
                if inner is not None:
                    x = x + inner(residual)
                x = self.act_layer0(x)
        elif inner is None and hip_norm0 and _is_exact_gelu(self.act_layer0):
            x = self.norm0(x, fuse_gelu=True, row_sums=sums0)  # norm0 + GELU: (no statistics pass,) one apply pass
        elif hip_norm0:
            x = self.norm0(x, row_sums=sums0)
            if inner is not None:
                x = x + inner(residual)
            x = self.act_layer0(x)
        else:
            x = self.norm0(x)
            if inner is not None:
                x = x + inner(residual)
            x = self.act_layer0(x)
        sums = None
        if hasattr(self, "mlp"):
            if isinstance(self.norm1, (InstanceNorm2d, DistributedInstanceNorm2d)):
                # the last GEMM of the MLP hands over the row sums of its output: norm1 needs no statistics pass
                x, sums = self.mlp(x, skip_last_bias=self._removes_channel_constants(self.norm1), want_row_sums=True)
            else:
                x = self.mlp(x, skip_last_bias=self._removes_channel_constants(self.norm1))
        outer = getattr(self, "outer_skip", None)
        if spec_skip:
            # outer skip in the spectral domain: isht(W c) instead of W isht(c), then norm1's apply pass and the add in one pass
            y = spectral_skip_plus_instance_norm(outer, self.filter.filter, residual, x, sums, self.norm1)
            if y is not None:
                return y
            residual = self.filter.filter.residual_from_spectrum(residual, batch, in_dtype)
        if sums is not None and isinstance(self.drop_path, nn.Identity) and not hasattr(self, "act_layer1"):
            # norm1 + outer skip: the norm's apply pass rides in the epilogue of the skip convolution
            y = conv_plus_instance_norm(outer, residual, x, sums, self.norm1)
            if y is not None:
                return y
        if isinstance(self.norm1, DistributedLayerNorm):
            x = self.drop_path(self.norm1(x, out_dtype=ln_dtype))
        else:
            x = self.drop_path(self.norm1(x, row_sums=sums) if sums is not None else self.norm1(x))
        if isinstance(outer, Conv1x1):
            x = outer(residual, addend=x)                     # skip add folded into the GEMM epilogue
        elif outer is not None:
            x = x + outer(residual)
        if hasattr(self, "act_layer1"):
            x = self.act_layer1(x)
        return x


class SphericalFourierNeuralOperatorNet(nn.Module):
    """SFNO (Bonev et al.) with the spectral path in hand-written HIP."""

    def __init__(self, spectral_transform="sht", model_grid_type="equiangular", sht_grid_type="legendre-gauss",
                 filter_type="linear", operator_type="dhconv", inp_shape=(721, 1440), out_shape=(721, 1440),
                 scale_factor=8, inp_chans=2, out_chans=2, embed_dim=32, num_layers=4, repeat_layers=1, use_mlp=True,
                 mlp_ratio=2.0, encoder_ratio=1, decoder_ratio=1, activation_function="gelu", encoder_layers=1,
                 pos_embed="none", pos_drop_rate=0.0, path_drop_rate=0.0, mlp_drop_rate=0.0,
                 normalization_layer="instance_norm", max_modes=None, hard_thresholding_fraction=1.0, big_skip=True,
                 rank=1.0, factorization=None, separable=False, complex_activation="real", spectral_layers=3,
                 bias=False, checkpointing=0, **kwargs):
        super().__init__()
        if comm.get_size("matmul") > 1:
            raise NotImplementedError("channel ('matmul', fin/fout) parallelism is outside the built hot path")
        if activation_function not in _ACTIVATIONS:
            raise ValueError(f"Unknown activation function {activation_function}")
        act = _ACTIVATIONS[activation_function]

        self.inp_shape, self.out_shape = tuple(inp_shape), tuple(out_shape)
        self.inp_chans, self.out_chans, self.embed_dim = inp_chans, out_chans, embed_dim
        self.repeat_layers, self.big_skip, self.checkpointing = repeat_layers, big_skip, checkpointing
        self.h, self.w = int(self.inp_shape[0] // scale_factor), int(self.inp_shape[1] // scale_factor)

        self._init_spectral_transforms(spectral_transform, model_grid_type, sht_grid_type, hard_thresholding_fraction, max_modes)

        self.encoder = EncoderDecoder(num_layers=encoder_layers, input_dim=inp_chans, output_dim=embed_dim,
                                      hidden_dim=int(encoder_ratio * embed_dim), act_layer=act, input_format="nchw")
        self.pos_drop = nn.Dropout(p=pos_drop_rate) if pos_drop_rate > 0.0 else nn.Identity()

        norm = self._norm_factory(normalization_layer, embed_dim)
        drop_rates = torch.linspace(0, path_drop_rate, num_layers).tolist()
        self.blocks = nn.ModuleList()
        for i, drop in enumerate(drop_rates):
            self.blocks.append(FourierNeuralOperatorBlock(
                self.trans_down if i == 0 else self.trans,
                self.itrans_up if i == num_layers - 1 else self.itrans,
                embed_dim, filter_type=filter_type, operator_type=operator_type, mlp_ratio=mlp_ratio,
                mlp_drop_rate=mlp_drop_rate, path_drop_rate=drop, act_layer=act, norm_layer=(norm, norm),
                inner_skip="none", outer_skip="linear", use_mlp=use_mlp, comm_feature_inp_name="fin",
                comm_feature_hidden_name="fout", rank=rank, factorization=factorization, separable=separable,
                complex_activation=complex_activation, spectral_layers=spectral_layers, bias=bias,
                checkpointing=checkpointing))

        self.decoder = EncoderDecoder(num_layers=encoder_layers, input_dim=embed_dim, output_dim=out_chans,
                                      hidden_dim=int(decoder_ratio * embed_dim), act_layer=act,
                                      gain=0.5 if big_skip else 1.0, input_format="nchw")
        if big_skip:
            self.residual_transform = Conv1x1(inp_chans, out_chans, bias=False)
            self.residual_transform.weight.is_shared_mp = ["spatial"]
            self.residual_transform.weight.sharded_dims_mp = [None, None, None, None]
            nn.init.normal_(self.residual_transform.weight, mean=0.0, std=math.sqrt(0.5 / inp_chans))
        self._init_pos_embed(pos_embed)

    # ------------------------------------------------------------------ construction helpers
    @staticmethod
    def _norm_factory(kind, embed_dim):
        if kind == "instance_norm":
            if comm.get_size("spatial") > 1:
                return partial(DistributedInstanceNorm2d, num_features=embed_dim, eps=1e-6, affine=True)
            return partial(InstanceNorm2d, num_features=embed_dim, eps=1e-6, affine=True, track_running_stats=False)
        if kind == "none":
            return nn.Identity
        if kind == "layer_norm":       # sfnonet.py:371-373: channel-wise layer norm per grid point (HIP channel-norm passes on the GPU)
            return partial(DistributedLayerNorm, normalized_shape=(embed_dim), elementwise_affine=True, eps=1e-6)
        raise NotImplementedError(f"Error, normalization {kind} not implemented.")

    def _init_spectral_transforms(self, spectral_transform="sht", model_grid_type="equiangular",
                                  sht_grid_type="legendre-gauss", hard_thresholding_fraction=1.0, max_modes=None):
        if max_modes is not None:
            modes = dict(lmax=max_modes[0], mmax=max_modes[1])
        else:
            modes = dict(lmax=int(self.h * hard_thresholding_fraction),
                         mmax=int((self.w // 2 + 1) * hard_thresholding_fraction))
        distributed = comm.get_size("spatial") > 1
        if spectral_transform == "sht":
            fwd, inv = (DistributedRealSHT, DistributedInverseRealSHT) if distributed else (RealSHT, InverseRealSHT)
            outer, inner = dict(grid=model_grid_type, **modes), dict(grid=sht_grid_type, **modes)
        elif spectral_transform == "fft":
            fwd, inv = (DistributedRealFFT2, DistributedInverseRealFFT2) if distributed else (RealFFT2, InverseRealFFT2)
            outer = inner = modes
        else:
            raise ValueError("Unknown spectral transform")
        # analysis / synthesis on the model grid (first / last block) and on the scaled internal grid; fp32 tables
        self.trans_down = fwd(*self.inp_shape, **outer).float()
        self.itrans_up = inv(*self.out_shape, **outer).float()
        self.trans = fwd(self.h, self.w, **inner).float()
        self.itrans = inv(self.h, self.w, **inner).float()
        self.inp_shape_loc = _local_shape(self.trans_down)
        self.out_shape_loc = _local_shape(self.itrans_up)
        self.h_loc, self.w_loc = _local_shape(self.itrans)

    def _init_pos_embed(self, kind):
        """Learned position embedding added behind the encoder (sfnonet.py:469-501): a grid field (``direct``) or real and
        imaginary spectral coefficients synthesised to the grid each step (``frequency``)."""
        if kind in ("none", "None", None):
            return
        if kind == "direct":
            self.pos_embed = nn.Parameter(torch.zeros(1, self.embed_dim, *self.inp_shape_loc))
            nn.init.trunc_normal_(self.pos_embed, std=0.02)
        elif kind == "frequency":
            if comm.get_size("spatial") > 1:
                lloc, mloc = self.itrans_up.l_shapes[comm.get_rank("h")], self.itrans_up.m_shapes[comm.get_rank("w")]
            else:
                lloc, mloc = self.itrans_up.lmax, self.itrans_up.mmax
            re = nn.Parameter(torch.tril(torch.randn(1, self.embed_dim, lloc, mloc), diagonal=0))
            im = nn.Parameter(torch.tril(torch.randn(1, self.embed_dim, lloc, mloc - 1), diagonal=-1))   # no m = 0 column
            for t in (re, im):
                nn.init.trunc_normal_(t, std=0.02)
            self.pos_embed = nn.ParameterList([re, im])
        else:
            raise ValueError("Unknown position embedding type")
        self.pos_embed.type = kind
        self.pos_embed.is_shared_mp = []
        self.pos_embed.sharded_dims_mp = [None, None, "h", "w"]

    def no_weight_decay(self):
        return {"pos_embed", "cls_token"}

    # ------------------------------------------------------------------ forward
    def _position_field(self, like):
        if self.pos_embed.type == "direct":
            return self.pos_embed
        re, im = self.pos_embed
        coeffs = torch.complex(re, F.pad(im, (1, 0)))
        with torch.autocast(device_type=like.device.type, enabled=False):
            return self.itrans_up(coeffs)

    def _big_skip_input(self, x):
        if self.out_shape == self.inp_shape:
            return x
        with torch.autocast(device_type=x.device.type, enabled=False):     # resample the input to the output grid
            return self.itrans_up(self.trans_down(x.float()).contiguous()).to(x.dtype)

    def _forward_features(self, x, premix=None):
        for _ in range(self.repeat_layers):
            for i, blk in enumerate(self.blocks):
                if i == 0 and premix is not None:
                    x = blk(x, premix=premix)
                else:
                    x = checkpoint(blk, x, use_reentrant=False) if self.checkpointing >= 3 else blk(x)
        return x

    def _spectral_encoder(self, x):
        """``(h, conv)`` when the encoder's last convolution can run behind block 0's analysis instead of in front of it
        (``sht(W x) = W sht(x)``): its output has no other consumer (no position embedding, no dropout, block 0's residual is
        synthesised from the spectrum, the big skip takes the raw input) -- else None."""
        blk = self.blocks[0] if len(self.blocks) else None
        if (blk is None or hasattr(self, "pos_embed") or not _is_noop(self.pos_drop) or self.checkpointing != 0
                or self.repeat_layers != 1 or not blk.filter.takes_spectral_mix() or not blk.filter.filter.scale_residual
                or hasattr(blk, "inner_skip")):
            return None
        return encoder_head(self.encoder, x)

    def _engine_arena(self, x):
        """The per-step arena of the pointwise stack (``ops.EngineArena``) when this call runs on the bf16 engine, else None."""
        from .layers import Conv1x1
        if not (x.is_cuda and x.dim() == 4 and ops._knob("MK_ENGINE_ARENA", "1") != "0"):
            return None
        if not (x.dtype == torch.bfloat16 or (torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16)):
            return None
        cached = self.__dict__.get("_arena")                # (convolutions, their weight pointers, arena): plain attribute, not state
        if cached is None:
            convs = [m for m in self.modules() if isinstance(m, Conv1x1)]
        else:
            convs = cached[0]
        ptrs = [m.weight.data_ptr() for m in convs]
        if cached is None or cached[1] != ptrs:             # first call, or a parameter's storage moved (.to(), .data = ...)
            cached = (convs, ptrs, ops.EngineArena([m.weight2d() for m in convs if m.weight.is_cuda]))
            self.__dict__["_arena"] = cached
        return cached[2] if cached[2].n else None

    def forward(self, x):
        arena = self._engine_arena(x)
        if arena is None:
            return self._forward(x)
        with arena.scope():       # every weight image of the step in one launch, every weight-gradient buffer in one fill
            return self._forward(x)

    def _forward(self, x):
        if self.big_skip and self.out_shape == self.inp_shape and x.dtype == torch.float32 and x.dim() == 4:
            # the input feeds the encoder AND the big skip: cast it for the bf16 engine once, not once per consumer
            x3 = _engine_field(x)
            if x3 is not None and x3.dtype != x.dtype:
                x = x3.view(x.shape)
        skip_in = self._big_skip_input(x) if self.big_skip else None
        head = self._spectral_encoder(x)
        if head is not None:
            x = self._forward_features(head[0], premix=head[1])       # the encoder's last convolution rides on block 0's spectrum
        else:
            x = checkpoint(self.encoder, x, use_reentrant=False) if self.checkpointing >= 1 else self.encoder(x)
            if hasattr(self, "pos_embed"):
                x = x + self._position_field(x)
            x = self._forward_features(self.pos_drop(x))
        x = checkpoint(self.decoder, x, use_reentrant=False) if self.checkpointing >= 1 else self.decoder(x)
        if skip_in is not None:
            x = self.residual_transform(skip_in, addend=x)     # big skip folded into the GEMM epilogue
        return x


class FourierNeuralOperatorNet(SphericalFourierNeuralOperatorNet):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, spectral_transform="fft", **kwargs)
