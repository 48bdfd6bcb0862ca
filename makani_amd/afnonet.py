"""The AFNO network (``nettype: "AFNO"``, networks/afnonet_v2.py): ``AFNO2D``, ``Block`` and
``AdaptiveFourierNeuralOperatorNet`` with the reference's constructor signatures, attributes and ``state_dict`` keys.

The filter's arithmetic -- per channel block a complex two-layer MLP on every Fourier coefficient, ReLU on both components after
the first product, soft-shrink on both after the second -- runs on the HIP planar transforms (``RealFFT2.forward_packed`` /
``InverseRealFFT2.inverse_packed``) with the ``mk_spec_bdmlp_*`` block-diagonal kernels of the bf16x3 engine in between
(``ops.spec_block_mlp``); the real bias and the residual are one ``mk_affine_add`` pass.  ``MK_AFNO=torch``, a transform pair that is
not ``hip_ready`` (``MK_PLANAR_FFT`` defaults to ``torch``) and every case the kernels do not take run
``AFNO2D._forward_torch``, the reference's formulation in torch ops (timings: DESIGN section 22).

Out of scope:

* the channels-last ``AFNOv1`` (networks/afnonet.py) is its own module, ``makani_amd/afnonet_v1.py``, on these kernels plus two
  layout passes, biases in the block MLP and a latitude DFT table over its frequency window;
* ``DistributedAFNO2Dv2`` / ``DistributedPatchEmbed``: the reference's are broken (``distributed_rfft2`` is undefined), so
  spatial or matmul group sizes above 1 raise ``NotImplementedError``; data parallelism works as for any module;
* the engines' shape limits: 768 -> 3072 and the 1664-wide patch and head GEMMs take whatever path ``Conv1x1`` / ``MLP`` give
  them today.
"""
from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F

try:
    from . import comm, ops
except ImportError:     # loaded by file path (the reference's registry: ``nettype: ".../makani_amd/afnonet.py:Name"``), no package
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from makani_amd import comm, ops
from makani_amd.layers import MLP, Conv1x1, DropPath, InstanceNorm2d, InverseRealFFT2, LayerNorm, PatchEmbed, RealFFT2
from makani_amd.spectral_convolution import ComplexReLU


def _mul_real(a, b):
    """afnonet_v2.py:34-38: the complex block product as one real einsum over the (re, im) axes."""
    tmp = torch.einsum("bkixys,kior->srbkoxy", a, b)
    return torch.stack([tmp[0, 0, ...] - tmp[1, 1, ...], tmp[1, 0, ...] + tmp[0, 1, ...]], dim=-1)


def _mul_complex(a, b):
    """afnonet_v2.py:41-47: the same product as a complex einsum."""
    return torch.view_as_real(torch.einsum("bkixy,kio->bkoxy", torch.view_as_complex(a), torch.view_as_complex(b)))


class _ResidualBias(torch.autograd.Function):
    """``r + x + b[c]`` on ``[B, C, H, W]`` fields of one dtype in one ``mk_affine_add`` pass (affine (1, b[c])); the bias
    gradient is the HIP row sums of the incoming gradient added over the batch."""

    @staticmethod
    def forward(ctx, r, x, b):
        B, C = x.shape[0], x.shape[1]
        affine = torch.stack([torch.ones(C, dtype=torch.float32, device=x.device), b.detach().float().reshape(C)], dim=1)
        ctx.meta = (b.shape, b.dtype)
        return ops.affine_add(r, x, affine.repeat(B, 1).contiguous())

    @staticmethod
    def backward(ctx, g):
        shape, dtype = ctx.meta
        gb = None
        if ctx.needs_input_grad[2]:
            g = g.contiguous()
            B, C = g.shape[0], g.shape[1]
            gb = ops.row_sums(g.view(B, C, -1)).view(B, C).sum(0).to(dtype).view(shape)
        return g, g, gb


class AFNO2D(nn.Module):
    """afnonet_v2.py:50-112.  Parameters ``w1 [nb, bs, bs * f, 2]``, ``b1 [1, C, 1, 1]``, ``w2 [nb, bs * f, bs, 2]`` (scale 0.02).

    The fused path (autocast off, as in ``SpectralAttention``): ``forward_packed`` -> ``ops.spec_block_mlp`` ->
    ``inverse_packed`` -> ``irfft + b1[c] + x``.  The transform pair is built per ``(H, W)`` on first use: ``lmax = H,
    mmax = W // 2 + 1`` when nothing is cut, else ``lmax = 2 * kept_H, mmax = kept_W`` -- that pair's first and last ``kept_H``
    latitude frequencies are the reference's two slices, and its implicit zero padding is the reference's ``zeros`` buffer
    (``softshrink(0) = 0``).  It applies to CUDA fp32 / bf16 4-D inputs with even ``bs`` and ``bs * f`` and even ``W``, on the
    bf16x3 engine, where the pair's ``hip_ready`` holds (``MK_PLANAR_FFT=hip``) and ``MK_AFNO`` (``hip`` | ``torch``, read and
    validated on every call) is not ``torch``.  Everything else takes ``_forward_torch``.

    ``use_complex_kernels`` selects the einsum of the torch formulation only; the fused path is fp32-accurate for both.  (Under
    autocast the reference's real einsum would run in bf16; the fused path does not follow it there.)  bf16 inputs get bf16
    output rows straight from the inverse FFT where ``ops.irfft_bf16_rows`` says so, else the fp32 rows are cast.  Grids whose
    ``H * W`` is no multiple of 8 (not the production 90 x 180) add bias and residual with torch adds behind the HIP transforms.
    """

    def __init__(self, hidden_size, num_blocks=8, sparsity_threshold=0.0, hard_thresholding_fraction=1, hidden_size_factor=1,
                 use_complex_kernels=False):
        super().__init__()
        assert hidden_size % num_blocks == 0, f"hidden_size {hidden_size} should be divisble by num_blocks {num_blocks}"
        self.hidden_size = hidden_size
        self.sparsity_threshold = sparsity_threshold
        self.num_blocks = num_blocks
        self.block_size = self.hidden_size // self.num_blocks
        self.hard_thresholding_fraction = hard_thresholding_fraction
        self.hidden_size_factor = hidden_size_factor
        self.scale = 0.02
        self.mult_handle = _mul_complex if use_complex_kernels else _mul_real
        self.w1 = nn.Parameter(self.scale * torch.randn(self.num_blocks, self.block_size, self.block_size * self.hidden_size_factor, 2))
        self.b1 = nn.Parameter(self.scale * torch.randn(1, self.num_blocks * self.block_size, 1, 1))
        self.w2 = nn.Parameter(self.scale * torch.randn(self.num_blocks, self.block_size * self.hidden_size_factor, self.block_size, 2))
        self.act = ComplexReLU(negative_slope=0.0, mode="cartesian")
        self._pairs = {}

    def _kept_modes(self, H, W):
        total_h, total_w = H // 2 + 1, W // 2 + 1
        return total_h, int(total_h * self.hard_thresholding_fraction), int(total_w * self.hard_thresholding_fraction)

    def _pair(self, H, W, device):
        key = (H, W, device)
        if key not in self._pairs:
            total_h, kept_h, kept_w = self._kept_modes(H, W)
            lmax = H if kept_h == total_h else 2 * kept_h
            self._pairs[key] = (RealFFT2(H, W, lmax, kept_w).to(device), InverseRealFFT2(H, W, lmax, kept_w).to(device))
        return self._pairs[key]

    def _takes_fused(self, x):
        hip = ops.afno_hip()        # validates the knob on every call
        if not (hip and x.is_cuda and x.dim() == 4 and x.dtype in (torch.float32, torch.bfloat16)):
            return False
        H, W = x.shape[-2], x.shape[-1]
        _, kept_h, kept_w = self._kept_modes(H, W)
        hb = self.block_size * self.hidden_size_factor
        if self.block_size % 2 or hb % 2 or W % 2 or kept_h < 1 or kept_w < 1 or ops.SPECTRAL_GEMM != "bf16x3":
            return False
        if x.shape[1] != self.hidden_size or self.w1.dtype != torch.float32 or not self.w1.is_cuda:
            return False
        ft, it = self._pair(H, W, x.device)
        return ft.hip_ready(x) and it.hip_ready(x)

    def _forward_fused(self, x):
        B, C, H, W = x.shape
        ft, it = self._pair(H, W, x.device)
        xin = x.contiguous()
        c = ft.forward_packed(xin.view(B * C, H, W))
        y = ops.spec_block_mlp(c, self.w1, self.w2, B, self.num_blocks, self.sparsity_threshold)
        r = it.inverse_packed(y, x.dtype).view(B, C, H, W)
        if ops.pointwise_supported(xin):
            return _ResidualBias.apply(r, xin, self.b1)
        return r + self.b1.to(r.dtype) + xin        # H * W no multiple of 8: mk_affine_add's rows would not be 16-byte aligned

    def _forward_torch(self, x):
        bias = x
        dtype = x.dtype
        x = x.float()
        B, C, H, W = x.shape
        total_modes_H, kept_modes_H, kept_modes_W = self._kept_modes(H, W)
        x = torch.fft.rfft2(x, dim=(-2, -1), norm="ortho")
        x = x.view(B, self.num_blocks, self.block_size, H, W // 2 + 1)
        x = torch.view_as_real(x)
        x_fft = torch.zeros(x.shape, device=x.device)
        if kept_modes_H == total_modes_H:
            oac = torch.view_as_complex(self.mult_handle(x[:, :, :, :, :kept_modes_W, :], self.w1))
            oa = torch.view_as_real(self.act(oac))
            x_fft[:, :, :, :, :kept_modes_W, :] = self.mult_handle(oa, self.w2)
        else:
            olc = torch.view_as_complex(self.mult_handle(x[:, :, :, :kept_modes_H, :kept_modes_W, :], self.w1))
            ohc = torch.view_as_complex(self.mult_handle(x[:, :, :, -kept_modes_H:, :kept_modes_W, :], self.w1))
            ol = torch.view_as_real(self.act(olc))
            oh = torch.view_as_real(self.act(ohc))
            x_fft[:, :, :, :kept_modes_H, :kept_modes_W, :] = self.mult_handle(ol, self.w2)
            x_fft[:, :, :, -kept_modes_H:, :kept_modes_W, :] = self.mult_handle(oh, self.w2)
        x = F.softshrink(x_fft, lambd=self.sparsity_threshold)
        x = torch.view_as_complex(x)
        x = x.reshape(B, C, H, W // 2 + 1)
        x = torch.fft.irfft2(x, s=(H, W), dim=(-2, -1), norm="ortho")
        x = x.type(dtype)
        return x + self.b1 + bias

    def forward(self, x):
        if self._takes_fused(x):
            with torch.autocast(device_type="cuda", enabled=False):
                return self._forward_fused(x)
        return self._forward_torch(x)


class Block(nn.Module):
    """afnonet_v2.py:115-187.  ``norm_layer`` is a factory without arguments; ``skip_layer`` a ``Conv1x1`` (``"linear"``) or
    ``nn.Identity``; ``mlp`` this package's ``layers.MLP``."""

    def __init__(self, h, w, dim, mlp_ratio=4.0, drop=0.0, drop_path=0.0, act_layer=nn.GELU, norm_layer=nn.LayerNorm, num_blocks=8,
                 sparsity_threshold=0.01, hard_thresholding_fraction=1.0, use_complex_kernels=True, skip_fno="linear",
                 nested_skip_fno=True, checkpointing=False, verbose=True):
        super().__init__()
        self.norm1 = norm_layer()
        if skip_fno is None:
            if verbose:
                print("Using no skip connection around FNO.")
        elif skip_fno == "linear":
            self.skip_layer = Conv1x1(dim, dim)
            if verbose:
                print("Using Linear skip connection around FNO.")
        elif skip_fno == "identity":
            self.skip_layer = nn.Identity()
            if verbose:
                print("Using Identity skip connection around FNO.")
        elif verbose:
            print(f"Got skip_fno={skip_fno}, not using any skip around FNO -- use linear or identity to change this.")
        self.skip_fno = skip_fno
        self.nested_skip_fno = nested_skip_fno
        self.filter = AFNO2D(dim, num_blocks, sparsity_threshold, hard_thresholding_fraction, use_complex_kernels=use_complex_kernels)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.norm2 = norm_layer()
        mlp_hidden_dim = int(dim * mlp_ratio)
        self.mlp = MLP(in_features=dim, hidden_features=mlp_hidden_dim, act_layer=act_layer, drop_rate=drop, checkpointing=checkpointing)

    def forward(self, x):
        residual = x
        x = self.norm1(x)
        x = self.filter(x)
        if self.skip_fno is not None:
            x = x + self.skip_layer(residual)
            if not self.nested_skip_fno:
                residual = x
        x = self.norm2(x)
        x = self.mlp(x)
        x = self.drop_path(x)
        x = x + residual
        return x


class AdaptiveFourierNeuralOperatorNet(nn.Module):
    """afnonet_v2.py:190-314: patch embedding, position embedding, ``num_layers`` blocks, a 1x1 head and the rearrangement of
    its ``out_chans * p0 * p1`` channels back onto the full grid.  All keywords and defaults of the reference; further
    keywords are tolerated like there.  ``instance_norm`` is this package's ``layers.InstanceNorm2d`` (HIP passes),
    ``layer_norm`` is ``layers.LayerNorm((h, w))``: the reference's ``nn.LayerNorm`` over the rows of ``h w`` grid points of each
    (sample, channel), on the ``mk_token_layernorm_*`` kernels under ``MK_TOKEN_NORM=hip``."""

    def __init__(self, inp_shape=(720, 1440), patch_size=(16, 16), inp_chans=2, out_chans=2, embed_dim=768, num_layers=12,
                 mlp_ratio=4.0, drop_rate=0.0, drop_path_rate=0.0, num_blocks=16, sparsity_threshold=0.01,
                 normalization_layer="instance_norm", skip_fno="linear", nested_skip_fno=True, hard_thresholding_fraction=1.0,
                 checkpointing=False, use_complex_kernels=True, verbose=False, **kwargs):
        super().__init__()
        if comm.get_size("h") * comm.get_size("w") > 1 or comm.get_size("fin") * comm.get_size("fout") > 1:
            raise NotImplementedError("AFNO runs data parallel only: no spatial or matmul model parallelism")
        self.img_size = inp_shape
        self.patch_size = patch_size
        self.inp_chans = inp_chans
        self.out_chans = out_chans
        self.embed_dim = embed_dim
        assert len(patch_size) == 2, f"Expected patch_size to have two entries but got {patch_size} instead"
        assert (self.img_size[0] % self.patch_size[0] == 0) and (self.img_size[1] % self.patch_size[1] == 0), \
            f"Error, the patch size {self.patch_size} does not divide the image dimensions {self.img_size} evenly."
        self.patch_embed = PatchEmbed(img_size=self.img_size, patch_size=self.patch_size, in_chans=self.inp_chans, embed_dim=self.embed_dim)
        num_patches = self.patch_embed.num_patches
        self.pos_embed = nn.Parameter(torch.zeros(1, embed_dim, num_patches))
        self.pos_drop = nn.Dropout(p=drop_rate) if drop_rate > 0.0 else nn.Identity()
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, num_layers)]
        self.h = self.img_size[0] // self.patch_size[0]
        self.w = self.img_size[1] // self.patch_size[1]
        if normalization_layer == "layer_norm":
            norm_layer = partial(LayerNorm, normalized_shape=(self.h, self.w), eps=1e-6)
        elif normalization_layer == "instance_norm":
            norm_layer = partial(InstanceNorm2d, num_features=embed_dim, eps=1e-6, affine=True, track_running_stats=False)
        else:
            raise NotImplementedError(f"Error, normalization {normalization_layer} not implemented.")
        self.blocks = nn.ModuleList([
            Block(h=self.h, w=self.w, dim=self.embed_dim, mlp_ratio=mlp_ratio, drop=drop_rate, drop_path=dpr[i], norm_layer=norm_layer,
                  num_blocks=num_blocks, sparsity_threshold=sparsity_threshold, hard_thresholding_fraction=hard_thresholding_fraction,
                  use_complex_kernels=use_complex_kernels, skip_fno=skip_fno, nested_skip_fno=nested_skip_fno,
                  checkpointing=checkpointing, verbose=verbose)
            for i in range(num_layers)])
        self.head = Conv1x1(embed_dim, self.out_chans * self.patch_size[0] * self.patch_size[1], bias=False)
        with torch.no_grad():
            nn.init.trunc_normal_(self.pos_embed, std=0.02)
        self.apply(self._init_weights)

    def _init_weights(self, m):
        if isinstance(m, nn.Linear) or isinstance(m, nn.Conv2d):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm) or isinstance(m, nn.InstanceNorm3d):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {"pos_embed", "cls_token"}

    def forward_features(self, x):
        B = x.shape[0]
        x = self.patch_embed(x)
        x = x + self.pos_embed
        x = self.pos_drop(x)
        x = x.reshape(B, self.embed_dim, self.h, self.w)
        for blk in self.blocks:
            x = blk(x)
        return x

    def forward(self, x):
        x = self.forward_features(x)
        x = self.head(x)
        b = x.shape[0]
        xv = x.view(b, self.patch_size[0], self.patch_size[1], -1, self.h, self.w)
        xvt = torch.permute(xv, (0, 3, 4, 1, 5, 2)).contiguous()
        return xvt.view(b, -1, (self.h * self.patch_size[0]), (self.w * self.patch_size[1]))
