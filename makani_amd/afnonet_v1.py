"""The channels-last AFNO network (``nettype: "AFNOv1"``, networks/afnonet.py, the one ``config/afnonet.yaml`` selects in its base
block): ``Mlp``, ``AFNO2D``, ``Block`` and ``AdaptiveFourierNeuralOperatorNet`` with the reference's constructor signatures,
attributes and ``state_dict`` keys.

The network carries tokens ``[B, H, W, C]``.  Its filter -- ``rfft2`` over the two middle axes, per channel block a complex
two-layer MLP with complex biases on a window of the coefficients, soft-shrink, ``irfft2``, plus its input -- runs under
``MK_AFNOV1=hip`` on

1. ``ops.tokens_to_fields`` (``mk_tokens_to_fields``: tokens to the channel-major fields the planar transforms read),
2. ``forward_packed`` of a planar pair whose latitude DFT table holds the window's frequencies (``mk_latdft_table_window``),
3. ``ops.spec_block_mlp`` with biases (``mk_spec_bdmlp_fwd_bias`` and the gradients of the ``mk_spec_bdmlp_*`` family),
4. ``inverse_packed``,
5. ``ops.fields_to_tokens`` with the filter's input as addend (``mk_fields_to_tokens``: the way back and the ``+ x`` in one pass).

The window (afnonet.py:78-103) is a quirk of the reference that is reproduced: with ``t = H // 2 + 1`` and ``k = int(t *
hard_thresholding_fraction)`` the latitude rows ``t - k ... min(t + k, H) - 1`` and the longitude columns ``0 ... min(k, W // 2 + 1)
- 1`` -- both limits from ``H``, the rows contiguous around the Nyquist row, not the low frequencies ``RealFFT2`` keeps.

A block's norms are ``layers.LayerNorm`` (``norm2`` one launch for the add of ``double_skip``, the norm and the sum, under
``MK_TOKEN_NORM=hip``), its MLP one ``ops.token_mlp`` node with the last residual add in ``fc2``'s epilogue (under
``MK_TOKEN_LINEAR=hip`` and bf16 autocast).  Under ``MK_PATCH=hip`` (default ``ops.PATCH_DEFAULT``) patch embedding and the position
add are ``PatchEmbed.forward_tokens`` -- ``mk_patchify`` and the token GEMM, for bf16 images or under bf16 autocast -- and the
un-patchify behind ``head`` one ``mk_unpatchify`` pass (csrc/patch.hip); ``MK_PATCH=torch`` keeps the convolution and the permute.
``MK_AFNOV1=torch`` (the default is ``hip``, timings: DESIGN section 27), a pair that is not ``hip_ready`` (``MK_PLANAR_FFT`` defaults to
``torch``) and every case the kernels do not take run ``AFNO2D._forward_torch``, the reference's formulation in torch ops.

Out of scope: ``PrecipNet``; model-parallel AFNO (spatial or matmul group sizes above 1 raise ``NotImplementedError``; data
parallelism works as for any module).
"""
from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F

try:
    from . import comm, ops
except ImportError:     # loaded by file path (the reference's registry: ``nettype: ".../makani_amd/afnonet_v1.py:Name"``), no package
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from makani_amd import comm, ops
from makani_amd.layers import DropPath, InverseRealFFT2, LayerNorm, Linear, PatchEmbed, RealFFT2, _is_exact_gelu


def kept_window(H, W, fraction):
    """afnonet.py:78-81 as ``(first, lmax, mmax)``: the latitude rows ``first ... first + lmax - 1`` and the longitude columns
    ``0 ... mmax - 1`` the filter processes; everything else of its output spectrum is zero."""
    total = H // 2 + 1
    kept = int(total * fraction)
    first = total - kept
    return first, max(min(total + kept, H) - first, 0), max(min(kept, W // 2 + 1), 0)


class _WindowTable:
    """The planar pair on a window of latitude frequencies: the same kernels, another table.  Packed forms only."""

    def _set_window(self, first):
        self.first = first
        if self._hip_sizes:
            self.dft_table = ops.latdft_table(self.nlat, self.lmax, first)

    def forward(self, x):
        raise NotImplementedError("the window pair serves forward_packed / inverse_packed only")

    _forward_torch = forward


class _WindowRealFFT2(_WindowTable, RealFFT2):
    def __init__(self, nlat, nlon, lmax, mmax, first):
        RealFFT2.__init__(self, nlat, nlon, lmax, mmax)
        self._set_window(first)


class _WindowInverseRealFFT2(_WindowTable, InverseRealFFT2):
    def __init__(self, nlat, nlon, lmax, mmax, first):
        InverseRealFFT2.__init__(self, nlat, nlon, lmax, mmax)
        self._set_window(first)


class Mlp(nn.Module):
    """afnonet.py:26-42 on token input; ``fc1`` / ``fc2`` are ``layers.Linear``.  With an exact GELU and inactive dropout the two
    linears are one ``ops.token_mlp`` node (which takes the torch calls for what the kernels decline); ``addend``: return
    ``addend + mlp(x)``, the block's residual add, in ``fc2``'s epilogue there."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.0):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = Linear(in_features, hidden_features)
        self.act = act_layer()
        self.fc2 = Linear(hidden_features, out_features)
        self.drop = nn.Dropout(drop)

    def forward(self, x, addend=None):
        if _is_exact_gelu(self.act) and not (self.training and self.drop.p > 0.0):
            return ops.token_mlp(x, self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias, addend)
        x = self.drop(self.fc2(self.drop(self.act(self.fc1(x)))))
        return x if addend is None else x + addend


class AFNO2D(nn.Module):
    """afnonet.py:45-112.  Parameters ``w1 [2, nb, bs, bs * f]``, ``b1 [2, nb, bs * f]``, ``w2 [2, nb, bs * f, bs]``, ``b2 [2, nb, bs]``
    (scale 0.02), the leading axis (real, imaginary).

    The fused path (autocast off inside) is the five steps of the module docstring on ``x [B, H, W, C]``.  The pair is built per
    ``(H, W)`` on first use for ``kept_window(H, W, fraction)``; the kernels' interleaved panels ``[nb, bs, hb, 2]`` /
    ``[nb * hb, 2]`` are permutes of the ``[2, ...]`` planes (weight-sized torch ops; the gradients come back through them).  The
    two gradients that meet at the filter's input -- the addend's and the transform's -- are added by autograd.  It applies to
    device fp32 / bf16 4-D inputs with even ``bs`` and ``bs * f``, even ``W``, ``lmax >= 2`` and ``mmax >= 1``, on the bf16x3 engine,
    where the pair's ``hip_ready`` holds (``MK_PLANAR_FFT=hip``) and ``MK_AFNOV1`` (``hip`` | ``torch``, read and validated on every
    call) is ``hip``.  Everything else takes ``_forward_torch``.

    Under autocast the reference's real einsums would run in bf16; the fused path does not follow it there and stays
    fp32-accurate.  A bf16 input gets bf16 rows from the inverse transform and one fp32 add rounded once: the reference's two
    rounding points.
    """

    def __init__(self, hidden_size, num_blocks=8, sparsity_threshold=0.01, hard_thresholding_fraction=1, hidden_size_factor=1):
        super().__init__()
        assert hidden_size % num_blocks == 0, f"hidden_size {hidden_size} should be divisble by num_blocks {num_blocks}"
        self.hidden_size = hidden_size
        self.sparsity_threshold = sparsity_threshold
        self.num_blocks = num_blocks
        self.block_size = self.hidden_size // self.num_blocks
        self.hard_thresholding_fraction = hard_thresholding_fraction
        self.hidden_size_factor = hidden_size_factor
        self.scale = 0.02
        nb, bs, hb = self.num_blocks, self.block_size, self.block_size * self.hidden_size_factor
        self.w1 = nn.Parameter(self.scale * torch.randn(2, nb, bs, hb))
        self.b1 = nn.Parameter(self.scale * torch.randn(2, nb, hb))
        self.w2 = nn.Parameter(self.scale * torch.randn(2, nb, hb, bs))
        self.b2 = nn.Parameter(self.scale * torch.randn(2, nb, bs))
        self._pairs = {}

    def _pair(self, H, W, device):
        key = (H, W, device)
        if key not in self._pairs:
            first, lmax, mmax = kept_window(H, W, self.hard_thresholding_fraction)
            self._pairs[key] = (_WindowRealFFT2(H, W, lmax, mmax, first).to(device),
                                _WindowInverseRealFFT2(H, W, lmax, mmax, first).to(device))
        return self._pairs[key]

    def _takes_fused(self, x):
        hip = ops.afnov1_hip()      # validates the knob on every call
        if not (hip and x.is_cuda and x.dim() == 4 and x.dtype in (torch.float32, torch.bfloat16) and x.numel() > 0):
            return False
        H, W = x.shape[1], x.shape[2]
        _, lmax, mmax = kept_window(H, W, self.hard_thresholding_fraction)
        hb = self.block_size * self.hidden_size_factor
        if self.block_size % 2 or hb % 2 or W % 2 or lmax < 2 or mmax < 1 or ops.SPECTRAL_GEMM != "bf16x3":
            return False
        if x.shape[3] != self.hidden_size or self.w1.dtype != torch.float32 or not self.w1.is_cuda:
            return False
        ft, it = self._pair(H, W, x.device)
        return ft.hip_ready(x) and it.hip_ready(x)

    def _forward_fused(self, x):
        B, H, W, C = x.shape
        ft, it = self._pair(H, W, x.device)
        tok = x.contiguous().view(B, H * W, C)
        c = ft.forward_packed(ops.tokens_to_fields(tok).view(B * C, H, W))
        w1, w2 = self.w1.permute(1, 2, 3, 0).contiguous(), self.w2.permute(1, 2, 3, 0).contiguous()
        b1, b2 = self.b1.permute(1, 2, 0).reshape(-1, 2), self.b2.permute(1, 2, 0).reshape(-1, 2)
        y = ops.spec_block_mlp(c, w1, w2, B, self.num_blocks, self.sparsity_threshold, b1, b2)
        r = it.inverse_packed(y, x.dtype)
        return ops.fields_to_tokens(r.view(B, C, H * W), tok).view(B, H, W, C)

    def _forward_torch(self, x):
        bias = x
        dtype = x.dtype
        x = x.float()
        B, H, W, C = x.shape
        x = torch.fft.rfft2(x, dim=(1, 2), norm="ortho")
        x = x.reshape(B, H, W // 2 + 1, self.num_blocks, self.block_size)
        o2_real = torch.zeros(x.shape, device=x.device)
        o2_imag = torch.zeros(x.shape, device=x.device)
        total_modes = H // 2 + 1
        kept_modes = int(total_modes * self.hard_thresholding_fraction)
        rows, cols = slice(total_modes - kept_modes, total_modes + kept_modes), slice(None, kept_modes)
        xs = x[:, rows, cols]

        def mul(a, w):
            return torch.einsum("...bi,bio->...bo", a, w)

        o1_real = F.relu(mul(xs.real, self.w1[0]) - mul(xs.imag, self.w1[1]) + self.b1[0])
        o1_imag = F.relu(mul(xs.imag, self.w1[0]) + mul(xs.real, self.w1[1]) + self.b1[1])
        o2_real[:, rows, cols] = mul(o1_real, self.w2[0]) - mul(o1_imag, self.w2[1]) + self.b2[0]
        o2_imag[:, rows, cols] = mul(o1_imag, self.w2[0]) + mul(o1_real, self.w2[1]) + self.b2[1]
        x = torch.stack([o2_real, o2_imag], dim=-1)
        x = F.softshrink(x, lambd=self.sparsity_threshold)
        x = torch.view_as_complex(x)
        x = x.reshape(B, H, W // 2 + 1, C)
        x = torch.fft.irfft2(x, s=(H, W), dim=(1, 2), norm="ortho")
        x = x.type(dtype)
        return x + bias

    def forward(self, x):
        if self._takes_fused(x):
            with torch.autocast(device_type="cuda", enabled=False):
                return self._forward_fused(x)
        return self._forward_torch(x)


class Block(nn.Module):
    """afnonet.py:115-152.  ``norm_layer`` is a factory taking ``dim`` (``nn.LayerNorm`` itself becomes ``layers.LayerNorm``).  With
    ``layers.LayerNorm`` norms, ``norm2`` is ``forward_add`` of the filter's output and the block's input and returns their sum, the
    ``double_skip`` residual; the last add is the MLP's ``addend`` unless ``drop_path`` is active."""

    def __init__(self, dim, mlp_ratio=4.0, drop=0.0, drop_path=0.0, act_layer=nn.GELU, norm_layer=nn.LayerNorm, double_skip=True,
                 num_blocks=8, sparsity_threshold=0.01, hard_thresholding_fraction=1.0):
        super().__init__()
        if norm_layer is nn.LayerNorm:
            norm_layer = LayerNorm
        self.norm1 = norm_layer(dim)
        self.filter = AFNO2D(dim, num_blocks, sparsity_threshold, hard_thresholding_fraction)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.norm2 = norm_layer(dim)
        mlp_hidden_dim = int(dim * mlp_ratio)
        self.mlp = Mlp(in_features=dim, hidden_features=mlp_hidden_dim, act_layer=act_layer, drop=drop)
        self.double_skip = double_skip

    def forward(self, x):
        residual = x
        if isinstance(self.norm1, LayerNorm) and isinstance(self.norm2, LayerNorm):
            (h,) = self.norm1.forward_add(x)
            h = self.filter(h)
            if self.double_skip:
                h, residual = self.norm2.forward_add(h, x, want_sum=True)
            else:
                (h,) = self.norm2.forward_add(h)
        else:
            h = self.filter(self.norm1(x))
            if self.double_skip:
                h = h + residual
                residual = h
            h = self.norm2(h)
        if isinstance(self.drop_path, nn.Identity):
            return self.mlp(h, addend=residual)
        return self.drop_path(self.mlp(h)) + residual


class AdaptiveFourierNeuralOperatorNet(nn.Module):
    """afnonet.py:174-268: patch embedding, position embedding, ``num_layers`` blocks on ``[B, h, w, embed_dim]`` tokens, a linear
    head and the rearrangement of its ``p0 * p1 * out_chans`` features back onto the full grid.  All keywords and defaults of the
    reference; further keywords are tolerated like there."""

    def __init__(self, inp_shape=(720, 1440), patch_size=(16, 16), inp_chans=2, out_chans=2, embed_dim=768, num_layers=12,
                 mlp_ratio=4.0, drop_rate=0.0, drop_path_rate=0.0, num_blocks=16, sparsity_threshold=0.01,
                 hard_thresholding_fraction=1.0, **kwargs):
        super().__init__()
        if comm.get_size("h") * comm.get_size("w") > 1 or comm.get_size("fin") * comm.get_size("fout") > 1:
            raise NotImplementedError("AFNOv1 runs data parallel only: no spatial or matmul model parallelism")
        self.img_size = inp_shape
        self.patch_size = patch_size
        self.inp_chans = inp_chans
        self.out_chans = out_chans
        self.embed_dim = embed_dim
        norm_layer = partial(LayerNorm, eps=1e-6)
        self.patch_embed = PatchEmbed(img_size=self.img_size, patch_size=self.patch_size, in_chans=self.inp_chans, embed_dim=self.embed_dim)
        num_patches = self.patch_embed.num_patches
        self.pos_embed = nn.Parameter(torch.zeros(1, num_patches, self.embed_dim))
        self.pos_drop = nn.Dropout(p=drop_rate)
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, num_layers)]
        self.h = self.img_size[0] // self.patch_size[0]
        self.w = self.img_size[1] // self.patch_size[1]
        self.blocks = nn.ModuleList([
            Block(dim=self.embed_dim, mlp_ratio=mlp_ratio, drop=drop_rate, drop_path=dpr[i], norm_layer=norm_layer,
                  num_blocks=num_blocks, sparsity_threshold=sparsity_threshold, hard_thresholding_fraction=hard_thresholding_fraction)
            for i in range(num_layers)])
        self.head = Linear(self.embed_dim, self.out_chans * self.patch_size[0] * self.patch_size[1], bias=False)
        with torch.no_grad():
            nn.init.trunc_normal_(self.pos_embed, std=0.02)
        self.apply(self._init_weights)

    def _init_weights(self, m):
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {"pos_embed", "cls_token"}

    def forward_features(self, x):
        B = x.shape[0]
        x = self.patch_embed.forward_tokens(x, self.pos_embed)
        x = self.pos_drop(x)
        x = x.reshape(B, self.h, self.w, self.embed_dim)
        for blk in self.blocks:
            x = blk(x)
        return x

    def forward(self, x):
        x = self.forward_features(x)
        x = self.head(x)
        # features (p0, p1, c): permute(0, 5, 1, 3, 2, 4) of [b, h, w, p0, p1, c] is order 1
        return ops.unpatchify(x, self.patch_size, self.out_chans, (self.h * self.patch_size[0], self.w * self.patch_size[1]), order=1)
