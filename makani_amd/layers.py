"""Glue layers that run between the spectral ops: encoder/decoder, MLP, DropPath, FFT wrappers.

Same constructor arguments, initialisation and ``state_dict`` keys as
``makani/models/common/layers.py:35-287``.  Pointwise 1x1 convolutions are evaluated as
one GEMM over the NCHW field viewed as ``[C, H*W]`` (hipBLASLt through torch) -- the
parameters stay ``nn.Conv2d`` weights ``[O, I, 1, 1]`` so reference checkpoints load.
"""
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.utils.checkpoint import checkpoint

from . import ops


class _X3Conv(torch.autograd.Function):
    """y[b] = W @ x[b] (+ addend[b], accumulated in place) on fp32 ``[B, C, P]`` fields: forward, data gradient and weight
    gradient on the bf16x3 MFMA engine of the spectral GEMMs (``mk_conv1x1_x3``: fp32-accurate, hand-written) -- the path of
    every 1x1 convolution outside bf16 autocast."""

    @staticmethod
    def forward(ctx, x3, w, addend):
        wf = w.detach().float()
        ctx.save_for_backward(x3, wf)
        ctx.cfg = (w.dtype, addend is not None)
        return ops.conv1x1_x3(wf, x3, out=None if addend is None else addend.detach())

    @staticmethod
    def backward(ctx, gy):
        x3, wf = ctx.saved_tensors
        wdt, has_addend = ctx.cfg
        gy = gy.contiguous()
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = ops.conv1x1_x3(wf.t().contiguous(), gy)
        if ctx.needs_input_grad[1]:
            gw = ops.conv1x1_x3_wgrad(gy, x3).to(wdt)
        return gx, gw, (gy if has_addend else None)


class _PointwiseConv(torch.autograd.Function):
    """y[b] = W @ x[b] on the NCHW field viewed as [C, H*W]; hand-written backward.

    hipBLASLt runs the weight-gradient GEMM  gW = gY @ X^T  (contraction over H*W ~ 1e5..1e6,
    output only [O x I]) on a few dozen workgroups; splitting the contraction into SPLIT batched
    chunks (strided views, no copies) and summing the partials in fp32 fills the chip.
    """
    SPLIT = int(os.environ.get("MK_WGRAD_SPLIT", "32"))

    @staticmethod
    def forward(ctx, x3, w_master, addend):
        # x3 [B, I, P], w_master [O, I] (the parameter view, any float dtype), optional addend [B, O, P] (skip
        # connection folded into the GEMM epilogue: y = addend + W x).  The weight is cast to the activation dtype
        # here, inside the node, so its gradient goes back in fp32 straight from the wgrad kernel (no bf16 round
        # trip, two tiny cast kernels fewer per convolution).
        w = w_master if w_master.dtype == x3.dtype else w_master.to(x3.dtype)
        ctx.master_dtype = w_master.dtype
        ctx.save_for_backward(x3, w)
        ctx.has_addend = addend is not None
        if addend is not None:
            # y = addend + W x accumulated IN PLACE into the addend's storage: an out-of-place addmm first copies the
            # addend into the result (one D2D copy of the whole activation per block, 0.5 ms per step).  The addend is
            # the block's norm1 output, which no backward needs (the norm keeps its input and statistics, this node
            # returns gy for it); should anyone have saved it, autograd's version check fails loudly in backward.
            out = addend.detach()
            if x3.shape[0] == 1:
                torch.addmm(out[0], w, x3[0], out=out[0])
            else:
                torch.baddbmm(out, w.unsqueeze(0).expand(x3.shape[0], -1, -1), x3, out=out)
            return out
        if x3.shape[0] == 1:
            return torch.mm(w, x3[0]).unsqueeze(0)
        return torch.bmm(w.unsqueeze(0).expand(x3.shape[0], -1, -1), x3)

    @staticmethod
    def backward(ctx, gy):
        x3, w = ctx.saved_tensors
        B, I, P = x3.shape
        O = w.shape[0]
        gy = gy.contiguous()
        gx = gw = None
        ga = gy if ctx.has_addend else None
        if ctx.needs_input_grad[0]:
            if B == 1:
                gx = torch.mm(w.t(), gy[0]).unsqueeze(0)
            else:
                gx = torch.bmm(w.t().unsqueeze(0).expand(B, -1, -1), gy)
        if ctx.needs_input_grad[1] and x3.is_cuda and x3.dtype == torch.bfloat16 and gy.dtype == torch.bfloat16 \
                and P % 8 == 0 and ops._knob("MK_CONV_WGRAD", "hip") == "hip":
            # hand-written bf16 MFMA kernel: pixel slabs per workgroup, fp32 atomics into gW
            gw = ops.conv1x1_wgrad_raw(gy, x3.contiguous()).to(ctx.master_dtype)
        elif ctx.needs_input_grad[1]:
            S = _PointwiseConv.SPLIT
            while S > 1 and P % S:
                S //= 2
            kc = P // S
            # per sample: [O, S, kc] -> [S, O, kc] and [I, S, kc] -> [S, kc, I] are strided views (no copies)
            gw32 = None
            for bi in range(B):
                a = gy[bi].view(O, S, kc).permute(1, 0, 2)
                b = x3[bi].view(I, S, kc).permute(1, 2, 0)
                part = torch.bmm(a, b).float().sum(0)
                gw32 = part if gw32 is None else gw32 + part
            gw = gw32.to(ctx.master_dtype)
        return gx, gw, ga


def _step_items(w):
    """What the backward pass of a convolution with weight ``w`` takes from the open ``ops.EngineArena`` scope: (transposed
    image, zeroed gradient buffer), each None outside a scope (the backward pass then packs / allocates itself)."""
    return ops.arena_image(w, True), (ops.arena_grad_buffer(w) if w.requires_grad else None)


def _engine_backward(ctx, g, x3, w, need_gx, need_gw, **gx_args):
    """The backward block of one engine convolution ``y = W @ x3`` for the gradient ``g`` of ``y``: ``(gx, gw)``, each None where
    not needed.  It uses up the next ``_step_items`` pair of ``ctx.step`` (a node with two weights stores two pairs, in the order
    of its calls); ``gx_args`` go to the launch of the data gradient."""
    # taken once: no reference may survive this call (autograd adopts gw only as its sole owner); a second backward pass
    # through the same node packs / allocates for itself
    step = ctx.step or (None, None)
    (wimg_t, gbuf), ctx.step = step[:2], step[2:]
    gx = gw = None
    if need_gx:
        gx = ops.pce_gemm(g, wimg_t if wimg_t is not None else ops.pce_pack(w, transpose=True), w.shape[1], **gx_args)
    if need_gw:
        gw = ops.conv1x1_wgrad_raw(g, x3, out=gbuf).to(w.dtype)
    return gx, gw


def _row_sums(t3):
    """sum over (batch, pixels) of a [B, C, P] field -> fp32 [C] (the HIP row-sum pass of the instance norm)."""
    r = ops.row_sums(t3).view(t3.shape[0], t3.shape[1])
    return r[0] if r.shape[0] == 1 else r.sum(0)      # one batch item: nothing to add up (saves a launch per bias gradient)


class _PceConv(torch.autograd.Function):
    """y[b] = W @ x[b] (+ bias) (+ addend[b]) on bf16 ``[B, C, P]`` fields, one pixel-column-engine launch
    (csrc/pce.hip) each way; the weight gradient comes from the bf16 MFMA wgrad kernel in fp32."""

    @staticmethod
    def forward(ctx, x3, w, bias, addend):
        ctx.save_for_backward(x3, w)
        ctx.has = (bias is not None, addend is not None)
        ctx.bias_dtype = None if bias is None else bias.dtype
        ctx.step = _step_items(w)
        return ops.pce_gemm(x3, ops.pce_pack(w), w.shape[0], bias=bias, addend=addend)

    @staticmethod
    def backward(ctx, gy):
        x3, w = ctx.saved_tensors
        has_bias, has_addend = ctx.has
        gy = gy.contiguous()
        gb = None
        gx, gw = _engine_backward(ctx, gy, x3, w, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        if has_bias and ctx.needs_input_grad[2]:
            gb = _row_sums(gy).to(ctx.bias_dtype)
        return gx, gw, gb, (gy if has_addend else None)


class _PceConvNormAdd(torch.autograd.Function):
    """out[b] = W @ x[b] (+ bias) + instance_norm(z)[b]: the tail of an SFNO block (``sfnonet.py:262-267``: norm1 of the
    MLP output, then the outer skip) as ONE engine launch.  The norm's statistics come with ``z`` from the launch that
    produced it (``sums``: fp64 ``[B * C, 2]`` local row sums), a 2 us kernel turns them into per-row coefficients, and the
    GEMM epilogue applies ``a * z + b`` while it adds the skip -- the normalised field is never written.  Backward: the
    convolution's two gradients as in ``_PceConv``; the norm's from ``z``, the incoming gradient and the saved (mean, rstd)."""

    @staticmethod
    def forward(ctx, x3, w, bias, z4, sums, nw, nb, eps, group, count):
        B, C, H, W = z4.shape
        if group is not None:
            torch.distributed.all_reduce(sums, group=group)
        cnt = H * W if group is None else int(count)
        wf = None if nw is None else nw.detach().float().contiguous()
        bf = None if nb is None else nb.detach().float().contiguous()
        stats, affine = ops.instance_norm_coeffs(sums, wf, bf, B * C, C, cnt, eps)
        y = ops.pce_gemm(x3, ops.pce_pack(w), w.shape[0], bias=bias, addend=z4.view(B, C, H * W), addend_affine=affine)
        empty = z4.new_empty(0, dtype=torch.float32)
        ctx.save_for_backward(x3, w, z4, stats, wf if wf is not None else empty, bf if bf is not None else empty)
        ctx.cfg = (None if bias is None else bias.dtype, None if nw is None else nw.dtype, None if nb is None else nb.dtype,
                   group, cnt)
        ctx.step = _step_items(w)
        return y

    @staticmethod
    def backward(ctx, gy):
        x3, w, z4, stats, wf, bf = ctx.saved_tensors
        bias_dtype, nw_dtype, nb_dtype, group, cnt = ctx.cfg
        B, C, H, W = z4.shape
        gy = gy.contiguous()
        gb = None
        gx, gw = _engine_backward(ctx, gy, x3, w, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        if bias_dtype is not None and ctx.needs_input_grad[2]:
            gb = _row_sums(gy).to(bias_dtype)
        gz, gnw, gnb = ops.instance_norm_backward(z4, gy.view(B, C, H, W), stats, wf if nw_dtype is not None else None,
                                                  bf if nb_dtype is not None else None, False, group, cnt,
                                                  grad_dtype=nw_dtype if (nw_dtype is not None and nw_dtype == nb_dtype) else None)
        return (gx, gw, gb, gz, None, gnw.to(nw_dtype) if nw_dtype is not None else None,
                gnb.to(nb_dtype) if nb_dtype is not None else None, None, None, None)


def conv_plus_instance_norm(conv, x, z, sums, norm):
    """``conv(x) + norm(z)`` as one launch (``_PceConvNormAdd``) when the engine can take it, else None: ``conv`` a
    ``Conv1x1``, ``norm`` an affine-or-not instance norm on the field's own statistics (single-GPU or spatially
    distributed), ``z`` a bf16 field that came with its row sums ``sums``."""
    from . import comm
    from .layer_norm import DistributedInstanceNorm2d
    if sums is None or not isinstance(conv, Conv1x1) or z.dtype != torch.bfloat16 or not z.is_contiguous() or z.dim() != 4:
        return None
    if ops._knob("MK_NORM_SKIP_FUSION", "1") == "0":
        return None
    group = count = None
    if isinstance(norm, DistributedInstanceNorm2d):
        if comm.get_size("spatial") > 1:
            group, count = comm.get_group("spatial"), norm._global_count(z)
        nw, nb = (norm.weight, norm.bias) if norm.affine else (None, None)
    elif isinstance(norm, InstanceNorm2d) and not norm.track_running_stats:
        nw, nb = norm.weight, norm.bias
    else:
        return None
    x3 = _engine_field(x)
    if x3 is None or not ops.pce_supported_train(conv.out_channels, conv.in_channels) or conv.out_channels != z.shape[1]:
        return None
    B, H, W = x.shape[0], x.shape[-2], x.shape[-1]
    if tuple(z.shape) != (B, conv.out_channels, H, W):
        return None
    with torch.autocast("cuda", enabled=False):
        y = _PceConvNormAdd.apply(x3, conv.weight2d(), conv.bias, z, sums, nw, nb, norm.eps, group, count)
    return y.view(B, conv.out_channels, H, W)


class _NormSkipAdd(torch.autograd.Function):
    """out = r + instance_norm(z): the tail of an SFNO block whose outer skip convolution ran in the spectral domain
    (``ops.spec_mix`` in front of the synthesis that produced ``r``).  The statistics come with ``z`` as in
    ``_PceConvNormAdd``; one streaming pass (``mk_affine_add``) applies ``a * z + b`` and adds the skip.  Backward: the
    gradient of ``r`` is the incoming gradient itself, the norm's comes from ``z`` and the saved (mean, rstd)."""

    @staticmethod
    def forward(ctx, r4, z4, sums, nw, nb, eps, group, count):
        B, C, H, W = z4.shape
        if group is not None:
            torch.distributed.all_reduce(sums, group=group)
        cnt = H * W if group is None else int(count)
        wf = None if nw is None else nw.detach().float().contiguous()
        bf = None if nb is None else nb.detach().float().contiguous()
        stats, affine = ops.instance_norm_coeffs(sums, wf, bf, B * C, C, cnt, eps)
        y = ops.affine_add(r4, z4, affine)
        empty = z4.new_empty(0, dtype=torch.float32)
        ctx.save_for_backward(z4, stats, wf if wf is not None else empty, bf if bf is not None else empty)
        ctx.cfg = (None if nw is None else nw.dtype, None if nb is None else nb.dtype, group, cnt)
        return y

    @staticmethod
    def backward(ctx, gy):
        z4, stats, wf, bf = ctx.saved_tensors
        nw_dtype, nb_dtype, group, cnt = ctx.cfg
        gy = gy.contiguous()
        gz, gnw, gnb = ops.instance_norm_backward(z4, gy, stats, wf if nw_dtype is not None else None,
                                                  bf if nb_dtype is not None else None, False, group, cnt,
                                                  grad_dtype=nw_dtype if (nw_dtype is not None and nw_dtype == nb_dtype) else None)
        return (gy, gz, None, gnw.to(nw_dtype) if nw_dtype is not None else None,
                gnb.to(nb_dtype) if nb_dtype is not None else None, None, None, None)


class _NormSkipAddFFT(torch.autograd.Function):
    """``_NormSkipAdd`` with the add folded into the inverse FFT that synthesises the skip (``mk_irfft_affine_add``):
    out = irfft(xf) + instance_norm(z); the synthesised skip is never written.  Backward: the adjoint FFT of the incoming
    gradient for ``xf`` (as ``ops._IRFFT``), the norm's gradients from ``z`` and the saved (mean, rstd).  Unsharded rows only."""

    @staticmethod
    def forward(ctx, xf, twiddles, nlon, kmajor, z4, sums, nw, nb, eps):
        B, C, H, W = z4.shape
        wf = None if nw is None else nw.detach().float().contiguous()
        bf = None if nb is None else nb.detach().float().contiguous()
        stats, affine = ops.instance_norm_coeffs(sums, wf, bf, B * C, C, H * W, eps)
        y = ops.irfft_affine_add_raw(xf, twiddles, nlon, z4, affine, kmajor)
        empty = z4.new_empty(0, dtype=torch.float32)
        ctx.save_for_backward(z4, stats, wf if wf is not None else empty, bf if bf is not None else empty, twiddles)
        ctx.cfg = (None if nw is None else nw.dtype, None if nb is None else nb.dtype, xf.shape[1] if kmajor else xf.shape[0],
                   bool(kmajor))
        return y

    @staticmethod
    def backward(ctx, gy):
        z4, stats, wf, bf, tw = ctx.saved_tensors
        nw_dtype, nb_dtype, mmax, kmajor = ctx.cfg
        B, C, H, W = z4.shape
        gy = gy.contiguous()
        gxf = ops.rfft_raw(gy.view(B * C, H, W), tw, mmax, 1.0, 2.0, 1.0, kmajor) if ctx.needs_input_grad[0] else None
        gz, gnw, gnb = ops.instance_norm_backward(z4, gy, stats, wf if nw_dtype is not None else None,
                                                  bf if nb_dtype is not None else None, False, None, H * W,
                                                  grad_dtype=nw_dtype if (nw_dtype is not None and nw_dtype == nb_dtype) else None)
        return (gxf, None, None, None, gz, None, gnw.to(nw_dtype) if nw_dtype is not None else None,
                gnb.to(nb_dtype) if nb_dtype is not None else None, None)


def spectral_skip_supported(conv, z_like):
    """The outer skip ``conv`` may run on the spectrum: a bias-free ``Conv1x1`` the channel mix takes, in a step on the bf16
    engine (the conditions ``conv_plus_instance_norm`` checks before it sees the MLP output)."""
    if not isinstance(conv, Conv1x1) or conv.bias is not None or not ops.spec_mix_supported(conv.in_channels, conv.out_channels):
        return False
    if ops._knob("MK_NORM_SKIP_FUSION", "1") == "0" or ops._knob("MK_CONV_ENGINE", "pce") != "pce":
        return False
    if not (z_like.is_cuda and z_like.dim() == 4):
        return False
    return z_like.dtype == torch.bfloat16 or (z_like.dtype == torch.float32 and torch.is_autocast_enabled()
                                              and torch.get_autocast_dtype("cuda") == torch.bfloat16)


def spectral_skip_plus_instance_norm(conv, filt, spec, z, sums, norm):
    """``isht(conv.weight . spec) + norm(z)``: the skip convolution as a channel mix of the block's input spectrum ``spec``
    (``filt``: the block's ``SpectralConv``, whose inverse transform synthesises it), the norm's apply pass and the add in one
    streaming pass -- or None where ``conv_plus_instance_norm`` would decline too (the caller then synthesises the residual)."""
    from . import comm
    from .layer_norm import DistributedInstanceNorm2d
    if sums is None or z.dtype != torch.bfloat16 or not z.is_contiguous() or z.dim() != 4 or not ops.pointwise_supported(z):
        return None
    group = count = None
    if isinstance(norm, DistributedInstanceNorm2d):
        if comm.get_size("spatial") > 1:
            group, count = comm.get_group("spatial"), norm._global_count(z)
        nw, nb = (norm.weight, norm.bias) if norm.affine else (None, None)
    elif isinstance(norm, InstanceNorm2d) and not norm.track_running_stats:
        nw, nb = norm.weight, norm.bias
    else:
        return None
    B, C, H, W = z.shape
    if C != conv.out_channels or (H, W) != (filt.nlat_local, filt.nlon_local):
        return None
    from .sht import InverseRealSHT
    it = filt.inverse_transform
    with torch.autocast("cuda", enabled=False):
        cm = ops.spec_mix(spec, conv.weight, B, filt.l_off, filt.m_off)
        if group is None and type(it) is InverseRealSHT and ops.irfft_affine_add_supported(it.nlon, it.mmax):
            # the synthesis' inverse FFT applies the norm and adds z while it stores: no residual field, no separate pass
            km = ops.SPECTRAL_GEMM == "bf16x3"
            xf = ops.legendre_inv(cm, it.pct, it.nlat, 0, km)
            return _NormSkipAddFFT.apply(xf, it.twiddles, it.nlon, km, z, sums, nw, nb, norm.eps)
        r = filt.synthesise(cm, B, z.dtype)
        return _NormSkipAdd.apply(r.view(B, C, H, W), z, sums, nw, nb, norm.eps, group, count)


class _PceConvGelu(torch.autograd.Function):
    """h = gelu(W @ x + bias) on bf16 ``[B, C, P]`` fields: an encoder in front of its last convolution when that convolution
    runs in the spectral domain (``ops.spec_mix`` behind the analysis).  Forward: one engine launch that also keeps the
    pre-activation.  Backward: ``gpre = gh * gelu'(pre)`` with the bias gradient as its row sums in one streaming pass
    (``mk_bias_gelu_bwd``), the weight gradient from the wgrad kernel, the data gradient (if anyone asks) from the engine."""

    @staticmethod
    def forward(ctx, x3, w, bias, keep_pre):
        if keep_pre:
            h, pre = ops.pce_gemm(x3, ops.pce_pack(w), w.shape[0], bias=bias, want_pre=True, gelu=True)
        else:
            h, pre = ops.pce_gemm(x3, ops.pce_pack(w), w.shape[0], bias=bias, gelu=True), x3.new_empty(0)
        ctx.save_for_backward(x3, w, pre)
        ctx.bias_dtype = None if bias is None else bias.dtype
        ctx.step = _step_items(w)
        return h

    @staticmethod
    def backward(ctx, gh):
        x3, w, pre = ctx.saved_tensors
        need_gb = ctx.bias_dtype is not None and ctx.needs_input_grad[2]
        gpre, gsum = ops.gelu_backward(pre, gh.contiguous(), need_gb)
        gx, gw = _engine_backward(ctx, gpre, x3, w, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return gx, gw, (gsum.to(ctx.bias_dtype) if need_gb else None), None


def encoder_head(encoder, x):
    """``(h, last)`` with ``h`` the field in front of the encoder's last convolution ``last`` -- for a caller that evaluates
    that convolution behind a spherical harmonic analysis (``ops.spec_mix``) -- or None where the pattern is not the one the
    engine takes in one launch: ``[Conv1x1, exact GELU, no-ops..., bias-free Conv1x1]`` on a bf16 (or autocast-to-bf16) field."""
    mods = list(encoder.fwd)
    pat = _mlp_pattern(mods)
    if pat is None or x.dim() != 4:
        return None
    fc1, fc2 = pat
    if fc2.bias is not None or not ops.spec_mix_supported(fc2.in_channels, fc2.out_channels):
        return None
    x3 = _engine_field(x)
    if x3 is None or not ops.pce_supported_train(fc1.out_channels, fc1.in_channels):
        return None
    with torch.autocast("cuda", enabled=False):
        h = _PceConvGelu.apply(x3, fc1.weight2d(), fc1.bias, torch.is_grad_enabled())
    return h.view(x.shape[0], fc1.out_channels, x.shape[2], x.shape[3]), fc2


class _PceMLP(torch.autograd.Function):
    """y = W2 @ gelu(W1 @ x + b1) (+ b2): the MLP / encoder / decoder of ``layers.py:86-216`` on bf16 ``[B, C, P]``
    fields.  Forward: two engine launches, bias + GELU in the epilogue of the first (which also keeps the
    pre-activation).  Backward: ``gpre = (W2^T gy) * gelu'(pre)`` in one launch, ``gx = W1^T gpre`` in another, the two
    weight gradients from the wgrad kernel, the bias gradients from row sums.

    ``b2`` may be switched off with ``apply_b2=False`` (the caller normalises the result per channel, which removes any
    per-channel constant): the parameter stays in the graph and receives the exact gradient of that case -- zero -- so
    wrappers that expect every parameter to get a gradient (DistributedDataParallel, ``mpu/mappings.py:86-96``) work."""

    @staticmethod
    def forward(ctx, x3, w1, b1, w2, b2, apply_b2, want_row_sums, keep_pre=True):
        # keep_pre: the caller's `torch.is_grad_enabled()` (inside forward grad mode is always off, and needs_input_grad ignores it)
        if keep_pre:
            h, pre = ops.pce_gemm(x3, ops.pce_pack(w1), w1.shape[0], bias=b1, want_pre=True, gelu=True)
        else:       # inference: nobody will ask for GELU'(pre) -- the first launch writes the hidden field once, not twice
            h, pre = ops.pce_gemm(x3, ops.pce_pack(w1), w1.shape[0], bias=b1, gelu=True), x3.new_empty(0)
        want_row_sums = bool(want_row_sums) and w2.shape[0] <= 768
        y = ops.pce_gemm(h, ops.pce_pack(w2), w2.shape[0], bias=b2 if (apply_b2 and b2 is not None) else None,
                         want_row_sums=want_row_sums)
        y, sums = y if want_row_sums else (y, x3.new_empty(0, dtype=torch.float64))
        ctx.save_for_backward(x3, w1, w2, pre, h)
        ctx.cfg = (None if b1 is None else b1.dtype, None if b2 is None else (b2.dtype, tuple(b2.shape)), bool(apply_b2))
        ctx.step = _step_items(w2) + _step_items(w1)       # in the order the backward pass uses them
        ctx.mark_non_differentiable(sums)
        return y, sums

    @staticmethod
    def backward(ctx, gy, _gsums):
        x3, w1, w2, pre, h = ctx.saved_tensors
        b1_dtype, b2_info, apply_b2 = ctx.cfg
        gy = gy.contiguous()
        need_gb1 = b1_dtype is not None and ctx.needs_input_grad[2]
        fused_gb1 = need_gb1 and w2.shape[1] <= 768
        gpre, gw2 = _engine_backward(ctx, gy, h, w2, True, ctx.needs_input_grad[3], aux_in=pre, want_row_sums=fused_gb1)
        if fused_gb1:       # the bias gradient is the pixel sum of gpre: a by-product of the launch that wrote it
            gpre, gsum = gpre
        gb1 = gb2 = None
        gx, gw1 = _engine_backward(ctx, gpre, x3, w1, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        if need_gb1:
            if fused_gb1:
                g1 = gsum.view(gy.shape[0], -1, 2)[..., 0]
                gb1 = (g1[0] if g1.shape[0] == 1 else g1.sum(0)).to(b1_dtype)
            else:
                gb1 = _row_sums(gpre).to(b1_dtype)
        if b2_info is not None and ctx.needs_input_grad[4]:
            gb2 = _row_sums(gy).to(b2_info[0]) if apply_b2 else torch.zeros(b2_info[1], dtype=b2_info[0], device=gy.device)
        return gx, gw1, gb1, gw2, gb2, None, None, None


class _PceMLPFused(torch.autograd.Function):
    """The same node as ``_PceMLP`` on the fused kernel (``mk_pce_mlp``, csrc/pce_mlp.hip): conv -> GELU -> conv in ONE launch with
    the hidden field on chip, forward and backward; only the pre-activation is kept (bf16), the second weight gradient applies
    the GELU while it stages it (``mk_conv1x1_wgrad_act``).  Opt-in (``MK_MLP_FUSED=1``): on MI355X the launch is 8-13 % faster
    than the pair it replaces going forward, 5 % slower going backward, and the activated weight gradient costs more than the
    bytes saved -- the step as a whole does not gain."""

    @staticmethod
    def forward(ctx, x3, w1, b1, w2, b2, apply_b2, want_row_sums):
        out = ops.pce_mlp(x3, ops.pce_mlp_pack(w1, False, w2, False), 0, b1=b1,
                          b2=b2 if (apply_b2 and b2 is not None) else None, want_row_sums=bool(want_row_sums))
        y, pre = out[0], out[1]
        sums = out[2] if want_row_sums else x3.new_empty(0, dtype=torch.float64)
        ctx.save_for_backward(x3, w1, w2, pre)
        ctx.cfg = (None if b1 is None else b1.dtype, None if b2 is None else (b2.dtype, tuple(b2.shape)), bool(apply_b2))
        ctx.step = (ops.arena_grad_buffer(w1) if w1.requires_grad else None, ops.arena_grad_buffer(w2) if w2.requires_grad else None)
        ctx.mark_non_differentiable(sums)
        return y, sums

    @staticmethod
    def backward(ctx, gy, _gsums):
        x3, w1, w2, pre = ctx.saved_tensors
        b1_dtype, b2_info, apply_b2 = ctx.cfg
        (g1buf, g2buf), ctx.step = (ctx.step or (None, None)), None
        gy = gy.contiguous()
        need_gb1 = b1_dtype is not None and ctx.needs_input_grad[2]
        out = ops.pce_mlp(gy, ops.pce_mlp_pack(w2, True, w1, True), 1, pre=pre, want_mid_sums=need_gb1)
        gx, gpre = out[0], out[1]
        gw1 = gb1 = gw2 = gb2 = None
        if ctx.needs_input_grad[1]:
            gw1 = ops.conv1x1_wgrad_raw(gpre, x3, out=g1buf).to(w1.dtype)
        if need_gb1:
            g1 = out[2].view(gy.shape[0], -1)
            gb1 = (g1[0] if g1.shape[0] == 1 else g1.sum(0)).to(b1_dtype)
        if ctx.needs_input_grad[3]:
            gw2 = ops.conv1x1_wgrad_raw(gy, pre, x_gelu=True, out=g2buf).to(w2.dtype)
        if b2_info is not None and ctx.needs_input_grad[4]:
            gb2 = _row_sums(gy).to(b2_info[0]) if apply_b2 else torch.zeros(b2_info[1], dtype=b2_info[0], device=gy.device)
        return (gx if ctx.needs_input_grad[0] else None), gw1, gb1, gw2, gb2, None, None


def _mlp_fused_ok(fc1, fc2):
    """The fused node takes the layer in both directions (K1, M <= 384, hidden <= 768) and is switched on."""
    return (ops._knob("MK_MLP_FUSED", "0") == "1" and fc2.out_channels <= 384
            and ops.pce_mlp_supported(fc2.out_channels, fc1.out_channels, fc1.in_channels)
            and ops.pce_mlp_supported(fc1.in_channels, fc1.out_channels, fc2.out_channels))


def _engine_field(x):
    """The field as the pixel-column engine takes it (bf16 ``[B, C, P]``, contiguous, P a multiple of 8), or None."""
    if ops._knob("MK_CONV_ENGINE", "pce") != "pce":
        return None
    if not (x.is_cuda and x.dim() == 4 and x.is_contiguous() and (x.shape[2] * x.shape[3]) % 8 == 0):
        return None
    if x.dtype == torch.bfloat16:
        return x.view(x.shape[0], x.shape[1], -1)
    if torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16 and x.dtype == torch.float32:
        return x.view(x.shape[0], x.shape[1], -1).to(torch.bfloat16)
    return None


class Conv1x1(nn.Conv2d):
    """``nn.Conv2d(cin, cout, 1)`` (same parameters and ``state_dict`` entries) evaluated as a GEMM over the pixels."""

    def __init__(self, in_channels, out_channels, bias=True):
        super().__init__(in_channels, out_channels, 1, bias=bias)

    def weight2d(self):
        return self.weight.view(self.out_channels, self.in_channels)

    def forward(self, x, add_bias=True, addend=None):
        """``addend`` (same shape as the output) is added inside the GEMM epilogue: y = addend + conv(x)."""
        B, H, W = x.shape[0], x.shape[-2], x.shape[-1]
        x3 = _engine_field(x) if x.dim() == 4 else None
        if x3 is not None and ops.pce_supported_train(self.out_channels, self.in_channels):
            a3 = None
            if addend is not None:
                a3 = addend.contiguous().view(B, self.out_channels, H * W).to(torch.bfloat16)
            with torch.autocast("cuda", enabled=False):
                y = _PceConv.apply(x3, self.weight2d(), self.bias if add_bias else None, a3)
            return y.view(B, self.out_channels, H, W)
        if x.dim() != 4 or not x.is_contiguous() or not x.is_cuda:
            y = F.conv2d(x, self.weight, self.bias if add_bias else None)
            return y if addend is None else y + addend
        if addend is None and add_bias and self.bias is not None:
            y = _x3_inference_conv(self, x, False)        # fp32 inference: the bias add rides in the GEMM's epilogue
            if y is not None:
                return y
        # fp32 fields (no autocast): the bf16x3 engine (`_X3Conv`); torch mm / bmm only as the MK_CONV_FP32=torch A/B path
        if torch.is_autocast_enabled():
            x3 = x.view(B, x.shape[1], H * W).to(torch.get_autocast_dtype('cuda'))
        else:
            x3 = x.view(B, x.shape[1], H * W)
        with torch.autocast("cuda", enabled=False):
            a3 = None
            if addend is not None:
                a3 = addend.contiguous().view(B, self.out_channels, H * W).to(x3.dtype)
            if ops.conv1x1_x3_supported(x3) and (H * W) % 4 == 0 and ops._knob("MK_CONV_FP32", "x3") == "x3":
                y = _X3Conv.apply(x3, self.weight2d(), a3)
            else:
                y = _PointwiseConv.apply(x3, self.weight2d(), a3)
        if self.bias is not None and add_bias:
            y = y + self.bias.to(y.dtype).view(1, -1, 1)
        return y.view(B, self.out_channels, H, W)


def _x3_inference_conv(m, x, gelu):
    """fp32 field, grad mode off: ``act(conv(x) + bias)`` as ONE launch of the bf16x3 engine (bias and exact GELU in the epilogue,
    ``mk_conv1x1_x3_bias_act``), or None where that path does not apply."""
    if torch.is_grad_enabled() or x.dim() != 4 or not x.is_cuda or not x.is_contiguous() or x.dtype != torch.float32:
        return None
    if torch.is_autocast_enabled() or ops._knob("MK_CONV_FP32", "x3") != "x3":
        return None
    B, H, W = x.shape[0], x.shape[2], x.shape[3]
    x3 = x.view(B, x.shape[1], H * W)
    if not ops.conv1x1_x3_supported(x3) or (H * W) % 4 != 0 or m.weight.dtype != torch.float32:
        return None
    y = ops.conv1x1_x3(m.weight2d().detach(), x3, bias=None if m.bias is None else m.bias.detach(), gelu=gelu)
    return y.view(B, m.out_channels, H, W)


def _is_exact_gelu(m):
    return isinstance(m, nn.GELU) and getattr(m, "approximate", "none") == "none"


def _is_noop(m):
    return isinstance(m, nn.Identity) or (isinstance(m, (nn.Dropout, nn.Dropout2d)) and (m.p == 0.0 or not m.training))


def _mlp_pattern(mods):
    """``[Conv1x1, exact GELU, no-ops..., Conv1x1, no-ops...]`` -> (fc1, fc2), else None."""
    convs = [m for m in mods if isinstance(m, Conv1x1)]
    if len(convs) != 2 or not isinstance(mods[0], Conv1x1) or len(mods) < 3 or not _is_exact_gelu(mods[1]):
        return None
    rest = [m for m in mods[2:] if not _is_noop(m)]
    if len(rest) != 1 or rest[0] is not convs[1]:
        return None
    return convs[0], convs[1]


def _token_mlp_pattern(mods):
    """``[Linear, exact GELU, no-ops..., Linear, no-ops...]`` -> (fc1, fc2), else None."""
    lins = [m for m in mods if isinstance(m, nn.Linear)]
    if len(lins) != 2 or not isinstance(mods[0], Linear) or len(mods) < 3 or not _is_exact_gelu(mods[1]):
        return None
    rest = [m for m in mods[2:] if not _is_noop(m)]
    if len(rest) != 1 or rest[0] is not lins[1] or not isinstance(lins[1], Linear):
        return None
    return lins[0], lins[1]


def _run_token_chain(mods, x, addend):
    """The chain on token input ``[..., features]``: the two-linear pattern as ``ops.token_mlp`` (which takes the torch calls for what
    the kernels decline); with active dropout or another activation every module runs singly."""
    pat = _token_mlp_pattern(mods)
    if pat is not None:
        fc1, fc2 = pat
        return ops.token_mlp(x, fc1.weight, fc1.bias, fc2.weight, fc2.bias, addend)
    for m in mods:
        x = m(x)
    return x if addend is None else addend + x


def run_pointwise_chain(mods, x, skip_last_bias=False, want_row_sums=False, addend=None):
    """Evaluate an ``nn.Sequential`` of 1x1 convs / activations / identities, or of linears / activations on token input.

    The two-convolution pattern of ``MLP`` and ``EncoderDecoder`` (conv + bias, exact GELU, conv) runs as one fused
    autograd node on the pixel-column engine when the field is bf16 (or autocast to it).  Otherwise every
    ``Conv1x1(bias) -> GELU`` pair is one GEMM plus one HIP bias+GELU pass.

    ``skip_last_bias``: the caller feeds the result straight into an instance norm without running statistics, which
    removes any per-channel constant -- the last conv's bias add is then a no-op on the output and its gradient is
    exactly zero, so the add is skipped (the parameter still receives that zero gradient).

    ``want_row_sums``: return ``(y, sums)`` with ``sums`` the fp64 ``[B * C, 2]`` per-row (sum, sum of squares) of ``y``
    when the engine produced them alongside (else ``None``) -- the statistics of the instance norm that follows.

    ``addend`` (token input only): return ``addend + chain(x)``; the two-linear pattern adds it in ``fc2``'s epilogue.
    """
    mods = list(mods)
    if any(isinstance(m, nn.Linear) for m in mods):
        y = _run_token_chain(mods, x, addend)
        return (y, None) if want_row_sums else y
    if addend is not None:
        raise ValueError("run_pointwise_chain: addend is for token input (the traditional format) only")
    pat = _mlp_pattern(mods)
    if pat is not None and x.dim() == 4:
        fc1, fc2 = pat
        x3 = _engine_field(x)
        if (x3 is not None and ops.pce_supported_train(fc1.out_channels, fc1.in_channels)
                and ops.pce_supported_train(fc2.out_channels, fc2.in_channels)):
            fused = _mlp_fused_ok(fc1, fc2)
            with torch.autocast("cuda", enabled=False):
                if fused:
                    y, sums = _PceMLPFused.apply(x3, fc1.weight2d(), fc1.bias, fc2.weight2d(), fc2.bias, not skip_last_bias, want_row_sums)
                else:       # inference (grad mode off): the pre-activation is not kept -- one 768-row store less per MLP
                    y, sums = _PceMLP.apply(x3, fc1.weight2d(), fc1.bias, fc2.weight2d(), fc2.bias, not skip_last_bias, want_row_sums,
                                            torch.is_grad_enabled())
            y = y.view(x.shape[0], fc2.out_channels, x.shape[2], x.shape[3])
            return (y, sums if sums.numel() else None) if want_row_sums else y
    last_conv = max((j for j, m in enumerate(mods) if isinstance(m, Conv1x1)), default=-1)
    tail_is_noop = all(_is_noop(m) for m in mods[last_conv + 1:])
    i = 0
    while i < len(mods):
        m = mods[i]
        if skip_last_bias and tail_is_noop and i == last_conv and m.bias is not None:
            x = _ZeroGradBias.apply(m(x, add_bias=False), m.bias)
            i += 1
            continue
        if isinstance(m, Conv1x1) and i + 1 < len(mods) and _is_exact_gelu(mods[i + 1]) and x.is_cuda:
            y = _x3_inference_conv(m, x, True)            # fp32 inference: conv + bias + GELU in one launch
            if y is not None:
                x = y
                i += 2
                continue
            y = m(x, add_bias=False)
            if ops.pointwise_supported(y):
                x = ops.bias_gelu(y, m.bias)
            else:
                if m.bias is not None:
                    y = y + m.bias.to(y.dtype).view(1, -1, 1, 1)
                x = mods[i + 1](y)
            i += 2
        else:
            x = m(x)
            i += 1
    return (x, None) if want_row_sums else x


class _ZeroGradBias(torch.autograd.Function):
    """Identity on ``y`` that keeps a skipped bias in the graph: its gradient in front of an instance norm is zero."""

    @staticmethod
    def forward(ctx, y, bias):
        ctx.meta = (bias.dtype, tuple(bias.shape))
        return y.view_as(y)

    @staticmethod
    def backward(ctx, gy):
        return gy, torch.zeros(ctx.meta[1], dtype=ctx.meta[0], device=gy.device)


class InstanceNorm2d(nn.InstanceNorm2d):
    """``nn.InstanceNorm2d(affine=True, track_running_stats=False)`` as two HIP streaming passes
    (row sums, apply), optionally with the block's GELU fused into the apply pass."""

    def forward(self, x, fuse_gelu=False, row_sums=None):
        if self.track_running_stats or not ops.pointwise_supported(x):
            y = super().forward(x)
            return F.gelu(y) if fuse_gelu else y
        return ops.instance_norm(x, self.weight, self.bias, self.eps, fuse_gelu, row_sums=row_sums)


class Linear(nn.Linear):
    """``nn.Linear`` (same constructor, parameters and ``state_dict`` entries) on the ``mk_token_linear_*`` kernels under
    ``MK_TOKEN_LINEAR=hip`` and, for fp32 rows outside autocast, on the ``mk_token_linear_x3_*`` kernels under
    ``MK_TOKEN_LINEAR_FP32=hip`` (both read and validated on every call).  On the CPU, on inputs that ``ops.token_linear_supported``
    and ``ops.token_linear_x3_supported`` decline and with both knobs at ``torch`` it is exactly ``nn.Linear.forward``."""

    def forward(self, x):
        fp32_hip = ops.token_linear_fp32_hip()
        if ops.token_linear_hip() and ops.token_linear_supported(x, self.weight, self.bias):
            return ops.token_linear(x, self.weight, self.bias)
        if fp32_hip and ops.token_linear_x3_supported(x, self.weight, self.bias):
            return ops.token_linear(x, self.weight, self.bias)
        return super().forward(x)


class LayerNorm(nn.LayerNorm):
    """``nn.LayerNorm`` (same constructor, parameters and ``state_dict`` entries) over one or more trailing axes on the
    ``mk_token_layernorm_*`` kernels under ``MK_TOKEN_NORM=hip`` (read and validated on every call).  On the CPU, on inputs that
    ``ops.token_layer_norm_supported`` declines and with ``MK_TOKEN_NORM=torch`` it is exactly ``nn.LayerNorm.forward``."""

    def hip_ready(self, x):
        return ops.token_norm_hip() and ops.token_layer_norm_supported(x, self.normalized_shape, self.weight, self.bias)

    def forward(self, x):
        if not self.hip_ready(x):
            return super().forward(x)
        return ops.token_layer_norm(x, self.weight, self.bias, self.eps, normalized_shape=self.normalized_shape)

    def forward_add(self, x, residual=None, lowp=False, want_sum=False, out_dtype=None):
        """The norm of ``x + residual`` for callers that fuse: a tuple of ``y`` (``out_dtype``: as ``ops.token_layer_norm``), then
        its bf16 copy if ``lowp``, then the sum if ``want_sum``.  One launch on the HIP path; the torch formulation elsewhere."""
        if self.hip_ready(x) and (residual is None or (residual.shape == x.shape
                                                       and ops.token_layer_norm_supported(residual, self.normalized_shape))):
            out = ops.token_layer_norm(x, self.weight, self.bias, self.eps, residual, out_dtype, lowp, want_sum, self.normalized_shape)
            return out if isinstance(out, tuple) else (out,)
        s = x if residual is None else x + residual
        y = super().forward(s)
        if out_dtype is not None:
            y = y.to(out_dtype)
        return (y,) + ((y.to(torch.bfloat16),) if lowp else ()) + ((s,) if want_sum else ())


def drop_path(x, drop_prob=0.0, training=False):
    if drop_prob == 0.0 or not training:
        return x
    keep_prob = 1.0 - drop_prob
    shape = (x.shape[0],) + (1,) * (x.ndim - 1)
    random_tensor = keep_prob + torch.rand(shape, dtype=x.dtype, device=x.device)
    random_tensor.floor_()
    return x.div(keep_prob) * random_tensor


class DropPath(nn.Module):
    def __init__(self, drop_prob=None):
        super().__init__()
        self.drop_prob = drop_prob

    def forward(self, x):
        return drop_path(x, self.drop_prob, self.training)


class PatchEmbed(nn.Module):
    """layers.py:65-83: a strided convolution over non-overlapping patches, ``[B, C, H, W]`` -> ``[B, embed_dim, patches]``;
    ``forward_tokens`` gives the token-major form the patch networks consume, on HIP kernels under ``MK_PATCH=hip``."""

    def __init__(self, img_size=(224, 224), patch_size=(16, 16), in_chans=3, embed_dim=768):
        super().__init__()
        self.red_img_size = ((img_size[0] // patch_size[0]), (img_size[1] // patch_size[1]))
        self.img_size = img_size
        self.patch_size = patch_size
        self.num_patches = self.red_img_size[0] * self.red_img_size[1]
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size, bias=True)
        self.proj.weight.is_shared_mp = ["spatial"]
        self.proj.bias.is_shared_mp = ["spatial"]

    def forward(self, x):
        H, W = x.shape[-2], x.shape[-1]
        assert H == self.img_size[0] and W == self.img_size[1], \
            f"Input image size ({H}*{W}) doesn't match model ({self.img_size[0]}*{self.img_size[1]})."
        return self.proj(x).flatten(2)

    def forward_tokens(self, x, pos_embed=None):
        """The tokens ``[B, patches, embed_dim]`` (``+ pos_embed``): ``forward(x).transpose(1, 2)`` as both patch networks use it.
        Under ``MK_PATCH=hip`` (read and validated on every call), for what ``ops.patch_embed_supported`` takes -- an fp32 or bf16
        image under bf16 autocast, or bf16 image and parameters without it -- one ``ops.patch_embed`` node: ``mk_patchify`` and the token GEMM with the bias and
        the position add in its epilogue; an fp32 image outside autocast takes the same node on the fp32 kernels when
        ``MK_TOKEN_LINEAR_FP32=hip`` is set as well (``ops.patch_embed_x3_supported``).  Everything else is the convolution."""
        H, W = x.shape[-2], x.shape[-1]
        assert H == self.img_size[0] and W == self.img_size[1], \
            f"Input image size ({H}*{W}) doesn't match model ({self.img_size[0]}*{self.img_size[1]})."
        patch, fp32_hip = ops.patch_hip(), ops.token_linear_fp32_hip()
        if patch and (ops.patch_embed_supported(x, self.proj.weight, self.proj.bias)
                      or (fp32_hip and ops.patch_embed_x3_supported(x, self.proj.weight, self.proj.bias))):
            return ops.patch_embed(x, self.proj.weight, self.proj.bias, pos_embed)
        x = self.proj(x).flatten(2).transpose(1, 2)
        return x if pos_embed is None else x + pos_embed


class EncoderDecoder(nn.Module):
    """layers.py:86-133."""

    def __init__(self, num_layers, input_dim, output_dim, hidden_dim, act_layer, gain=1.0, input_format="nchw"):
        super().__init__()
        if input_format not in ("nchw", "traditional"):
            raise NotImplementedError(f"Error, input format {input_format} not supported.")
        mods = []
        current_dim = input_dim
        for _ in range(num_layers):
            if input_format == "nchw":
                mods.append(Conv1x1(current_dim, hidden_dim, bias=True))
            else:
                mods.append(Linear(current_dim, hidden_dim, bias=True))
            mods[-1].weight.is_shared_mp = ["spatial"]
            nn.init.normal_(mods[-1].weight, mean=0.0, std=math.sqrt(2.0 / current_dim))
            if mods[-1].bias is not None:
                mods[-1].bias.is_shared_mp = ["spatial"]
                nn.init.constant_(mods[-1].bias, 0.0)
            mods.append(act_layer())
            current_dim = hidden_dim
        if input_format == "nchw":
            mods.append(Conv1x1(current_dim, output_dim, bias=False))
        else:
            mods.append(Linear(current_dim, output_dim, bias=False))
        mods[-1].weight.is_shared_mp = ["spatial"]
        nn.init.normal_(mods[-1].weight, mean=0.0, std=math.sqrt(gain / current_dim))
        self.fwd = nn.Sequential(*mods)

    def forward(self, x):
        return run_pointwise_chain(self.fwd, x)


class MLP(nn.Module):
    """layers.py:136-216."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, output_bias=True,
                 input_format="nchw", drop_rate=0.0, drop_type="iid", checkpointing=0, gain=1.0, **kwargs):
        super().__init__()
        self.checkpointing = checkpointing
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        if input_format == "nchw":
            fc1 = Conv1x1(in_features, hidden_features, bias=True)
            fc1.weight.is_shared_mp = ["spatial"]
            fc1.bias.is_shared_mp = ["spatial"]
        elif input_format == "traditional":
            fc1 = Linear(in_features, hidden_features, bias=True)
        else:
            raise NotImplementedError(f"Error, input format {input_format} not supported.")
        nn.init.normal_(fc1.weight, mean=0.0, std=math.sqrt(2.0 / in_features))
        nn.init.constant_(fc1.bias, 0.0)
        act = act_layer()
        if (input_format == "traditional") and (drop_type == "features"):
            raise NotImplementedError("Error, traditional input format and feature dropout cannot be selected simultaneously")
        if input_format == "nchw":
            fc2 = Conv1x1(hidden_features, out_features, bias=output_bias)
            fc2.weight.is_shared_mp = ["spatial"]
            if output_bias:
                fc2.bias.is_shared_mp = ["spatial"]
        else:
            fc2 = Linear(hidden_features, out_features, bias=output_bias)
        nn.init.normal_(fc2.weight, mean=0.0, std=math.sqrt(gain / hidden_features))
        if fc2.bias is not None:
            nn.init.constant_(fc2.bias, 0.0)
        if drop_rate > 0.0:
            if drop_type == "iid":
                drop = nn.Dropout(drop_rate)
            elif drop_type == "features":
                drop = nn.Dropout2d(drop_rate)
            else:
                raise NotImplementedError(f"Error, drop_type {drop_type} not supported")
        else:
            drop = nn.Identity()
        self.fwd = nn.Sequential(fc1, act, drop, fc2, drop)

    def _run(self, x, skip_last_bias=False, want_row_sums=False, addend=None):
        return run_pointwise_chain(self.fwd, x, skip_last_bias, want_row_sums, addend)

    def checkpoint_forward(self, x, skip_last_bias=False, addend=None):
        return checkpoint(self._run, x, skip_last_bias, False, addend, use_reentrant=False)

    def forward(self, x, skip_last_bias=False, want_row_sums=False, addend=None):
        """``want_row_sums``: return ``(y, sums)`` -- see ``run_pointwise_chain``.  ``addend`` (traditional format only): return
        ``addend + mlp(x)``, the residual add of a transformer block, which the token kernels fold into ``fc2``."""
        if self.checkpointing >= 2:
            y = self.checkpoint_forward(x, skip_last_bias, addend)
            return (y, None) if want_row_sums else y
        return self._run(x, skip_last_bias, want_row_sums, addend)


# The HIP path is opt-in: the rule for the default is "not slower than the torch formulation at both grids of
# tools/fft2_bench.py", and at 384 x 240 x 480 `RealFFT2.forward` on fp32 rows is 11 % slower (every other row is faster, the
# full grid 5.6-9.7x): DESIGN section 19.
PLANAR_FFT_DEFAULT = "torch"


def planar_fft_hip():
    """The planar transforms run on this package's kernels: ``MK_PLANAR_FFT`` (``hip`` | ``torch``, read at call time), and
    the bf16x3 engine selected -- ``MK_SPECTRAL_GEMM=f32`` has no fp32-MFMA variant of the latitude DFT."""
    return ops._hip_or_torch("MK_PLANAR_FFT", PLANAR_FFT_DEFAULT) and ops.SPECTRAL_GEMM == "bf16x3"


class _PlanarFFT2Base(nn.Module):
    """Sizes of layers.py:219-287 plus what the HIP path needs: the latitude DFT table and the FFT twiddles as non-persistent
    buffers (no ``state_dict`` keys).  Sizes the kernels do not take (odd ``nlon``, ``lmax < 2``) get no buffers and stay on
    the torch formulation."""

    def __init__(self, nlat, nlon, lmax=None, mmax=None):
        super().__init__()
        self.nlat, self.nlon = nlat, nlon
        self.lmax = min(lmax or self.nlat, self.nlat)
        self.mmax = min(mmax or self.nlon // 2 + 1, self.nlon // 2 + 1)
        self.truncate = not ((self.lmax == self.nlat) and (self.mmax == (self.nlon // 2 + 1)))
        self.lmax_high = math.ceil(self.lmax / 2)
        self.lmax_low = math.floor(self.lmax / 2)
        self._hip_sizes = nlon % 2 == 0 and nlon >= 2 and self.lmax >= 2 and nlat >= 2
        if self._hip_sizes:
            self.register_buffer("twiddles", ops.fft_twiddles(nlon), persistent=False)
            self.register_buffer("dft_table", ops.latdft_table(nlat, self.lmax), persistent=False)

    def hip_ready(self, x):
        """The HIP path takes ``x``: a CUDA tensor next to CUDA buffers, sizes the kernels are built for, not switched off."""
        return self._hip_sizes and x.is_cuda and self.dft_table.is_cuda and planar_fft_hip()

    @staticmethod
    def _flatten(x, inner):
        lead = x.shape[:-2]
        bc = 1
        for s in lead:
            bc *= s
        return lead, x.reshape(bc, *inner)


class RealFFT2(_PlanarFFT2Base):
    """layers.py:219-250 -- the planar transform of ``spectral_transform="fft"``: real ``[..., nlat, nlon]`` -> complex
    ``[..., lmax, mmax]`` = ``rfft2(norm="ortho")`` truncated to the first ``ceil(lmax / 2)`` / last ``floor(lmax / 2)``
    latitude frequencies.  With ``MK_PLANAR_FFT=hip`` CUDA fp32 / bf16 inputs run on the HIP real FFT (``mk_rfft_ex``, scale ``1 / sqrt(nlon)``) and the
    MFMA latitude DFT (``mk_latdft_fwd``); everything else on the torch formulation (``_forward_torch``)."""

    def forward_packed(self, x3):
        """x3 [BC, nlat, nlon] (fp32 or bf16, contiguous) -> private spectrum [lmax, mmax, BC] (every entry is data: no triangle)."""
        xf = ops.rfft(x3, self.twiddles, self.mmax, True, scale=1.0 / math.sqrt(self.nlon))
        return ops.lat_dft(xf, self.dft_table, self.lmax)

    def forward_packed_fields(self, x4):
        """``RealSHT.forward_packed_fields`` for the planar spectrum: x4 [B, C, nlat, nlon] -> ``(spectrum, 0, 0)``."""
        return self.forward_packed(x4.reshape(-1, *x4.shape[-2:]).contiguous()), 0, 0

    def _forward_torch(self, x):
        y = torch.fft.rfft2(x, s=(self.nlat, self.nlon), dim=(-2, -1), norm="ortho")
        if self.truncate:
            y = torch.cat((y[..., : self.lmax_high, : self.mmax], y[..., -self.lmax_low:, : self.mmax]), dim=-2)
        return y

    def forward(self, x):
        if (x.dim() < 2 or x.dtype not in (torch.float32, torch.bfloat16) or tuple(x.shape[-2:]) != (self.nlat, self.nlon)
                or x.numel() == 0 or not self.hip_ready(x)):
            return self._forward_torch(x)
        lead, x3 = self._flatten(x.contiguous(), (self.nlat, self.nlon))
        c = ops.spec_unpack(self.forward_packed(x3), self.mmax, 0)       # degree offset mmax: dense, no triangle zeroed
        return c.reshape(*lead, self.lmax, self.mmax)


class InverseRealFFT2(_PlanarFFT2Base):
    """layers.py:253-287: complex ``[..., lmax, mmax]`` -> real ``[..., nlat, nlon]``, the zero padding between the high and
    the low latitude modes implicit in the kernel (``mk_latdft_inv``), then ``mk_irfft_ex`` with scale ``1 / sqrt(nlon)``."""

    def inverse_packed(self, c, out_dtype=torch.float32, want_row_sums=False):
        """private spectrum [lmax, mmax, BC] -> x [BC, nlat, nlon] (fp32, or bf16 rows straight from the FFT kernel); with
        ``want_row_sums`` (and a length the split kernels serve) also the fp64 ``[BC, 2]`` sums / sums of squares of the rows of x,
        else None in their place -- the conventions of ``InverseRealSHT.inverse_packed``."""
        s = 1.0 / math.sqrt(self.nlon)
        xf = ops.lat_idft(c, self.dft_table, self.nlat)
        if want_row_sums:
            if ops.irfft_sums_supported(self.nlon, self.mmax) and out_dtype in (torch.float32, torch.bfloat16):
                return ops.irfft(xf, self.twiddles, self.nlon, out_dtype, True, True, scale=s, exact_sums=True)
            return ops.irfft(xf, self.twiddles, self.nlon, out_dtype, True, scale=s), None
        return ops.irfft(xf, self.twiddles, self.nlon, out_dtype, True, scale=s)

    def _forward_torch(self, x):
        xt = x[..., : self.mmax]
        if self.truncate:
            xth = xt[..., : self.lmax_high, :]
            xtl = xt[..., -self.lmax_low:, :]
            xthp = F.pad(xth, (0, 0, 0, self.nlat - self.lmax))
            xt = torch.cat([xthp, xtl], dim=-2)
        return torch.fft.irfft2(xt, s=(self.nlat, self.nlon), dim=(-2, -1), norm="ortho")

    def forward(self, x):
        if (x.dim() < 2 or x.dtype != torch.complex64 or tuple(x.shape[-2:]) != (self.lmax, self.mmax) or x.numel() == 0
                or not self.hip_ready(x)):
            return self._forward_torch(x)
        lead, c3 = self._flatten(x.contiguous(), (self.lmax, self.mmax))
        y = self.inverse_packed(ops.spec_pack(c3, self.mmax, 0))
        return y.reshape(*lead, self.nlat, self.nlon)
