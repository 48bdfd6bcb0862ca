"""The ViT network (``nettype: "ViT"``, networks/vit.py): ``Attention``, ``Block`` and ``VisionTransformer`` with the reference's
constructor signatures, attributes and ``state_dict`` keys.

The attention product -- at the 18 540 tokens of ``config/vit.yaml`` nearly all of a block's arithmetic -- runs on the
``mk_attn_*`` kernels (csrc/attn.hip) under ``MK_ATTN=hip`` (read and validated on every call; default ``ops.ATTN_DEFAULT``):

* ``qk_norm`` off: ``ops.attention_packed`` reads q, k and v in place from the ``qkv`` projection's output ``[B, N, 3, H, D]``,
  writes the output token-major ``[B, N, H D]`` and returns one gradient tensor for the projection: no permuted copy, no cat;
* ``qk_norm`` on: ``ops.attention`` on the normalised ``[B, H, N, D]`` views.

fp32 activations without autocast (the reference's ``amp_mode none``) reach, through the same two functions, the ``mk_attn_x3_*``
kernels (csrc/x3_attn.hip) under ``MK_ATTN_FP32=hip`` (read and validated on every call; default ``ops.ATTN_FP32_DEFAULT``): fp32
operands, output and lse, every matrix product on the bf16x3 arithmetic of the spectral engine, head sizes that are multiples of
16 up to 64, and ``MK_SPECTRAL_GEMM=bf16x3``.

fp16 activations, fp32 ones with ``MK_ATTN_FP32=torch``, CPU tensors, head sizes that are no multiple of 16 in 16 ... 128 (bf16) or
16 ... 64 (fp32), attention dropout in training and ``MK_ATTN=torch`` take ``F.scaled_dot_product_attention``, the reference's call.

The norms of the blocks (``norm1``, ``norm2``) and the final ``norm`` are ``layers.LayerNorm``: under ``MK_TOKEN_NORM=hip`` (read
and validated on every call; default ``ops.TOKEN_NORM_DEFAULT``) they run on the ``mk_token_layernorm_*`` kernels
(csrc/toknorm.hip), and a block fuses what surrounds them: under bf16 autocast ``norm1`` writes only the bf16 operand of ``qkv``,
and ``norm2`` is one launch for ``x + drop_path(attn)``, the norm, its fp32 result for the residual and the bf16 operand of
``fc1`` (the sum is not stored; the backward recomputes it) -- the rounding points of the torch path under autocast.  Without
autocast there is one output in the tokens' dtype.  ``q_norm`` / ``k_norm`` stay ``nn.LayerNorm`` in torch: they act on strided
head views ``[B, H, N, D]`` of the projection output, whose rows the kernels do not take.

The linears -- ``qkv``, ``proj``, the two of the MLP and ``head`` -- are ``layers.Linear``: under ``MK_TOKEN_LINEAR=hip`` (read and
validated on every call; default ``ops.TOKEN_LINEAR_DEFAULT``) with bf16 tokens or bf16 autocast they run on the
``mk_token_linear_*`` kernels (csrc/toklinear.hip).  The MLP is one autograd node (``ops.token_mlp``): the GELU in ``fc1``'s epilogue,
the block's residual add in ``fc2``'s (when ``drop_path`` is an identity; with stochastic depth the block keeps the separate add)
and the GELU gradient in the epilogue of ``fc2``'s data gradient.  Weight gradients are accumulated and returned in fp32.  fp32
tokens without autocast, feature counts that are no multiple of 8, CPU tensors and ``MK_TOKEN_LINEAR=torch`` take ``F.linear``.

Patch embedding and the un-patchify behind ``head`` run on the layout passes of csrc/patch.hip under ``MK_PATCH=hip`` (read and
validated on every call; default ``ops.PATCH_DEFAULT``): ``PatchEmbed.forward_tokens`` is ``mk_patchify`` to bf16 patch rows and the
token GEMM with the convolution's bias and the position add in its epilogue (bf16 images, or bf16 autocast; an fp32 run keeps
``nn.Conv2d``), ``forward_head`` ends in one ``mk_unpatchify`` pass (fp32 and bf16).  ``MK_PATCH=torch`` and CPU tensors take the
convolution and torch's permuted copy.

Out of scope: ``DistributedAttention`` / ``DistributedMLP`` / ``DistributedMatmul`` -- matmul group sizes (``fin``, ``fout``) above 1
raise ``NotImplementedError``; data parallelism works as for any module.
"""
import torch
import torch.nn as nn

try:
    from . import comm, ops
except ImportError:     # loaded by file path (the reference's registry: ``nettype: ".../makani_amd/vit.py:Name"``), no package
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from makani_amd import comm, ops
from makani_amd.layers import MLP, DropPath, LayerNorm, Linear, PatchEmbed


def _matmul_parallel(comm_inp_name, comm_hidden_name):
    return comm.get_size(comm_inp_name) * comm.get_size(comm_hidden_name) > 1


class Attention(nn.Module):
    """vit.py:14-55: multi-head self-attention on ``[B, N, C]`` tokens; ``qkv`` and ``proj`` are ``layers.Linear``.  The product is
    ``ops.attention_packed`` (``qk_norm`` off) or ``ops.attention`` (on): bf16 operands on the ``mk_attn_*`` kernels under
    ``MK_ATTN=hip``, fp32 operands outside autocast on the ``mk_attn_x3_*`` kernels under ``MK_ATTN_FP32=hip``, else torch's call."""

    def __init__(self, dim, input_format="traditional", num_heads=8, qkv_bias=False, qk_norm=False, attn_drop_rate=0.0,
                 proj_drop_rate=0.0, norm_layer=nn.LayerNorm):
        super().__init__()
        if dim % num_heads != 0:
            raise AssertionError("dim should be divisible by num_heads")
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.qkv = Linear(dim, 3 * dim, bias=qkv_bias)
        self.q_norm = norm_layer(self.head_dim) if qk_norm else nn.Identity()
        self.k_norm = norm_layer(self.head_dim) if qk_norm else nn.Identity()
        self.attn_drop_rate = attn_drop_rate
        self.proj = Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop_rate) if proj_drop_rate > 0 else nn.Identity()

    def forward(self, x):
        B, N, C = x.shape
        H, D = self.num_heads, self.head_dim
        # attention dropout acts in training only (the reference passes dropout_p whatever the mode, vit.py:50, which drops
        # weights at inference too); with it the product takes the torch formulation
        p = self.attn_drop_rate if self.training else 0.0
        qkv = self.qkv(x)
        if isinstance(self.q_norm, nn.Identity) and isinstance(self.k_norm, nn.Identity):
            y = ops.attention_packed(qkv, H, dropout_p=p)
        else:
            q, k, v = qkv.reshape(B, N, 3, H, D).permute(2, 0, 3, 1, 4).unbind(0)
            y = ops.attention(self.q_norm(q), self.k_norm(k), v, dropout_p=p).transpose(1, 2).reshape(B, N, C)
        return self.proj_drop(self.proj(y))


class Block(nn.Module):
    """vit.py:58-120: ``x + attn(norm1(x))``, then ``norm2`` of that and ``+ mlp`` of it (the reference adds the MLP to the
    NORMALISED tokens, vit.py:117-118; kept)."""

    def __init__(self, dim, num_heads, mlp_ratio=4.0, qkv_bias=False, mlp_drop_rate=0.0, attn_drop_rate=0.0, path_drop_rate=0.0,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm, comm_inp_name="fin", comm_hidden_name="fout"):
        super().__init__()
        if _matmul_parallel(comm_inp_name, comm_hidden_name):
            raise NotImplementedError("ViT runs data parallel only: no DistributedAttention / DistributedMLP")
        self.attn = Attention(dim, input_format="traditional", num_heads=num_heads, qkv_bias=qkv_bias,
                              attn_drop_rate=attn_drop_rate, proj_drop_rate=mlp_drop_rate, norm_layer=norm_layer)
        self.drop_path = DropPath(path_drop_rate) if path_drop_rate > 0.0 else nn.Identity()
        block_norm = LayerNorm if norm_layer is nn.LayerNorm else norm_layer
        self.norm1 = block_norm(dim)
        self.norm2 = block_norm(dim)
        self.mlp = MLP(in_features=dim, hidden_features=int(dim * mlp_ratio), out_features=dim, act_layer=act_layer,
                       drop_rate=mlp_drop_rate, input_format="traditional")

    def _fused_norms(self, x):
        return all(isinstance(n, LayerNorm) and n.hip_ready(x) for n in (self.norm1, self.norm2))

    def _add_mlp(self, x, h):
        """``x + drop_path(mlp(h))``; without stochastic depth the add is the MLP's (``fc2``'s epilogue on the token kernels)."""
        if isinstance(self.drop_path, nn.Identity):
            return self.mlp(h, addend=x)
        return x + self.drop_path(self.mlp(h))

    def forward(self, x):
        if not self._fused_norms(x):
            x = x + self.drop_path(self.attn(self.norm1(x)))
            x = self.norm2(x)
            return self._add_mlp(x, x)
        if torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16:
            # norm1's one consumer is qkv, which takes bf16; fc1 takes norm2's bf16 copy, the residual its fp32 result
            (h,) = self.norm1.forward_add(x, out_dtype=torch.bfloat16)
            x, h = self.norm2.forward_add(self.drop_path(self.attn(h)), x, lowp=True)
            return self._add_mlp(x, h)
        (x,) = self.norm2.forward_add(self.drop_path(self.attn(self.norm1(x))), x)
        return self._add_mlp(x, x)


class VisionTransformer(nn.Module):
    """vit.py:123-231: patch embedding, learned position embedding, ``depth`` blocks, a final norm and a linear head that
    writes each token's ``patch_size[0] x patch_size[1] x out_chans`` patch."""

    def __init__(self, inp_shape=[224, 224], patch_size=(16, 16), inp_chans=3, out_chans=3, embed_dim=768, depth=12, num_heads=12,
                 mlp_ratio=4.0, qkv_bias=True, mlp_drop_rate=0.0, attn_drop_rate=0.0, path_drop_rate=0.0, norm_layer="layer_norm",
                 comm_inp_name="fin", comm_hidden_name="fout", **kwargs):
        super().__init__()
        if _matmul_parallel(comm_inp_name, comm_hidden_name):
            raise NotImplementedError("ViT runs data parallel only: no matmul model parallelism")
        if norm_layer != "layer_norm":
            raise NotImplementedError(f"Error, normalization layer type {norm_layer} not implemented for ViT.")
        self.num_features = self.embed_dim = embed_dim
        self.patch_size = patch_size
        self.img_size = inp_shape
        self.out_ch = out_chans
        self.comm_inp_name = comm_inp_name
        self.comm_hidden_name = comm_hidden_name

        self.patch_embed = PatchEmbed(img_size=self.img_size, patch_size=patch_size, in_chans=inp_chans, embed_dim=embed_dim)
        self.pos_embed = nn.Parameter(torch.zeros(1, self.patch_embed.num_patches, embed_dim))
        self.pos_embed.is_shared_mp = []
        self.pos_drop = nn.Dropout(p=path_drop_rate)
        rates = [r.item() for r in torch.linspace(0, path_drop_rate, depth)]      # stochastic depth grows with the layer
        self.blocks = nn.ModuleList([
            Block(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, mlp_drop_rate=mlp_drop_rate,
                  attn_drop_rate=attn_drop_rate, path_drop_rate=rates[i], norm_layer=nn.LayerNorm, comm_inp_name=comm_inp_name,
                  comm_hidden_name=comm_hidden_name) for i in range(depth)])
        self.norm = LayerNorm(embed_dim)
        self.out_size = self.out_ch * self.patch_size[0] * self.patch_size[1]
        self.head = Linear(embed_dim, self.out_size, bias=False)

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

    def prepare_tokens(self, x):
        return self.pos_drop(self.patch_embed.forward_tokens(x, self.pos_embed))          # [B, N, embed_dim]

    def forward_head(self, x):
        B = x.shape[0]
        h, w = self.patch_embed.red_img_size
        ph, pw = self.patch_size
        x = self.head(x.reshape(B, h, w, self.embed_dim))           # features (p, q, c): "nhwpqc->nchpwq" is order 1
        return ops.unpatchify(x, self.patch_size, self.out_ch, self.img_size, order=1)

    def forward(self, x):
        x = self.prepare_tokens(x)
        for blk in self.blocks:
            x = blk(x)
        return self.forward_head(self.norm(x))
