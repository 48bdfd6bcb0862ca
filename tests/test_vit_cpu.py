"""The ViT modules on the CPU against ``tests/golden/ref_vit.npz``, the recorded run of the reference's own ``vit.py``
(``tests/golden/make_vit_golden.py``; ``qkv.weight`` drawn there so that the scaled scores have a standard deviation of 2.5-2.7:
the softmax is far from a mean).

On CPU tensors the modules run the reference's own op sequence (``nn.Linear``, ``F.scaled_dot_product_attention`` on the same
permuted views, ``nn.LayerNorm``, the MLP's linear - GELU - linear), so the output and every gradient are required to be
bit-equal to the recording where that holds on the machine at hand and otherwise within 1e-6 relative L2: the BLAS behind
``nn.Linear`` may block a product differently with another thread count, which is an fp32 rounding, not an error.  The test
prints which of the two it met."""
import os

import numpy as np
import pytest
import torch

BOUND = 1e-6
NET_KW = dict(inp_shape=[21, 40], patch_size=(7, 8), inp_chans=3, out_chans=2, embed_dim=64, depth=2, num_heads=2, mlp_ratio=1.0)


@pytest.fixture(scope="module")
def ref(golden_dir):
    with np.load(os.path.join(golden_dir, "ref_vit.npz")) as z:
        return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return (torch.linalg.norm(a - b) / torch.linalg.norm(b)).item()


def build(ref):
    from makani_amd.vit import VisionTransformer
    net = VisionTransformer(**NET_KW)
    state = {k[len("state."):]: v for k, v in ref.items() if k.startswith("state.")}
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == {k: tuple(v.shape) for k, v in state.items()}
    net.load_state_dict(state, strict=True)
    return net


def run(ref, net, dev="cpu"):
    """forward + backward on the recorded input and cotangent -> (y, {name: gradient}) with the input gradient as ``x``."""
    net.zero_grad(set_to_none=True)
    x = ref["x"].to(dev).requires_grad_(True)
    y = net(x)
    y.backward(ref["g"].to(dev).to(y.dtype))
    grads = {"x": x.grad}
    grads.update({n: p.grad for n, p in net.named_parameters()})
    return y, grads


def wanted(ref, name):
    return ref["gx"] if name == "x" else ref["grad." + name]


def test_state_dict_keys_and_attributes(ref):
    net = build(ref)
    keys = set(net.state_dict())
    for k in ("patch_embed.proj.weight", "pos_embed", "blocks.0.attn.qkv.weight", "blocks.0.attn.qkv.bias", "blocks.1.attn.proj.bias",
              "blocks.0.norm1.weight", "blocks.1.norm2.bias", "blocks.0.mlp.fwd.0.weight", "blocks.1.mlp.fwd.3.bias", "norm.weight",
              "head.weight"):
        assert k in keys, k
    assert "head.bias" not in keys
    assert net.pos_embed.is_shared_mp == []
    assert (net.embed_dim, net.num_features, net.out_ch, net.out_size, net.patch_embed.num_patches) == (64, 64, 2, 112, 15)
    a = net.blocks[0].attn
    assert (a.num_heads, a.head_dim, a.scale, a.attn_drop_rate) == (2, 32, 32 ** -0.5, 0.0)
    assert isinstance(a.q_norm, torch.nn.Identity) and isinstance(a.proj_drop, torch.nn.Identity)
    assert isinstance(net.blocks[0].drop_path, torch.nn.Identity)
    assert 1.0 < float(ref["score_std"].min()) and float(ref["score_std"].max()) < 3.0


def test_forward_and_gradients_against_the_reference_run(ref):
    net = build(ref)
    y, grads = run(ref, net)
    assert y.shape == ref["y"].shape
    errs = {"y": rel(y, ref["y"])}
    exact = [torch.equal(y.detach(), ref["y"])]
    for n, g in grads.items():
        assert g is not None and g.shape == wanted(ref, n).shape, n
        errs[n] = rel(g, wanted(ref, n))
        exact.append(torch.equal(g, wanted(ref, n)))
    worst = max(errs, key=errs.get)
    print(f"[vit] cpu: {sum(exact)} of {len(exact)} tensors bit-equal to the recording; worst {worst} {errs[worst]:.2e}")
    assert errs[worst] <= BOUND, (worst, errs[worst])


def test_qk_norm_and_dropout_variants():
    from makani_amd.vit import Attention, Block
    torch.manual_seed(0)
    a = Attention(32, num_heads=2, qkv_bias=True, qk_norm=True, proj_drop_rate=0.1)
    assert isinstance(a.q_norm, torch.nn.LayerNorm) and a.q_norm.normalized_shape == (16,) and isinstance(a.proj_drop, torch.nn.Dropout)
    a.eval()
    x = torch.randn(2, 5, 32)
    F = torch.nn.functional
    qkv = a.qkv(x).reshape(2, 5, 3, 2, 16).permute(2, 0, 3, 1, 4).double()
    q = F.layer_norm(qkv[0], (16,), a.q_norm.weight.double(), a.q_norm.bias.double(), a.q_norm.eps)
    k = F.layer_norm(qkv[1], (16,), a.k_norm.weight.double(), a.k_norm.bias.double(), a.k_norm.eps)
    p = torch.softmax(q @ k.transpose(-1, -2) / 4.0, -1)
    want = F.linear((p @ qkv[2]).transpose(1, 2).reshape(2, 5, 32), a.proj.weight.double(), a.proj.bias.double())
    assert rel(a(x), want) <= 2e-6
    b = Block(32, 2, mlp_ratio=2.0, attn_drop_rate=0.5, path_drop_rate=0.2)
    assert b.attn.attn_drop_rate == 0.5 and b.drop_path.drop_prob == 0.2
    b.eval()
    assert torch.equal(b(x), b(x))                  # neither dropout acts at inference
    b.train()
    assert b(x).shape == x.shape


def test_matmul_parallel_groups_are_refused(monkeypatch):
    from makani_amd import comm
    from makani_amd.vit import Block, VisionTransformer
    monkeypatch.setattr(comm, "get_size", lambda name: 2 if name == "fin" else 1)
    with pytest.raises(NotImplementedError):
        VisionTransformer(**NET_KW)
    with pytest.raises(NotImplementedError):
        Block(32, 2)
    with pytest.raises(NotImplementedError):
        monkeypatch.setattr(comm, "get_size", lambda name: 1)
        VisionTransformer(**dict(NET_KW, norm_layer="instance_norm"))
