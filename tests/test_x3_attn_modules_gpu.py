"""The fp32 attention path (``MK_ATTN_FP32=hip``, no autocast) through ``ops.attention``, ``ops.attention_packed`` and the ViT
modules, against a float64 CPU copy of the same computation.

Criterion, for the output and for EVERY parameter and input gradient: the worst relative L2 error of a row (``row_rel``) of the
hip path is at most 4 times that of the torch fp32 path on the same inputs and weights, computed in the same test.  The factor
is the one of tests/test_x3_toklinear_modules_gpu.py for two chained products: ``X3_C / F32_C`` of tests/kernel_checks.py
rounded up to 2, doubled.  Both numbers are printed."""
import copy

import numpy as np
import pytest
import torch

import kernel_checks as kc
from kernel_checks import node_kinds as _node_kinds

pytestmark = pytest.mark.gpu

C, HEADS, B, N = 64, 4, 2, 150          # D = 16; 150 tokens: two query tiles of the forward, a ragged last tile everywhere
FACTOR = 4.0
SDPA = torch.nn.functional.scaled_dot_product_attention


class _Op(torch.nn.Module):
    """``ops.attention_packed`` / ``ops.attention`` on a ``[B, N, 3 H D]`` input, as a module without parameters."""

    def __init__(self, packed, heads):
        super().__init__()
        self.packed, self.heads = packed, heads

    def forward(self, x):
        from makani_amd import ops
        Bx, Nx, C3 = x.shape
        if self.packed:
            return ops.attention_packed(x, self.heads)
        q, k, v = (t.permute(0, 2, 1, 3) for t in x.view(Bx, Nx, 3, self.heads, C3 // (3 * self.heads)).unbind(2))
        return ops.attention(q, k, v).transpose(1, 2).reshape(Bx, Nx, C3 // 3)


def _build(name):
    from makani_amd import vit
    torch.manual_seed(11)
    if name in ("attention", "attention_packed"):
        return _Op(name == "attention_packed", HEADS), (B, N, 3 * C)
    if name in ("module", "module_qk_norm"):
        mod = vit.Attention(C, num_heads=HEADS, qkv_bias=True, qk_norm=name == "module_qk_norm")
        with torch.no_grad():
            mod.qkv.weight.mul_(4.0)                       # scores with a standard deviation of order 1, not a mean
        return mod, (B, N, C)
    if name == "block":
        return vit.Block(C, HEADS, qkv_bias=True), (B, N, C)
    net = vit.VisionTransformer(inp_shape=[16, 32], patch_size=(2, 2), inp_chans=3, out_chans=3, embed_dim=C, depth=2, num_heads=HEADS)
    with torch.no_grad():       # the head and the biases start at values that make every gradient non-trivial
        for p in net.parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))
    return net, (B, 3, 16, 32)


def _run(mod, x, g, autocast=False):
    x = x.clone().requires_grad_()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        y = mod(x)
    grads = torch.autograd.grad(y, [x] + list(mod.parameters()), g.to(y.dtype), allow_unused=True)
    return [y.detach()] + list(grads)


def _worst_row(got, want):
    g, w = got.double().cpu().numpy(), want.numpy()
    g, w = g.reshape(-1, g.shape[-1]), w.reshape(-1, w.shape[-1])
    keep = np.sqrt((w ** 2).sum(-1)) > 0          # a row whose exact gradient is zero has no relative error
    return float(kc.row_rel(g[keep], w[keep]).max())


def _reference(mod, x, gen):
    ref_mod = copy.deepcopy(mod).double()
    x64 = x.double().requires_grad_()
    y64 = ref_mod(x64)
    g = torch.randn(y64.shape, generator=gen)
    want = [y64.detach()] + list(torch.autograd.grad(y64, [x64] + list(ref_mod.parameters()), g.double(), allow_unused=True))
    return g, want


@pytest.mark.parametrize("name", ["attention", "attention_packed", "module", "module_qk_norm", "block", "vit"])
def test_hip_path_is_as_accurate_as_the_torch_path(dev, name, monkeypatch):
    monkeypatch.setenv("MK_ATTN_FP32", "torch")
    mod, shape = _build(name)
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(shape, generator=gen)
    g, want = _reference(mod, x, gen)
    names = ["output", "input gradient"] + [n for n, _ in mod.named_parameters()]
    mod = mod.to(dev)
    got = {}
    for mode in ("hip", "torch"):
        monkeypatch.setenv("MK_ATTN_FP32", mode)
        got[mode] = _run(mod, x.to(dev), g.to(dev))
    worst, failures = 0.0, []
    for n, h, t, w in zip(names, got["hip"], got["torch"], want):
        if w is None:
            assert h is None and t is None
            continue
        assert h.dtype == torch.float32
        if n.endswith("k_norm.bias"):
            # a constant added to every key shifts all scores of a row alike and leaves the softmax unchanged: this gradient is
            # exactly zero (the float64 value is its own rounding noise); the errors are measured against the weight's gradient
            w = want[names.index(n[:-4] + "weight")].norm() * torch.ones_like(w)
            h, t = h.cpu().double() + w, t.cpu().double() + w
        eh, et = _worst_row(h, w), _worst_row(t, w)
        worst = max(worst, eh / et if et else float("inf"))
        print(f"[x3 attn modules] {name} {n}: hip {eh:.3e} torch {et:.3e} ratio {eh / et if et else float('inf'):.3f}")
        if not eh <= FACTOR * et:
            failures.append(f"{n}: hip {eh:.3e} against torch {et:.3e}")
    print(f"[x3 attn modules] {name}: worst hip / torch {worst:.3f} (limit {FACTOR})")
    assert not failures, f"{name}: " + "; ".join(failures)


def test_hip_path_runs_the_kernels(dev, monkeypatch):
    """Under the knob the attention of the modules is the package's fp32 autograd function: the node names of the graph say so."""
    for mode in ("hip", "torch"):
        monkeypatch.setenv("MK_ATTN_FP32", mode)
        for name, packed, plain in (("attention", 0, 1), ("attention_packed", 1, 0), ("module", 1, 0), ("module_qk_norm", 0, 1),
                                    ("block", 1, 0), ("vit", 2, 0)):
            mod, shape = _build(name)
            kinds = _node_kinds(mod.to(dev)(torch.randn(shape, device=dev).requires_grad_()))
            n_packed = sum(k.startswith("_AttentionPackedX3") for k in kinds)
            n_plain = sum(k.startswith("_AttentionX3") for k in kinds)
            assert (n_packed, n_plain) == ((packed, plain) if mode == "hip" else (0, 0)), (mode, name, kinds)
            if mode == "hip":
                assert not any("ScaledDotProduct" in k or k.startswith(("SoftmaxBackward", "BmmBackward")) for k in kinds), (name, kinds)


@pytest.mark.parametrize("setting", ["knob at torch", "bf16 autocast", "MK_SPECTRAL_GEMM=f32", "declined head size", "head size 128",
                                     "dropout"])
@pytest.mark.parametrize("packed", [True, False])
def test_everything_else_is_the_torch_call_bit_for_bit(dev, setting, packed, monkeypatch):
    from makani_amd import ops
    monkeypatch.setenv("MK_ATTN_FP32", "torch" if setting == "knob at torch" else "hip")
    monkeypatch.setenv("MK_ATTN", "torch")           # under autocast the bf16 kernels would take the call: not what is compared
    if setting == "MK_SPECTRAL_GEMM=f32":
        monkeypatch.setattr(ops, "SPECTRAL_GEMM", "f32")
    autocast = setting == "bf16 autocast"
    D = {"declined head size": 24, "head size 128": 128}.get(setting, 16)
    p = 0.25 if setting == "dropout" else 0.0
    H = 2
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(B, 70, 3 * H * D, generator=gen).to(dev)
    g = torch.randn(B, 70, H * D, generator=gen).to(dev)

    def run(ours):
        leaf = x.clone().requires_grad_()
        torch.manual_seed(9)                          # the dropout mask
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            if ours and packed:
                y = ops.attention_packed(leaf, H, dropout_p=p)
            else:
                q, k, v = (t.permute(0, 2, 1, 3) for t in leaf.reshape(B, 70, 3, H, D).unbind(2))
                o = ops.attention(q, k, v, dropout_p=p) if ours else SDPA(q, k, v, dropout_p=p)
                y = o.transpose(1, 2).reshape(B, 70, H * D)
        assert not any(k.startswith("_Attention") for k in _node_kinds(y))
        (gx,) = torch.autograd.grad(y, [leaf], g.to(y.dtype))
        return y.detach(), gx

    (y, gx), (y0, gx0) = run(True), run(False)
    assert y.dtype == y0.dtype and torch.equal(y, y0) and torch.equal(gx, gx0)


def test_grad_mode_off_allocates_no_lse(dev, monkeypatch):
    from makani_amd import ops
    monkeypatch.setenv("MK_ATTN_FP32", "hip")
    seen, orig = [], ops.attn_x3_fwd_raw

    def fwd(q, k, v, o, lse, scale):
        seen.append(lse is not None)
        return orig(q, k, v, o, lse, scale)

    monkeypatch.setattr(ops, "attn_x3_fwd_raw", fwd)
    mod, shape = _build("module")
    mod, x = mod.to(dev), torch.randn(shape, device=dev)
    y1 = mod(x)
    with torch.no_grad():
        y0 = mod(x)
    mod.requires_grad_(False)
    y2 = mod(x)                                       # grad mode on, nothing requires a gradient
    assert seen == [True, False, False]
    assert torch.equal(y0, y1.detach()) and torch.equal(y2, y0)


def test_attention_module_in_a_graph(dev, monkeypatch):
    """Forward and backward of one ``Attention`` captured with ``torch.cuda.graph`` after warm-up on a side stream; the replay
    on new data is bit-equal to the eager run on the same data."""
    monkeypatch.setenv("MK_ATTN_FP32", "hip")
    mod, shape = _build("module")
    mod = mod.to(dev)
    gen = torch.Generator().manual_seed(7)
    data, gs = torch.randn(shape, generator=gen).to(dev), torch.randn(shape, generator=gen).to(dev)
    xs = torch.zeros(shape, device=dev).requires_grad_(True)
    warm = torch.randn_like(xs)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.no_grad():
            xs.copy_(warm)
        for _ in range(3):
            mod.zero_grad(set_to_none=True)
            xs.grad = None
            mod(xs).backward(gs)
    torch.cuda.current_stream().wait_stream(side)
    mod.zero_grad(set_to_none=True)
    xs.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ys = mod(xs)
        assert any(k.startswith("_AttentionPackedX3") for k in _node_kinds(ys))
        ys.backward(gs)
    with torch.no_grad():
        xs.copy_(data)
    graph.replay()
    torch.cuda.synchronize()
    got = [ys.detach().clone(), xs.grad.clone()] + [p.grad.clone() for p in mod.parameters()]
    mod.zero_grad(set_to_none=True)
    want = _run(mod, data, gs)
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b)
