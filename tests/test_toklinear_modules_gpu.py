"""The modules on the token-major linear kernels against the torch path, both measured against a float64 CPU evaluation of the
same module: the traditional ``MLP``, ``Attention``, one ViT ``Block`` and a two-block ``VisionTransformer`` under bf16
autocast, with ``MK_TOKEN_LINEAR=hip`` and then ``torch`` on the same inputs and weights.

Criterion, for every output and every parameter and input gradient: the relative L2 error of the hip path is at most 1.5 times
that of the torch path plus 2^-9.  The torch path is the yardstick of the measurement, not the code under test; the margin covers
the two documented rounding differences (fp32 weight gradients, one rounding in the GELU gradient), which go in the accurate
direction, and the run-to-run noise of the vendor path."""
import copy
import gc

import pytest
import torch
import torch.nn as nn

from kernel_checks import node_kinds

pytestmark = pytest.mark.gpu

C, HEADS, B, N = 64, 4, 2, 200


def _build(name):
    from makani_amd import layers, vit
    torch.manual_seed(11)
    if name == "mlp":
        return layers.MLP(C, 4 * C, C, input_format="traditional"), (B, N, C)
    if name == "attention":
        return vit.Attention(C, num_heads=HEADS, qkv_bias=True), (B, N, C)
    if name == "block":
        return vit.Block(C, HEADS, qkv_bias=True), (B, N, C)
    net = vit.VisionTransformer(inp_shape=[28, 32], patch_size=(7, 8), inp_chans=3, out_chans=3, embed_dim=C, depth=2, num_heads=HEADS)
    with torch.no_grad():       # the head and the biases start at values that make every gradient non-trivial
        for p in net.parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))
    return net, (B, 3, 28, 32)


def _run(mod, x, g, autocast):
    x = x.clone().requires_grad_()
    params = [p for p in mod.parameters()]
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        y = mod(x)
    grads = torch.autograd.grad(y, [x] + params, g.to(y.dtype), allow_unused=True)
    return [y.detach()] + list(grads)


def _rel(got, want):
    return float((got.double().cpu() - want).norm() / want.norm())


@pytest.mark.parametrize("name", ["mlp", "attention", "block", "vit"])
def test_hip_path_is_as_accurate_as_the_torch_path(dev, name, monkeypatch):
    mod, shape = _build(name)
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(shape, generator=gen)
    ref_mod = copy.deepcopy(mod).double()
    x64 = x.double().requires_grad_()
    y64 = ref_mod(x64)
    g = torch.randn(y64.shape, generator=gen)
    want = [y64.detach()] + list(torch.autograd.grad(y64, [x64] + list(ref_mod.parameters()), g.double(), allow_unused=True))
    names = ["output", "input gradient"] + [n for n, _ in mod.named_parameters()]

    mod = mod.to(dev)
    got = {}
    for mode in ("hip", "torch"):
        monkeypatch.setenv("MK_TOKEN_LINEAR", mode)
        got[mode] = _run(mod, x.to(dev), g.to(dev), True)
    worst = 0.0
    for n, h, t, w in zip(names, got["hip"], got["torch"], want):
        if w is None:
            assert h is None and t is None
            continue
        eh, et = _rel(h, w), _rel(t, w)
        worst = max(worst, eh / (1.5 * et + 2.0 ** -9))
        print(f"{name} {n}: hip {eh:.3e} torch {et:.3e} ratio {eh / et if et else float('inf'):.3f}")
        assert eh <= 1.5 * et + 2.0 ** -9, f"{name} {n}: hip {eh:.3e} against torch {et:.3e}"
    print(f"{name}: worst error / allowance {worst:.3f}")


def test_hip_path_runs_the_kernels(dev, monkeypatch):
    """Under the knob the block's linears are the package's autograd functions: the node names of the graph say so."""
    monkeypatch.setenv("MK_TOKEN_LINEAR", "hip")
    mod, shape = _build("block")
    mod = mod.to(dev)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = mod(torch.randn(shape, device=dev))
    kinds = node_kinds(y)
    assert sum(k.startswith("_TokenLinear") for k in kinds) == 2 and sum(k.startswith("_TokenMLP") for k in kinds) == 1
    assert not any("Addmm" in k or "MmBackward" in k for k in kinds), kinds


def test_unsupported_inputs_take_the_torch_call(dev, monkeypatch):
    from makani_amd import layers, ops
    monkeypatch.setenv("MK_TOKEN_LINEAR", "hip")
    torch.manual_seed(3)
    for (i, o), dtype, autocast in (((64, 128), torch.float32, False), ((60, 128), torch.bfloat16, False), ((64, 124), torch.float32, True)):
        ref = nn.Linear(i, o).to(dev)
        mine = layers.Linear(i, o).to(dev)
        mine.load_state_dict(ref.state_dict(), strict=True)
        if dtype == torch.bfloat16:
            ref, mine = ref.to(dtype), mine.to(dtype)
        x = torch.randn(3, 50, i, device=dev, dtype=dtype)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            assert not ops.token_linear_supported(x, mine.weight, mine.bias)
            xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
            ya, yb = ref(xa), mine(xb)
        assert torch.equal(ya, yb)
        g = torch.randn_like(ya)
        for a, b in zip(torch.autograd.grad(ya, [xa] + list(ref.parameters()), g), torch.autograd.grad(yb, [xb] + list(mine.parameters()), g)):
            assert torch.equal(a, b)


def test_the_addend_alone_can_ask_for_a_gradient(dev, monkeypatch):
    """Frozen weights and a detached input: the addend's gradient is the incoming gradient, and nothing else is computed."""
    from makani_amd import ops
    monkeypatch.setenv("MK_TOKEN_LINEAR", "hip")
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(2, 40, 64, generator=gen).to(dev).bfloat16()
    w1, w2 = torch.randn(128, 64, generator=gen).to(dev), torch.randn(64, 128, generator=gen).to(dev)
    for out_features, call in ((128, lambda a: ops.token_linear(x, w1, None, addend=a)), (64, lambda a: ops.token_mlp(x, w1, None, w2, None, addend=a))):
        a = torch.randn(2, 40, out_features, generator=gen).to(dev).requires_grad_()
        g = torch.randn(2, 40, out_features, generator=gen).to(dev)
        out = call(a)
        assert out.dtype == torch.float32 and type(out.grad_fn).__name__.startswith("_Token")
        (ga,) = torch.autograd.grad(out, [a], g)
        assert torch.equal(ga, g)


def test_captured_mlp_step_replays_the_eager_bits(dev, monkeypatch):
    """One forward + backward of the MLP captured on a single stream and replayed twice equals the eager run bit for bit."""
    monkeypatch.setenv("MK_TOKEN_LINEAR", "hip")
    mod, shape = _build("mlp")
    mod = mod.to(dev)
    params = list(mod.parameters())
    gen = torch.Generator().manual_seed(9)
    x, g = torch.randn(shape, generator=gen).to(dev), torch.randn(shape, generator=gen).to(dev)

    def step(inp):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = mod(inp, addend=inp)
        return [y] + list(torch.autograd.grad(y, [inp] + params, g))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        static = x.clone().requires_grad_()
        eager = [t.detach().clone() for t in step(static)]
        step(static)                                                    # a second warm-up on the capture stream
        gc.collect()
        torch.cuda.empty_cache()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            outs = step(static)
        for _ in range(2):
            graph.replay()
            side.synchronize()
            for a, b in zip(outs, eager):
                assert torch.equal(a.detach(), b)
    torch.cuda.current_stream().wait_stream(side)
