"""The modules on the fp32 token-major linear kernels (``MK_TOKEN_LINEAR_FP32=hip``, no autocast) against a float64 CPU copy of
the same module: ``layers.Linear`` with and without bias, the traditional ``MLP``, the AFNOv1 ``Mlp``, one ViT ``Block`` and a
two-block ``VisionTransformer`` (both ``MK_PATCH`` values).

Criterion, for the output and for EVERY parameter and input gradient: the worst relative L2 error of a row (``row_rel``) of the
hip path is at most 4 times that of the torch fp32 path on the same inputs and weights, computed in the same test.  The factor
is ``X3_C / F32_C`` of tests/kernel_checks.py rounded up to 2 -- what the engine's six piece products may lose against an fp32
fused-multiply-add chain -- doubled for two chained GEMMs.  Both numbers are printed."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

import kernel_checks as kc
from kernel_checks import node_kinds as _node_kinds

pytestmark = pytest.mark.gpu

C, HEADS, B, N = 64, 4, 2, 50
FACTOR = 4.0


def _build(name):
    from makani_amd import afnonet_v1, layers, vit
    torch.manual_seed(11)
    if name == "linear":
        return layers.Linear(C, 132), (B, N, C)
    if name == "linear_nobias":
        return layers.Linear(C, 132, bias=False), (B, N, C)
    if name == "mlp":
        return layers.MLP(C, 4 * C, C, input_format="traditional"), (B, N, C)
    if name == "afnov1_mlp":
        return afnonet_v1.Mlp(C, 4 * C), (B, N, C)
    if name == "block":
        return vit.Block(C, HEADS, qkv_bias=True), (B, N, C)
    net = vit.VisionTransformer(inp_shape=[16, 32], patch_size=(4, 4), inp_chans=3, out_chans=3, embed_dim=C, depth=2, num_heads=HEADS)
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


CASES = [("linear", "torch"), ("linear_nobias", "torch"), ("mlp", "torch"), ("afnov1_mlp", "torch"), ("block", "torch"), ("vit", "torch"),
         ("vit", "hip")]


@pytest.mark.parametrize("name,patch", CASES)
def test_hip_path_is_as_accurate_as_the_torch_path(dev, name, patch, monkeypatch):
    monkeypatch.setenv("MK_PATCH", patch)
    monkeypatch.setenv("MK_TOKEN_LINEAR_FP32", "torch")
    mod, shape = _build(name)
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(shape, generator=gen)
    g, want = _reference(mod, x, gen)
    names = ["output", "input gradient"] + [n for n, _ in mod.named_parameters()]
    mod = mod.to(dev)
    got = {}
    for mode in ("hip", "torch"):
        monkeypatch.setenv("MK_TOKEN_LINEAR_FP32", mode)
        got[mode] = _run(mod, x.to(dev), g.to(dev))
    worst = 0.0
    failures = []
    for n, h, t, w in zip(names, got["hip"], got["torch"], want):
        if w is None:
            assert h is None and t is None
            continue
        assert h.dtype == torch.float32
        eh, et = _worst_row(h, w), _worst_row(t, w)
        worst = max(worst, eh / et if et else float("inf"))
        print(f"[x3 modules] {name} (MK_PATCH={patch}) {n}: hip {eh:.3e} torch {et:.3e} ratio {eh / et if et else float('inf'):.3f}")
        if not eh <= FACTOR * et:
            failures.append(f"{n}: hip {eh:.3e} against torch {et:.3e}")
    print(f"[x3 modules] {name} (MK_PATCH={patch}): worst hip / torch {worst:.3f} (limit {FACTOR})")
    assert not failures, f"{name}: " + "; ".join(failures)


def test_hip_path_runs_the_kernels(dev, monkeypatch):
    """Under the knob the linears of a block are the package's fp32 autograd functions: the node names of the graph say so."""
    monkeypatch.setenv("MK_TOKEN_LINEAR_FP32", "hip")
    for name, linears, mlps in (("linear", 1, 0), ("mlp", 0, 1), ("afnov1_mlp", 0, 1), ("block", 2, 1)):
        mod, shape = _build(name)
        kinds = _node_kinds(mod.to(dev)(torch.randn(shape, device=dev)))
        assert sum(k.startswith("_TokenLinearX3") for k in kinds) == linears and sum(k.startswith("_TokenMLPX3") for k in kinds) == mlps, kinds
        assert not any(k.startswith(("AddmmBackward", "MmBackward")) for k in kinds), kinds


@pytest.mark.parametrize("setting", ["knob at torch", "bf16 autocast", "MK_SPECTRAL_GEMM=f32", "declined shape"])
def test_everything_else_is_todays_path_bit_for_bit(dev, setting, monkeypatch):
    """With the knob at ``torch``, under bf16 autocast, with the fp32-MFMA engine selected and for a shape the kernels decline,
    ``layers.Linear`` and the MLP give the bits of ``nn.Linear`` / the module-by-module evaluation, gradients included."""
    from makani_amd import layers, ops
    monkeypatch.setenv("MK_TOKEN_LINEAR_FP32", "torch" if setting == "knob at torch" else "hip")
    if setting == "MK_SPECTRAL_GEMM=f32":
        monkeypatch.setattr(ops, "SPECTRAL_GEMM", "f32")
    autocast = setting == "bf16 autocast"
    o = 130 if setting == "declined shape" else 132
    torch.manual_seed(3)
    ref, mine = nn.Linear(C, o).to(dev), layers.Linear(C, o).to(dev)
    mine.load_state_dict(ref.state_dict(), strict=True)
    x = torch.randn(B, N, C, device=dev)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        assert not (ops.token_linear_fp32_hip() and ops.token_linear_x3_supported(x, mine.weight, mine.bias))
    g = torch.randn(B, N, o, device=dev)
    for a, b in zip(_run(ref, x, g, autocast), _run(mine, x, g, autocast)):
        assert torch.equal(a, b)
    if setting == "declined shape":
        return
    mlp = layers.MLP(C, 4 * C, C, input_format="traditional").to(dev)
    chain = nn.Sequential(*[m for m in mlp.fwd])             # the same modules, evaluated one by one
    g = torch.randn(B, N, C, device=dev)
    for a, b in zip(_run(chain, x, g, autocast), _run(mlp, x, g, autocast)):
        assert torch.equal(a, b)


def test_the_addend_alone_can_ask_for_a_gradient(dev, monkeypatch):
    """Frozen weights and a detached input: the addend's gradient is the incoming gradient, and nothing else is computed."""
    from makani_amd import ops
    monkeypatch.setenv("MK_TOKEN_LINEAR_FP32", "hip")
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(2, 40, 64, generator=gen).to(dev)
    w1, w2 = torch.randn(128, 64, generator=gen).to(dev), torch.randn(64, 128, generator=gen).to(dev)
    for out_features, call in ((128, lambda a: ops.token_linear(x, w1, None, addend=a)), (64, lambda a: ops.token_mlp(x, w1, None, w2, None, addend=a))):
        a = torch.randn(2, 40, out_features, generator=gen).to(dev).requires_grad_()
        g = torch.randn(2, 40, out_features, generator=gen).to(dev)
        out = call(a)
        assert out.dtype == torch.float32 and type(out.grad_fn).__name__.startswith("_Token")
        (ga,) = torch.autograd.grad(out, [a], g)
        assert torch.equal(ga, g)


def test_single_linear_with_gelu(dev, monkeypatch):
    """``ops.token_linear(gelu=True)``: the GELU in the epilogue, its gradient one pointwise pass; against float64 as above."""
    from makani_amd import ops
    gen = torch.Generator().manual_seed(6)
    x, w, b = torch.randn(B, N, C, generator=gen), torch.randn(132, C, generator=gen) / 8, torch.randn(132, generator=gen)
    g = torch.randn(B, N, 132, generator=gen)
    l64 = [t.double().requires_grad_() for t in (x, w, b)]
    y64 = torch.nn.functional.gelu(torch.nn.functional.linear(*l64))
    want = [y64.detach()] + list(torch.autograd.grad(y64, l64, g.double()))
    got = {}
    for mode in ("hip", "torch"):
        monkeypatch.setenv("MK_TOKEN_LINEAR_FP32", mode)
        leaves = [t.to(dev).requires_grad_() for t in (x, w, b)]
        y = ops.token_linear(*leaves, gelu=True)
        assert type(y.grad_fn).__name__.startswith("_TokenLinearX3") == (mode == "hip")
        got[mode] = [y.detach()] + list(torch.autograd.grad(y, leaves, g.to(dev)))
    for n, h, t, w64 in zip(("output", "dx", "dw", "db"), got["hip"], got["torch"], want):
        eh, et = _worst_row(h, w64), _worst_row(t, w64)
        print(f"[x3 modules] linear + gelu {n}: hip {eh:.3e} torch {et:.3e}")
        assert eh <= FACTOR * et, f"{n}: hip {eh:.3e} against torch {et:.3e}"


@pytest.mark.parametrize("with_pos", [True, False])
def test_patch_embed_fp32(dev, with_pos, monkeypatch):
    """``ops.patch_embed`` on an fp32 image outside autocast under both knobs: ``mk_patchify`` to fp32 rows and the x3 GEMM with the
    bias (and ``pos`` as the addend).  The node is three engine GEMMs around permutations, so the result and the gradients of
    image and weight are held to the engine's own criterion, every element under ``x3_elementwise`` against the float64 GEMM on
    the patch rows (``x3_slack_add`` per epilogue addition, ``x3_slack_sum`` for the weight gradient's slabs); the bias gradient
    is a float64 sum rounded once, the gradient of ``pos`` one fp32 addition per element.  (The torch convolution is no
    yardstick here: at this size its weight gradient comes from a kernel that accumulates in float64.)  With either knob at
    ``torch`` it is the convolution bit for bit."""
    from makani_amd import _lib, ops
    gen = torch.Generator().manual_seed(8)
    Bp, Cp, H, W, p0, p1, E = 2, 3, 20, 24, 4, 2, 36                     # F = 24, N = 60: ragged in every tile axis
    F, Np = Cp * p0 * p1, (H // p0) * (W // p1)
    x, w = torch.randn(Bp, Cp, H, W, generator=gen), torch.randn(E, Cp, p0, p1, generator=gen) / 5
    b, pos = torch.randn(E, generator=gen), torch.randn(1, Np, E, generator=gen)
    g = torch.randn(Bp, Np, E, generator=gen)
    ts = (x, w, b, pos) if with_pos else (x, w, b)
    got = {}
    for patch, fp32 in (("hip", "hip"), ("torch", "hip"), ("hip", "torch")):
        monkeypatch.setenv("MK_PATCH", patch)
        monkeypatch.setenv("MK_TOKEN_LINEAR_FP32", fp32)
        leaves = [t.to(dev).requires_grad_() for t in ts]
        y = ops.patch_embed(*leaves)
        kinds = _node_kinds(y)
        assert any(k.startswith("_PatchEmbedX3") for k in kinds) == (patch == fp32 == "hip"), kinds
        got[patch, fp32] = [y.detach()] + list(torch.autograd.grad(y, leaves, g.to(dev)))
    for a, c in zip(got["torch", "hip"], got["hip", "torch"]):
        assert torch.equal(a, c)
    hip = [t.cpu() for t in got["hip", "hip"]]
    assert all(t.dtype == torch.float32 for t in hip)
    # float64 references on the patch rows (order 0: the convolution weight's view(E, F))
    rows, w2, g2 = ops._patchify_torch(x, (p0, p1), 0).reshape(-1, F), w.reshape(E, F), g.reshape(-1, E)
    r64, w64, g64 = rows.double(), w2.double(), g2.double()
    pre = r64 @ w64.t() + b.double()
    ref = (pre.view(Bp, Np, E) + pos.double()) if with_pos else pre.view(Bp, Np, E)
    slack = kc.x3_slack_add(pre).view(Bp, Np, E) + (kc.x3_slack_add(ref) if with_pos else 0.0)
    worst = [kc.x3_elementwise(hip[0], ref, kc.absdot("rf,ef->re", rows, w2).view(Bp, Np, E), slack64=slack, what="output")]
    unpatch = lambda t: ops._unpatchify_torch(t.view(Bp, Np, F), (p0, p1), Cp, H, W, 0)
    worst.append(kc.x3_elementwise(hip[1], unpatch(g64 @ w64), unpatch(kc.absdot("re,ef->rf", g2, w2)), what="image gradient"))
    nbytes = _lib.load().mk_token_linear_x3_wgrad_workspace(Bp * Np, E, F, 0)
    slabs = max(1, (nbytes - (Bp * Np + 127) // 128 * E * 8) // (E * F * 4))
    mag = kc.absdot("re,rf->ef", g2, rows)
    worst.append(kc.x3_elementwise(hip[2], (g64.t() @ r64).view(E, Cp, p0, p1), mag.view(E, Cp, p0, p1),
                                   slack64=kc.x3_slack_sum(slabs, mag).view(E, Cp, p0, p1), what="weight gradient"))
    db64 = g64.sum(0)
    assert bool(((hip[3].double() - db64).abs() <= 2.0 ** -23 * db64.abs() + 2.0 ** -40 * g64.abs().sum(0)).all()), "bias gradient"
    if with_pos:
        assert bool(((hip[4].double() - g.double().sum(0, keepdim=True)).abs() <= 2.0 ** -23 * g.double().abs().sum(0, keepdim=True)).all()), "pos"
    print(f"[x3 modules] patch embed (pos={with_pos}): worst ratios output {worst[0]:.2f}, image gradient {worst[1]:.2f}, "
          f"weight gradient {worst[2]:.2f} of {kc.X3_C} ({slabs} slab(s))")
