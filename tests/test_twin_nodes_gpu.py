"""The gradient branches of the five autograd nodes that exist in two arithmetics -- ``token_linear``, ``token_mlp``,
``patch_embed``, ``attention``, ``attention_packed``; bf16 and fp32 on bf16x3 -- characterised through the public functions only.

Every case runs forward and backward once with every floating leaf requiring a gradient, then once per leaf with only that leaf
requiring one.  The output and the leaf's gradient of the second run must be ``torch.equal`` to the first run's: which
gradients are asked for selects launches and saved tensors (``needs_input_grad``), never values.  The kernels use no atomics and
fixed summation orders, so equal bits are what a correct node gives.  The node taken is asserted by its ``grad_fn`` name.

Shapes are the smallest that straddle the tile edges: 2 x 35 rows (no multiple of 64 or 128), feature counts that are small
multiples of the arithmetic's unit, 70 queries against 45 keys."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ARITH = {
    "bf16": dict(dtype=torch.bfloat16, suffix="", unit=8,
                 env=dict(MK_ATTN="hip", MK_TOKEN_LINEAR="hip", MK_PATCH="hip")),
    "fp32": dict(dtype=torch.float32, suffix="X3", unit=4,
                 env=dict(MK_ATTN_FP32="hip", MK_TOKEN_LINEAR_FP32="hip", MK_PATCH="hip")),
}
ROWS = (2, 35)
B, H, D, NQ, NK, N_PACKED = 2, 2, 16, 70, 45, 70


def _linear_case(arith, kind, bias, sliced=False, rows=ROWS, out=None):
    """``token_linear``: ``kind`` plain / gelu / addend.  bf16 takes a bf16 weight next to an fp32 bias: both casts of the
    parameter gradients, to bf16 and none, are on the path."""
    dt = ARITH[arith]["dtype"]
    I, O = (24, 40) if arith == "bf16" else (12, 20)
    O = O if out is None else out

    def make(rnd):
        if sliced:          # a [..., :I] view of a wider buffer; its row stride stays a multiple of 16 bytes
            x = rnd(*rows, I + ARITH[arith]["unit"]).to(dt)[..., :I]
        else:
            x = rnd(*rows, I).to(dt)
        leaves = dict(x=x, weight=(0.3 * rnd(O, I)).to(dt))
        if bias:
            leaves["bias"] = rnd(O)
        if kind == "addend":
            leaves["addend"] = rnd(*rows, O)
        return leaves

    def fn(ops, x, weight, bias=None, addend=None):
        return ops.token_linear(x, weight, bias, gelu=(kind == "gelu"), addend=addend)

    return make, fn, "_TokenLinear"


def _mlp_case(arith, addend, biases):
    dt = ARITH[arith]["dtype"]
    I, Hd, O = (24, 40, 16) if arith == "bf16" else (12, 20, 8)

    def make(rnd):
        leaves = dict(x=rnd(*ROWS, I).to(dt), w1=0.3 * rnd(Hd, I), w2=(0.3 * rnd(O, Hd)).to(dt))
        if biases:
            leaves.update(b1=rnd(Hd).to(dt), b2=rnd(O))
        if addend:
            leaves["addend"] = rnd(*ROWS, O)
        return leaves

    def fn(ops, x, w1, w2, b1=None, b2=None, addend=None):
        return ops.token_mlp(x, w1, b1, w2, b2, addend=addend)

    return make, fn, "_TokenMLP"


def _patch_case(arith, pos):
    dt = ARITH[arith]["dtype"]          # outside autocast the bf16 node takes bf16 parameters only, as nn.Conv2d does
    E, C, hw, p = 16, 3, (8, 16), 4

    def make(rnd):
        leaves = dict(img=rnd(2, C, *hw).to(dt), weight=(0.2 * rnd(E, C, p, p)).to(dt), bias=rnd(E).to(dt))
        if pos:
            leaves["pos"] = rnd(1, (hw[0] // p) * (hw[1] // p), E)
        return leaves

    def fn(ops, img, weight, bias, pos=None):
        return ops.patch_embed(img, weight, bias, pos)

    return make, fn, "_PatchEmbed"


def _attention_case(arith):
    dt = ARITH[arith]["dtype"]

    def make(rnd):
        return dict(q=rnd(B, H, NQ, D).to(dt), k=rnd(B, H, NK, D).to(dt), v=rnd(B, H, NK, D).to(dt))

    return make, (lambda ops, q, k, v: ops.attention(q, k, v)), "_Attention"


def _packed_case(arith, sliced):
    dt = ARITH[arith]["dtype"]

    def make(rnd):
        qkv = rnd(B, N_PACKED, 3 * H * D * (2 if sliced else 1)).to(dt)
        return dict(qkv=qkv[..., ::2] if sliced else qkv)       # element stride 2: the op has to make it contiguous

    return make, (lambda ops, qkv: ops.attention_packed(qkv, H)), "_AttentionPacked"


def _cases(arith):
    out = {}
    for kind in ("plain", "gelu", "addend"):
        for bias in (True, False):
            out[f"linear-{kind}-{'bias' if bias else 'nobias'}"] = _linear_case(arith, kind, bias)
    out["linear-plain-bias-sliced"] = _linear_case(arith, "plain", True, sliced=True)
    if arith == "fp32":     # R O = 35 * 12 is no multiple of 8: the GELU is torch's, behind the node without one
        out["linear-gelu-decomposed"] = _linear_case(arith, "gelu", True, rows=(1, 35), out=12)
    for addend in (False, True):
        for biases in (True, False):
            out[f"mlp-{'addend' if addend else 'plain'}-{'biases' if biases else 'nobiases'}"] = _mlp_case(arith, addend, biases)
    out["patch-pos"] = _patch_case(arith, True)
    out["patch-nopos"] = _patch_case(arith, False)
    out["attention"] = _attention_case(arith)
    out["packed"] = _packed_case(arith, False)
    out["packed-sliced"] = _packed_case(arith, True)
    return out


CASES = [(arith, name) for arith in ARITH for name in _cases(arith)]


def run_case(ops, dev, arith, name):
    """{"y": output, leaf name: gradient with every leaf asking, ("only", leaf name): (output, gradient) with that leaf alone}.
    The knobs of ``ARITH[arith]["env"]`` are the caller's to set."""
    make, fn, node = _cases(arith)[name]
    gen = torch.Generator().manual_seed(1 + CASES.index((arith, name)))
    base = make(lambda *shape: torch.randn(*shape, generator=gen).to(dev))      # slices are taken on the device: they stay views
    assert all(t.is_floating_point() for t in base.values())

    def run(asking):
        leaves = {n: t.detach().requires_grad_(n in asking) for n, t in base.items()}
        y = fn(ops, **leaves)
        return y, leaves

    y, leaves = run(set(base))
    kind = type(y.grad_fn).__name__
    want = node + ARITH[arith]["suffix"] + "Backward"
    if name.endswith("decomposed"):
        assert kind.startswith("GeluBackward"), kind
        kind = type(y.grad_fn.next_functions[0][0]).__name__
    assert kind == want, (arith, name, kind)
    g = torch.randn(y.shape, generator=gen).to(dev, y.dtype)
    names = list(base)
    got = {"y": y.detach()}
    got.update(zip(names, torch.autograd.grad(y, [leaves[n] for n in names], g)))
    for n in names:
        y1, leaves1 = run({n})
        (g1,) = torch.autograd.grad(y1, [leaves1[n]], g)
        got["only", n] = (y1.detach(), g1)
    return got


@pytest.mark.parametrize("arith,name", CASES, ids=[f"{a}-{n}" for a, n in CASES])
def test_a_gradient_alone_has_the_bits_of_all_gradients_together(dev, arith, name, monkeypatch):
    from makani_amd import ops
    for knob, value in ARITH[arith]["env"].items():
        monkeypatch.setenv(knob, value)
    got = run_case(ops, dev, arith, name)
    for key, value in got.items():
        if isinstance(key, tuple):
            y1, g1 = value
            assert torch.equal(y1, got["y"]), (arith, name, key, "output")
            assert g1.dtype == got[key[1]].dtype and torch.equal(g1, got[key[1]]), (arith, name, key, "gradient")
