"""The fp32 token-major linears (csrc/x3_toklinear.hip, ``MK_TOKEN_LINEAR_FP32``) without a device: the knob is validated, CPU
tensors take the torch formulation bit for bit, ``token_linear_x3_supported`` declines what it must, the tile is reported, and
the constants and the criterion that tests/test_x3_toklinear_gpu.py holds the kernels to are themselves measured and checked."""
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import kernel_checks as kc

import capi_checks as capi
from makani_amd import _lib, layers, ops

FWD_SHAPES = [(1, 4, 4), (33, 36, 68), (129, 132, 132), (200, 280, 260)]       # (R, I, O) of the GPU test
WGRAD_SHAPES = [(200, 68, 36), (129, 132, 132)]                               # (R, O, I)
U = 2.0 ** -23


# ---- the rounding of the activation's own fp32 evaluation ------------------------------------------------------------------------
def _gelu_points():
    z = torch.cat([torch.linspace(-9.0, 9.0, 360001), 1.5 * torch.randn(200000, generator=torch.Generator().manual_seed(11))])
    return z[z != 0].float()


def _gelu32(z):
    """``mk::gelu::Act<float>::gelu`` in torch fp32, operation by operation."""
    return 0.5 * z * (1.0 + torch.erf(z * 0.70710678118654752440))


def _gelu_grad32(z):
    """``mk::gelu::Act<float>::gelu_grad`` in torch fp32, operation by operation."""
    return 0.5 * (1.0 + torch.erf(z * 0.70710678118654752440)) + z * 0.39894228040143267794 * torch.exp(-0.5 * z * z)


def _measure():
    z = _gelu_points()
    assert z.dtype == torch.float32
    g = ((_gelu32(z).double() - kc.gelu64(z.double())).abs() / (U * z.double().abs())).max()
    gg = ((_gelu_grad32(z).double() - kc.gelu_grad64(z.double())).abs() / U).max()
    return float(g), float(gg)


_MEASURED = _measure()
# |gelu_fp32(z) - gelu(z)| <= GELU_ROUND_C 2^-23 |z|  and  |gelu'_fp32(z) - gelu'(z)| <= GELU_GRAD_ROUND_C 2^-23: twice what
# the fp32 expression reaches in torch against float64 over [-9, 9] and N(0, 1.5) points, rounded up to a quarter
GELU_ROUND_C = math.ceil(8 * _MEASURED[0]) / 4
GELU_GRAD_ROUND_C = math.ceil(8 * _MEASURED[1]) / 4


def test_gelu_rounding_constants():
    """The measured worst cases are what the error analysis expects (a few roundings of values at most 2), and the doubled
    constants stay small against the engine's own allowance ``X3_C``."""
    print(f"[x3 toklinear] gelu rounding {_MEASURED[0]:.3f} -> C = {GELU_ROUND_C}; gelu' rounding {_MEASURED[1]:.3f} -> C = {GELU_GRAD_ROUND_C}")
    assert 0.25 <= _MEASURED[0] <= 2.0 and 0.25 <= _MEASURED[1] <= 2.0
    assert GELU_ROUND_C >= 2 * _MEASURED[0] and GELU_GRAD_ROUND_C >= 2 * _MEASURED[1]
    assert GELU_ROUND_C <= kc.X3_C / 2 and GELU_GRAD_ROUND_C <= kc.X3_C / 2
    assert float(kc.gelu_grad64(torch.linspace(-9, 9, 100001, dtype=torch.float64)).abs().max()) <= kc.GELU_GRAD_MAX


# ---- knob, dispatch, info -------------------------------------------------------------------------------------------------------
def test_knob_is_validated(monkeypatch):
    x, lin = torch.randn(2, 8), layers.Linear(8, 8)
    monkeypatch.setenv("MK_TOKEN_LINEAR_FP32", "bogus")
    for call in (ops.token_linear_fp32_hip, lambda: lin(x), lambda: ops.token_linear(x, lin.weight, lin.bias),
                 lambda: ops.token_mlp(x, lin.weight, lin.bias, lin.weight, lin.bias)):
        with pytest.raises(ValueError, match="MK_TOKEN_LINEAR_FP32"):
            call()
    monkeypatch.delenv("MK_TOKEN_LINEAR_FP32")
    assert ops.token_linear_fp32_hip() == (ops.TOKEN_LINEAR_FP32_DEFAULT == "hip")
    monkeypatch.setenv("MK_TOKEN_LINEAR_FP32", "hip")
    assert ops.token_linear_fp32_hip() is True
    monkeypatch.setenv("MK_TOKEN_LINEAR", "bogus")          # the two knobs are separate: the bf16 one is still validated
    with pytest.raises(ValueError, match="MK_TOKEN_LINEAR "):
        lin(x)


def _grads(out, inputs, seed=3):
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(seed)).to(out.dtype)
    return torch.autograd.grad(out, inputs, g)


@pytest.mark.parametrize("mode", ["hip", "torch"])
def test_cpu_tensors_are_the_torch_formulation(mode, monkeypatch):
    monkeypatch.setenv("MK_TOKEN_LINEAR_FP32", mode)
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(2, 7, 16, generator=gen)
    w1, b1 = torch.randn(32, 16, generator=gen), torch.randn(32, generator=gen)
    w2, b2 = torch.randn(16, 32, generator=gen), torch.randn(16, generator=gen)
    addend = torch.randn(2, 7, 16, generator=gen)

    def same(fa, fb, ts):
        la, lb = [t.clone().requires_grad_() for t in ts], [t.clone().requires_grad_() for t in ts]
        ya, yb = fa(*la), fb(*lb)
        assert torch.equal(ya, yb)
        for a, b in zip(_grads(ya, la), _grads(yb, lb)):
            assert torch.equal(a, b)

    same(lambda x, w, b: ops.token_linear(x, w, b), lambda x, w, b: F.linear(x, w, b), (x, w1, b1))
    same(lambda x, w, b: ops.token_linear(x, w, b, gelu=True), lambda x, w, b: F.gelu(F.linear(x, w, b)), (x, w1, b1))
    same(lambda x, w1, b1, w2, b2, a: ops.token_mlp(x, w1, b1, w2, b2, addend=a),
         lambda x, w1, b1, w2, b2, a: a + F.linear(F.gelu(F.linear(x, w1, b1)), w2, b2), (x, w1, b1, w2, b2, addend))
    torch.manual_seed(0)
    ref, mine = nn.Linear(16, 32), layers.Linear(16, 32)
    mine.load_state_dict(ref.state_dict())
    same(lambda x: ref(x), lambda x: mine(x), (x,))
    mlp = layers.MLP(16, 32, 16, input_format="traditional")
    want = mlp.fwd[3](mlp.fwd[1](mlp.fwd[0](x)))
    assert torch.equal(mlp(x), want) and torch.equal(mlp(x, addend=x), x + want)


def test_supported_declines():
    x, w, b = torch.randn(6, 16), torch.randn(32, 16), torch.randn(32)
    declined = {
        "a CPU tensor": (x, w, b),
        "a bf16 input": (x.bfloat16(), w, b),
        "a float64 input": (x.double(), w.double(), b.double()),
        "a bf16 weight": (x, w.bfloat16(), b),
        "a bf16 bias": (x, w, b.bfloat16()),
        "I not a multiple of 4": (torch.randn(6, 18), torch.randn(32, 18), b),
        "O not a multiple of 4": (x, torch.randn(30, 16), torch.randn(30)),
        "a weight of another shape": (x, torch.randn(32, 20), b),
        "a 3-d weight": (x, torch.randn(2, 32, 16), b),
        "an empty input": (torch.randn(0, 16), w, b),
        "not a tensor": (None, w, b),
    }
    for name, args in declined.items():
        assert ops.token_linear_x3_supported(*args) is False, name
    assert ops.token_linear_x3_supported(x, w) is False


def test_patch_embed_declines_and_is_the_convolution_on_the_cpu(monkeypatch):
    monkeypatch.setenv("MK_PATCH", "hip")
    monkeypatch.setenv("MK_TOKEN_LINEAR_FP32", "hip")
    x, w, b = torch.randn(2, 3, 8, 8), torch.randn(16, 3, 4, 4), torch.randn(16)
    for name, args in {"a CPU image": (x, w, b), "a bf16 image": (x.bfloat16(), w, b), "a bf16 weight": (x, w.bfloat16(), b),
                       "E not a multiple of 4": (x, torch.randn(18, 3, 4, 4), torch.randn(18)),
                       "F not a multiple of 4": (x, torch.randn(16, 3, 1, 2), b),
                       "a patch that does not divide": (x, torch.randn(16, 3, 3, 4), b), "a 3-d image": (x[0], w, b)}.items():
        assert ops.patch_embed_x3_supported(*args) is False, name
    want = F.conv2d(x, w, b, stride=(4, 4)).flatten(2).transpose(1, 2)
    assert torch.equal(ops.patch_embed(x, w, b), want)
    monkeypatch.setenv("MK_TOKEN_LINEAR_FP32", "bogus")
    with pytest.raises(ValueError, match="MK_TOKEN_LINEAR_FP32"):
        ops.patch_embed(x, w, b)
    with pytest.raises(ValueError, match="MK_TOKEN_LINEAR_FP32"):
        layers.PatchEmbed((8, 8), (4, 4), 3, 16).forward_tokens(x)


def test_supported_follows_the_engine_switch(monkeypatch):
    """With ``MK_SPECTRAL_GEMM=f32`` nothing is supported, before any other question is asked."""
    class Anything:
        pass

    monkeypatch.setattr(ops, "SPECTRAL_GEMM", "f32")
    assert ops.token_linear_x3_supported(Anything(), Anything()) is False
    assert ops.patch_embed_x3_supported(Anything(), Anything()) is False


def test_info_without_a_device():
    assert ops.token_linear_x3_info() == {"tr": 128, "tc": 128, "tk": 32}
    lib = _lib.load()
    assert lib.mk_token_linear_x3_info(None) != 0 and "null pointer" in lib.mk_last_error().decode()
    # the workspace query needs no device either: -1 for refused sizes; one slab still holds the bias gradient's float64 partials
    assert lib.mk_token_linear_x3_wgrad_workspace(200, 68, 38, 1) == -1
    assert lib.mk_token_linear_x3_wgrad_workspace(200, 68, 36, 65) == -1
    assert lib.mk_token_linear_x3_wgrad_workspace(200, 68, 36, 1) == 2 * 68 * 8
    assert lib.mk_token_linear_x3_wgrad_workspace(200, 68, 36, 3) == 3 * 68 * 36 * 4 + 2 * 68 * 8
    assert lib.mk_token_linear_x3_wgrad_workspace(20, 68, 36, 3) == 68 * 8             # one 32-row step: one slab


# ---- the criterion is checked: planted defects at the GPU test's shapes --------------------------------------------------------------
def _caught(y, ref, mag, slack=None):
    try:
        kc.x3_elementwise(y, ref, mag, slack64=slack)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("R,I,O", FWD_SHAPES)
def test_planted_forward_defects_are_caught(R, I, O):
    """A result that is the correctly rounded value passes; against a float64 reference with one k-step (32 contraction
    indices) or the bias left out, the same result fails: a kernel with that defect is caught at this shape.  The same with the
    GELU row's wider bound."""
    g = torch.Generator().manual_seed(R + I + O)
    x, w, b = torch.randn(R, I, generator=g), torch.randn(O, I, generator=g) / I ** 0.5, torch.randn(O, generator=g)
    x64, w64 = x.double(), w.double()
    mag = kc.absdot("rk,ok->ro", x, w)
    pre = torch.einsum("rk,ok->ro", x64, w64) + b.double()
    y = pre.float()
    slack = kc.x3_slack_add(pre)
    assert not _caught(y, pre, mag, slack)
    k0 = (I // 32 // 2) * 32
    no_step = pre - torch.einsum("rk,ok->ro", x64[:, k0:k0 + 32], w64[:, k0:k0 + 32])
    assert _caught(y, no_step, mag, kc.x3_slack_add(no_step))
    no_bias = pre - b.double()
    assert _caught(y, no_bias, mag, kc.x3_slack_add(no_bias))
    # the GELU row: bound GELU_GRAD_MAX (X3_C 2^-23 mag + 2^-23 |pre|) + GELU_ROUND_C 2^-23 |pre|
    yg = kc.gelu64(pre).float()
    for ref, bad in ((pre, False), (no_step, True), (no_bias, True)):
        gs = kc.GELU_GRAD_MAX * kc.x3_slack_add(ref) + GELU_ROUND_C * U * ref.abs()
        assert _caught(yg, kc.gelu64(ref), kc.GELU_GRAD_MAX * mag, gs) is bad


@pytest.mark.parametrize("R,O,I", WGRAD_SHAPES)
@pytest.mark.parametrize("slabs", [1, 2, 3])
def test_planted_wgrad_defects_are_caught(R, O, I, slabs):
    """The weight gradient with one slab of tokens left out of the reference is caught, with the slack of ``slabs`` panels."""
    g = torch.Generator().manual_seed(R + O + I)
    dy, x = torch.randn(R, O, generator=g), torch.randn(R, I, generator=g)
    mag = kc.absdot("ro,ri->oi", dy, x)
    ref = torch.einsum("ro,ri->oi", dy.double(), x.double())
    y = ref.float()
    slack = kc.x3_slack_sum(slabs, mag)
    assert not _caught(y, ref, mag, slack)
    kslab = -(-(-(-R // 32)) // slabs) * 32                 # rows of a slab: whole 32-row steps
    lo = (slabs - 1) * kslab                                # the last, shortest slab
    assert lo < R
    missing = ref - torch.einsum("ro,ri->oi", dy.double()[lo:], x.double()[lo:])
    assert _caught(y, missing, mag, slack)
    # a bias gradient that misses one row is outside the GPU test's bound
    db, db_bad = dy.double().sum(0), dy.double()[1:].sum(0)
    tol = U * db_bad.abs() + 2.0 ** -40 * dy.double().abs().sum(0)
    assert bool(((db.float().double() - db_bad).abs() > tol).any())


# ---------------------------------------------------------------------------------------------------------------------
# misaligned pointers: refused by the host checks, with the message of the check (tests/capi_checks.py)
# ---------------------------------------------------------------------------------------------------------------------
_A = capi.A
MISALIGNED = [      # entry point, its arguments in front of the stream with one pointer moved off its alignment, the refusal
    ("mk_token_linear_x3_fwd", (_A, 8, _A, 8, 0, None, _A + 4, 4) + (None, 0) * 3 + (0, 3, 4, 8), "operand not 16-byte aligned"),
    ("mk_token_linear_x3_fwd", (_A, 8, _A, 8, 0, _A + 8, _A, 4) + (None, 0) * 3 + (0, 3, 4, 8), "bias not 16-byte aligned"),
    ("mk_token_linear_x3_wgrad", (_A, 4, _A + 4, 8, _A, 8, None, None, 3, 4, 8, 1), "operand not 16-byte aligned"),
    ("mk_token_linear_x3_wgrad", (_A, 4, _A, 8, _A, 8, _A + 8, _A, 3, 4, 8, 1), "db not 16-byte aligned"),
    ("mk_token_linear_x3_wgrad", (_A, 4, _A, 8, _A, 8, _A, _A + 8, 3, 4, 8, 1), "workspace null or not 16-byte aligned"),
]


@pytest.mark.parametrize("case", MISALIGNED, ids=capi.case_ids(MISALIGNED))
def test_misaligned_pointer_is_refused_before_any_launch(case):
    capi.assert_refused(*case)
