"""The token-major linears without a device: ``layers.Linear``, ``ops.token_linear`` and ``ops.token_mlp`` are the torch calls bit
for bit on the CPU, the knob is validated, and the bounds of tests/toklinear_checks.py are themselves checked -- each defect a
kernel of this kind can have exceeds them on a small case, and the stated arithmetic evaluated exactly stays inside."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import toklinear_checks as tc

import capi_checks as capi
from makani_amd import layers, ops

BF = torch.bfloat16


def _grads(out, inputs, seed=3):
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(seed)).to(out.dtype)
    return torch.autograd.grad(out, inputs, g)


@pytest.mark.parametrize("bias", [True, False])
def test_linear_module_is_nn_linear_on_the_cpu(bias, monkeypatch):
    torch.manual_seed(0)
    ref = nn.Linear(24, 40, bias=bias)
    mine = layers.Linear(24, 40, bias=bias)
    assert isinstance(mine, nn.Linear)
    assert list(mine.state_dict()) == list(ref.state_dict())
    mine.load_state_dict(ref.state_dict(), strict=True)
    x = torch.randn(3, 5, 24)
    for mode in ("hip", "torch"):
        monkeypatch.setenv("MK_TOKEN_LINEAR", mode)
        xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
        ya, yb = ref(xa), mine(xb)
        assert torch.equal(ya, yb)
        for a, b in zip(_grads(ya, [xa] + list(ref.parameters())), _grads(yb, [xb] + list(mine.parameters()))):
            assert torch.equal(a, b)


@pytest.mark.parametrize("mode", ["hip", "torch"])
def test_ops_on_cpu_tensors_are_the_torch_formulation(mode, monkeypatch):
    monkeypatch.setenv("MK_TOKEN_LINEAR", mode)
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(2, 7, 16, generator=gen)
    w1, b1 = torch.randn(32, 16, generator=gen), torch.randn(32, generator=gen)
    w2, b2 = torch.randn(16, 32, generator=gen), torch.randn(16, generator=gen)
    addend = torch.randn(2, 7, 16, generator=gen)
    assert not ops.token_linear_supported(x, w1, b1)

    def leaves(*ts):
        return [t.clone().requires_grad_() for t in ts]

    def same(fa, fb, ts):
        la, lb = leaves(*ts), leaves(*ts)
        ya, yb = fa(*la), fb(*lb)
        assert torch.equal(ya, yb)
        for a, b in zip(_grads(ya, la), _grads(yb, lb)):
            assert torch.equal(a, b)

    same(lambda x, w, b: ops.token_linear(x, w, b), lambda x, w, b: F.linear(x, w, b), (x, w1, b1))
    same(lambda x, w: ops.token_linear(x, w), lambda x, w: F.linear(x, w), (x, w1))
    same(lambda x, w, b: ops.token_linear(x, w, b, gelu=True), lambda x, w, b: F.gelu(F.linear(x, w, b)), (x, w1, b1))
    same(lambda x, w, b, a: ops.token_linear(x, w, b, addend=a), lambda x, w, b, a: a + F.linear(x, w, b), (x, w2.T.contiguous(), b1, torch.randn(2, 7, 32, generator=gen)))
    same(lambda x, w1, b1, w2, b2: ops.token_mlp(x, w1, b1, w2, b2), lambda x, w1, b1, w2, b2: F.linear(F.gelu(F.linear(x, w1, b1)), w2, b2),
         (x, w1, b1, w2, b2))
    same(lambda x, w1, b1, w2, b2, a: ops.token_mlp(x, w1, b1, w2, b2, addend=a),
         lambda x, w1, b1, w2, b2, a: a + F.linear(F.gelu(F.linear(x, w1, b1)), w2, b2), (x, w1, b1, w2, b2, addend))
    with pytest.raises(ValueError):
        ops.token_linear(x, w1, b1, gelu=True, addend=addend)


def test_traditional_modules_keep_their_results_and_keys(monkeypatch):
    """The traditional ``MLP`` (with and without the addend) and ``EncoderDecoder`` equal the module-by-module evaluation."""
    monkeypatch.setenv("MK_TOKEN_LINEAR", "hip")
    torch.manual_seed(2)
    mlp = layers.MLP(16, 32, 16, input_format="traditional")
    assert all(isinstance(m, nn.Linear) for m in (mlp.fwd[0], mlp.fwd[3]))
    assert list(mlp.state_dict()) == ["fwd.0.weight", "fwd.0.bias", "fwd.3.weight", "fwd.3.bias"]
    x = torch.randn(2, 5, 16)
    want = mlp.fwd[3](mlp.fwd[1](mlp.fwd[0](x)))
    assert torch.equal(mlp(x), want)
    assert torch.equal(mlp(x, addend=x), x + want)
    enc = layers.EncoderDecoder(2, 16, 24, 32, nn.GELU, input_format="traditional")
    assert torch.equal(enc(x), enc.fwd(x))
    with pytest.raises(ValueError):
        layers.MLP(16, 32, 16)(torch.randn(1, 16, 4, 4), addend=torch.randn(1, 16, 4, 4))


def test_knob_is_validated(monkeypatch):
    monkeypatch.setenv("MK_TOKEN_LINEAR", "bogus")
    with pytest.raises(ValueError):
        ops.token_linear_hip()
    with pytest.raises(ValueError):
        layers.Linear(8, 8)(torch.randn(2, 8))
    monkeypatch.delenv("MK_TOKEN_LINEAR")
    assert ops.token_linear_hip() == (ops.TOKEN_LINEAR_DEFAULT == "hip")


def test_info_without_a_device():
    t = ops.token_linear_info()
    assert set(t) == {"tr", "tc", "tk", "to", "ti", "ts"} and all(v >= 8 for v in t.values())


# ---- the checker is checked ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    t = ops.token_linear_info()
    R, O, I = 96, 64, 2 * t["tk"]
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(R, I, generator=gen).to(BF)
    w = (torch.randn(O, I, generator=gen) * I ** -0.5).to(BF)
    b = torch.randn(O, generator=gen) * 0.5
    addend = torch.randn(R, O, generator=gen)
    aux = torch.randn(R, O, generator=gen).to(BF)
    dy = (torch.randn(R, O, generator=gen) + 0.5).to(BF)
    return dict(x=x, w=w, b=b, addend=addend, aux=aux, dy=dy, tk=t["tk"], ref=tc.Ref(x, w, b), ref0=tc.Ref(x, w))


def test_exact_evaluation_with_the_stated_rounding_points_passes(small):
    s = small
    pre = tc.emulate_plain(s["ref"])
    tc.check_plain(pre, s["ref"], "plain")
    tc.check_pre(pre, s["ref"], "pre")
    tc.check_act(tc.emulate_act(pre), pre, "act")
    tc.check_addend(tc.emulate_addend(s["ref"], s["addend"]), s["addend"], s["ref"], "addend")
    tc.check_aux(tc.emulate_aux(s["ref0"], s["aux"]), s["ref0"], s["aux"], "aux")
    dw = (s["dy"].double().T @ s["x"].double()).float()
    tc.check_wgrad(dw, s["dy"], s["x"], "dW")
    tc.check_dbias(s["dy"].double().sum(0).float(), s["dy"], "db")
    # an fp32 accumulation in another order (here: torch's) passes as well
    tc.check_wgrad(s["dy"].float().T @ s["x"].float(), s["dy"], s["x"], "dW fp32")
    tc.check_plain((s["x"].float() @ s["w"].float().T + s["b"]).to(BF), s["ref"], "plain fp32")


def test_a_dropped_last_k_step_is_caught(small):
    s = small
    k = s["x"].shape[1] - s["tk"]
    short = (s["x"][:, :k].double() @ s["w"][:, :k].double().T + s["b"].double())
    for check in (tc.check_plain, tc.check_pre):
        with pytest.raises(AssertionError):
            check(short.to(BF), s["ref"], "dropped k-step")
    with pytest.raises(AssertionError):
        tc.check_addend((s["addend"].double() + short.to(BF).double()).float(), s["addend"], s["ref"], "dropped k-step")
    with pytest.raises(AssertionError):
        acc = s["x"][:, :k].double() @ s["w"][:, :k].double().T
        tc.check_aux((acc * tc.kc.gelu_grad64(s["aux"].double())).to(BF), s["ref0"], s["aux"], "dropped k-step")


def test_a_dropped_last_token_is_caught(small):
    s = small
    dy, x = s["dy"].double(), s["x"].double()
    with pytest.raises(AssertionError):
        tc.check_wgrad((dy[:-1].T @ x[:-1]).float(), s["dy"], s["x"], "dropped token")
    with pytest.raises(AssertionError):
        tc.check_dbias(dy[:-1].sum(0).float(), s["dy"], "dropped token")


def test_a_gelu_of_the_unrounded_pre_is_caught(small):
    s = small
    pre = tc.emulate_plain(s["ref"])
    with pytest.raises(AssertionError):
        tc.check_act(tc.kc.gelu64(s["ref"].pre).to(BF), pre, "gelu of the unrounded pre")


def test_a_missing_bias_is_caught(small):
    s = small
    nobias = s["ref0"].pre
    for check in (tc.check_plain, tc.check_pre):
        with pytest.raises(AssertionError):
            check(nobias.to(BF), s["ref"], "no bias")
    with pytest.raises(AssertionError):
        tc.check_addend((s["addend"].double() + nobias.to(BF).double()).float(), s["addend"], s["ref"], "no bias")


# ---------------------------------------------------------------------------------------------------------------------
# misaligned pointers: refused by the host checks, with the message of the check (tests/capi_checks.py)
# ---------------------------------------------------------------------------------------------------------------------
_A = capi.A
MISALIGNED = [      # entry point, its arguments in front of the stream with one pointer moved off its alignment, the refusal
    ("mk_token_linear_fwd", (_A + 8, 16, _A, 16, None, _A, 8) + (None, 0) * 5 + (3, 8, 16), "operand not 16-byte aligned"),
    ("mk_token_linear_fwd", (_A, 16, _A, 16, _A + 4, _A, 8) + (None, 0) * 5 + (3, 8, 16), "bias not 16-byte aligned"),
    ("mk_token_linear_pack", (_A + 8, 0, 16, _A, 16, 8, 16, 0), "operand not 16-byte aligned"),
    ("mk_token_linear_gelu_grad", (_A, 8, _A + 8, 8, _A, 8, 3, 8), "operand not 16-byte aligned"),
    ("mk_token_linear_wgrad", (_A, 8, _A, 16, _A + 8, 16, None, None, 3, 8, 16, 1), "operand not 16-byte aligned"),
    ("mk_token_linear_wgrad", (_A, 8, _A, 16, _A, 16, _A + 4, None, 3, 8, 16, 1), "db not 16-byte aligned"),
    ("mk_token_linear_wgrad", (_A, 8, _A, 16, _A, 16, None, _A + 8, 4096, 8, 16, 2), "workspace null or not 16-byte aligned"),
]


@pytest.mark.parametrize("case", MISALIGNED, ids=capi.case_ids(MISALIGNED))
def test_misaligned_pointer_is_refused_before_any_launch(case):
    capi.assert_refused(*case)
