"""CPU side of the attention checks: the emulation of the kernels' rounding points (tests/attn_checks.py) against the bounds the
GPU tests apply, ``ops.attention`` / ``ops.attention_packed`` on CPU tensors against the float64 formula, ``MK_ATTN`` validation."""
import pytest
import torch

import attn_checks as ac


@pytest.fixture(scope="module")
def emulated():
    """(N, D, input scale, seed, rounded_sum) -> (reference, emulation), computed once."""
    out = {}
    for N, D, sc in ac.EMU_SHAPES:
        for seed in range(ac.EMU_SEEDS):
            q, k, v, go = ac.make_inputs(N, D, sc, seed=seed)
            ref = ac.reference(q, k, v, go)
            for rs in (False, True):
                out[(N, D, sc, seed, rs)] = (ref, ac.emulate(q, k, v, go, rounded_sum=rs))
    return out


def test_constants_are_twice_the_emulation_s_worst_ratio():
    for c, worst in ((ac.DV_C, ac.EMU_WORST_DV), (ac.DQ_C, ac.EMU_WORST_DQ), (ac.DK_C, ac.EMU_WORST_DK), (ac.LSE_C, ac.EMU_WORST_LSE)):
        assert 2 * worst <= c <= 2 * worst + 1.0
    assert ac.FWD_C == 2.0


@pytest.mark.parametrize("rounded_sum", [False, True])
@pytest.mark.parametrize("shape", ac.EMU_SHAPES, ids=str)
def test_emulation_within_bounds(emulated, shape, rounded_sum):
    """Forward: below the bound with its derived factor 2, and below 0.81 of it with the factor at 1.  Backward and lse: the
    emulation needs at most half of each constant (they are twice its worst ratio)."""
    N, D, sc = shape
    for seed in range(ac.EMU_SEEDS):
        ref, e = emulated[(N, D, sc, seed, rounded_sum)]
        what = f"{shape} seed {seed} rounded_sum={rounded_sum}"
        ac.check_forward(e["o"], ref, D, what)
        assert ac.check_forward(e["o"], ref, D, what, c=1.0) <= 0.81
        ac.check_backward(e["dq"], e["dk"], e["dv"], ref, what)
        assert ac.excess_ratio(e["dv"], ref["dv"], ref["mag_dv"]) <= ac.DV_C / 2
        assert ac.excess_ratio(e["dq"], ref["dq"], ref["mag_dq"]) <= ac.DQ_C / 2
        assert ac.excess_ratio(e["dk"], ref["dk"], ref["mag_dk"]) <= ac.DK_C / 2
        assert ac.check_lse(e["lse"], ref, D, what) <= ac.LSE_C / 2


def test_bounds_catch_defects(emulated):
    """What the bounds are for: a dropped key, a missing exponential (softmax taken as a mean) and a gradient without the
    delta term all exceed them."""
    N, D, sc = ac.EMU_SHAPES[1]
    q, k, v, go = ac.make_inputs(N, D, sc, seed=0)
    ref = ac.reference(q, k, v, go)
    short = ac.emulate(q, k[:-1], v[:-1], go)
    with pytest.raises(AssertionError):
        ac.check_forward(short["o"], ref, D)
    with pytest.raises(AssertionError):
        ac.check_lse(short["lse"], ref, D)
    with pytest.raises(AssertionError):
        ac.check_forward(v.float().mean(0, keepdim=True).expand(N, D).bfloat16(), ref, D)
    e = ac.emulate(q, k, v, go)
    p = ref["P"]
    no_delta = (ref["scale"] * (p * (go.double() @ v.double().T)) @ k.double()).bfloat16()
    with pytest.raises(AssertionError):
        ac.check_backward(no_delta, e["dk"], e["dv"], ref)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ops_on_cpu_tensors(dtype, monkeypatch):
    """CPU tensors take the torch formulation whatever MK_ATTN says: value and gradients against the float64 formula."""
    from makani_amd import ops
    monkeypatch.setenv("MK_ATTN", "hip")
    B, H, N, D = 2, 3, 37, 16
    torch.manual_seed(3)
    qkv = torch.randn(B, N, 3 * H * D).to(dtype).requires_grad_(True)
    g = torch.randn(B, N, H * D).to(dtype)
    q, k, v = (t.permute(0, 2, 1, 3) for t in qkv.detach().view(B, N, 3, H, D).unbind(2))
    assert not ops.attention_supported(q, k, v)
    ref = ac.reference(q, k, v, g.view(B, N, H, D).permute(0, 2, 1, 3))
    tol = 2e-6 if dtype == torch.float32 else 2e-2

    def rel(a, b):
        return float(torch.linalg.norm(a.detach().double() - b) / torch.linalg.norm(b))

    y = ops.attention_packed(qkv, H)
    assert y.shape == (B, N, H * D) and y.dtype == dtype
    y.backward(g)
    want = torch.stack([ref["dq"], ref["dk"], ref["dv"]], 0).permute(1, 3, 0, 2, 4).reshape(B, N, 3 * H * D)
    assert rel(y, ref["o"].permute(0, 2, 1, 3).reshape(B, N, H * D)) <= tol
    assert rel(qkv.grad, want) <= tol

    qs, ks, vs = (t.clone().requires_grad_(True) for t in (q, k, v))
    o = ops.attention(qs, ks, vs, scale=None)
    assert o.shape == (B, H, N, D)
    o.backward(g.view(B, N, H, D).permute(0, 2, 1, 3))
    assert rel(o, ref["o"]) <= tol
    for got, name in ((qs.grad, "dq"), (ks.grad, "dk"), (vs.grad, "dv")):
        assert rel(got, ref[name]) <= tol, name
    # an explicit scale
    o2 = ops.attention(q, k, v, scale=0.5)
    assert rel(o2, ac.reference(q, k, v, scale=0.5)["o"]) <= tol


def test_mk_attn_is_validated_at_call_time(monkeypatch):
    from makani_amd import ops
    q = torch.randn(1, 1, 4, 16)
    monkeypatch.setenv("MK_ATTN", "flash")
    with pytest.raises(ValueError, match="MK_ATTN"):
        ops.attention(q, q, q)
    with pytest.raises(ValueError, match="MK_ATTN"):
        ops.attention_packed(torch.randn(1, 4, 48), 1)
    monkeypatch.setenv("MK_ATTN", "torch")
    assert ops.attention(q, q, q).shape == q.shape
    monkeypatch.delenv("MK_ATTN")
    assert ops.attn_hip() == (ops.ATTN_DEFAULT == "hip")
    with pytest.raises(ValueError, match="attention_packed"):
        ops.attention_packed(torch.randn(1, 4, 50), 1)


def test_info_and_refusals_without_a_device():
    """Tile sizes and the validation of sizes, strides and alignment need no GPU: code 1 before any launch."""
    import ctypes
    from makani_amd import _lib, ops
    lib = _lib.load()
    for D in (16, 32, 48, 64, 80, 96, 112, 128):
        for tq, tk in ops.attn_info(D):
            assert tq % 32 == 0 and tk % 32 == 0
    for D in (0, 8, 24, 144):
        with pytest.raises(RuntimeError, match="head size"):
            ops.attn_info(D)
    P = 4096
    good = [64 * 40, 40, 40 * 3] * 6
    for D, strides, ptr in ((40, good, P), (32, [64 * 40, 40, 36] + good[3:], P), (32, good, P + 8), (32, [64, 40, 16] + good[3:], P)):
        st = (ctypes.c_longlong * len(strides))(*strides)
        sp = ctypes.addressof(st)
        assert lib.mk_attn_fwd(ptr, P, P, P, None, 1, 2, 5, 5, D, sp, 1.0, None) == 1
        assert lib.mk_last_error()
        assert lib.mk_attn_bwd_delta(ptr, P, P, 1, 2, 5, D, sp, None) == 1
        assert lib.mk_attn_bwd_dkv(ptr, P, P, P, P, P, P, P, 1, 2, 5, 5, D, sp, 1.0, None) == 1
        assert lib.mk_attn_bwd_dq(ptr, P, P, P, P, P, P, 1, 2, 5, 5, D, sp, 1.0, None) == 1


def test_every_refusal_keeps_its_words_without_a_device():
    from makani_amd import _lib
    assert ac.check_refusal_texts(_lib.load(), "mk_attn", 128, 8) == 4 * 8 + 1 + 2 + 4 + 4
