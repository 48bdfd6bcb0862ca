"""The bounds of tests/x3_attn_checks.py against the CPU emulation of the fp32 attention kernels (csrc/x3_attn.hip), the planted
defects, and what the fp32 attention path does without a device: the knob, the tile sizes, the refusals, CPU tensors."""
import ctypes
import functools

import pytest
import torch

import attn_checks as ac
import x3_attn_checks as xc


def test_emulation_stays_within_half_of_each_constant():
    worst = {}
    for N, D, in_scale in xc.EMU_SHAPES:
        for seed in range(xc.EMU_SEEDS):
            q, k, v, go = xc.make_inputs(N, D, in_scale, seed=seed)
            for n, x in xc.ratios(xc.emulate(q, k, v, go), ac.reference(q, k, v, go)).items():
                worst[n] = max(worst.get(n, 0.0), x)
    print({n: round(x, 3) for n, x in worst.items()})
    recorded = dict(o=xc.EMU_WORST_O, lse=xc.EMU_WORST_LSE, dq=xc.EMU_WORST_DQ, dk=xc.EMU_WORST_DK, dv=xc.EMU_WORST_DV)
    for n, x in worst.items():
        assert x <= 0.5 * xc.CONSTANTS[n], (n, x)
        # the figure moves with the summation order of the host's fp32 matmul: the record is held loosely, the constant is not
        assert x <= 1.1 * recorded[n] + 0.01, f"{n}: the emulation reaches {x:.3f}, the module records {recorded[n]}"
        assert xc.CONSTANTS[n] == float(-(-2.0 * recorded[n] // 1)), f"{n}: the constant is not twice the recorded figure, rounded up"


@functools.lru_cache(maxsize=None)
def _defect_case(N, D):
    """Operands at a shape of the GPU test (its B = 2, H = 3, its seed) and their reference, computed once."""
    q, k, v, go = xc.make_inputs(N, D, 1.0, seed=1, lead=(2, 3))
    ref = ac.reference(q, k, v, go)
    clean = xc.emulate(q, k, v, go)
    for n in xc.CONSTANTS:
        xc.check(n, clean[n], ref, f"N={N} D={D}")
    return q, k, v, go, ref


# the result a product feeds first: a defect must push THAT result past its bound
_SEEN_IN = dict(s="o", pv="o", bs="dv", dp="dq", dv="dv", dq="dq", dk="dk")


@pytest.mark.parametrize("t", xc.DROPS)
@pytest.mark.parametrize("product", xc.PRODUCTS)
@pytest.mark.parametrize("N,D", xc.DEFECT_SHAPES)
def test_a_dropped_piece_product_exceeds_its_bound(N, D, product, t):
    q, k, v, go, ref = _defect_case(N, D)
    bad = xc.emulate(q, k, v, go, drop=(product, t))
    name = _SEEN_IN[product]
    with pytest.raises(AssertionError, match="exceed the limit"):
        xc.check(name, bad[name], ref)


@pytest.mark.parametrize("N,D", xc.DEFECT_SHAPES)
def test_a_missing_key_exceeds_every_bound(N, D):
    q, k, v, go, ref = _defect_case(N, D)
    bad = xc.emulate(q, k, v, go, drop_key=(N // 2, N - 1))
    for name in xc.CONSTANTS:
        with pytest.raises(AssertionError, match="exceed the limit"):
            xc.check(name, bad[name], ref)


def test_defect_shapes_are_shapes_of_the_gpu_test():
    from makani_amd import ops
    for N, D in xc.DEFECT_SHAPES:
        counts = set()
        for tq, tk in ops.attn_x3_info(D):
            counts |= {1, tk - 1, tk, tk + 1, tq + 1, 2 * max(tq, tk) + 3}
        assert N in counts and N <= 300, (N, D, sorted(counts))


def test_mk_attn_fp32_is_validated_at_call_time(monkeypatch):
    from makani_amd import ops
    q = torch.randn(1, 1, 4, 16)
    monkeypatch.setenv("MK_ATTN_FP32", "x3")
    with pytest.raises(ValueError, match="MK_ATTN_FP32"):
        ops.attention(q, q, q)
    with pytest.raises(ValueError, match="MK_ATTN_FP32"):
        ops.attention_packed(torch.randn(1, 4, 48), 1)
    monkeypatch.setenv("MK_ATTN_FP32", "hip")
    assert ops.attn_fp32_hip() and ops.attention(q, q, q).shape == q.shape
    monkeypatch.delenv("MK_ATTN_FP32")
    assert ops.ATTN_FP32_DEFAULT == "torch" and not ops.attn_fp32_hip()


def test_info_and_refusals_without_a_device():
    """Tile sizes and the validation of sizes, strides and alignment need no GPU: code 1 before any launch."""
    from makani_amd import _lib, ops
    lib = _lib.load()
    for D in (16, 32, 48, 64):
        for tq, tk in ops.attn_x3_info(D):
            assert tq % 32 == 0 and tk % 32 == 0
    for D in (0, 8, 24, 80, 128, 144):
        with pytest.raises(RuntimeError, match="head size"):
            ops.attn_x3_info(D)
    P = 4096
    good = [64 * 40, 40, 40 * 3] * 6
    cases = ((40, good, P, 5),                                   # head size
             (32, [64 * 40, 40, 34] + good[3:], P, 5),           # a stride that is no multiple of 4
             (32, good, P + 8, 5),                               # alignment
             (32, [64, 40, 16] + good[3:], P, 5),                # token stride below the head size
             (32, good, P, 2 ** 30))                             # B H N past the 32-bit row range
    for D, strides, ptr, N in cases:
        st = (ctypes.c_longlong * len(strides))(*strides)
        sp = ctypes.addressof(st)
        assert lib.mk_attn_x3_fwd(ptr, P, P, P, None, 1, 2, N, N, D, sp, 1.0, None) == 1
        assert lib.mk_last_error()
        assert lib.mk_attn_x3_bwd_delta(ptr, P, P, 1, 2, N, D, sp, None) == 1
        assert lib.mk_attn_x3_bwd_dkv(ptr, P, P, P, P, P, P, P, 1, 2, N, N, D, sp, 1.0, None) == 1
        assert lib.mk_attn_x3_bwd_dq(ptr, P, P, P, P, P, P, 1, 2, N, N, D, sp, 1.0, None) == 1
    st = (ctypes.c_longlong * len(good))(*good)
    assert lib.mk_attn_x3_bwd_dq(P, P, P, P, None, P, P, 1, 2, 5, 5, 32, ctypes.addressof(st), 1.0, None) == 1     # null lse


def test_every_refusal_keeps_its_words_without_a_device():
    from makani_amd import _lib
    assert ac.check_refusal_texts(_lib.load(), "mk_attn_x3", 64, 4) == 4 * 8 + 1 + 2 + 4 + 4


@pytest.mark.parametrize("knob", ["hip", "torch"])
def test_cpu_tensors_take_the_torch_call_bit_for_bit(knob, monkeypatch):
    from makani_amd import ops
    monkeypatch.setenv("MK_ATTN_FP32", knob)
    B, H, N, D = 2, 3, 37, 16
    torch.manual_seed(3)
    qkv = torch.randn(B, N, 3 * H * D)
    g = torch.randn(B, N, H * D)
    q, k, v = (t.permute(0, 2, 1, 3) for t in qkv.view(B, N, 3, H, D).unbind(2))
    assert not ops.attention_x3_supported(q, k, v)

    def run(packed, ours):
        x = qkv.clone().requires_grad_(True)
        if packed and ours:
            y = ops.attention_packed(x, H)
        else:
            qq, kk, vv = (t.permute(0, 2, 1, 3) for t in x.reshape(B, N, 3, H, D).unbind(2))
            o = ops.attention(qq, kk, vv) if ours else torch.nn.functional.scaled_dot_product_attention(qq, kk, vv)
            y = o.transpose(1, 2).reshape(B, N, H * D)
        y.backward(g)
        return y.detach(), x.grad

    for packed in (False, True):
        (y, gx), (y0, gx0) = run(packed, True), run(packed, False)
        assert torch.equal(y, y0) and torch.equal(gx, gx0)
