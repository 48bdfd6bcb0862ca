"""The checker checked (tests/kernel_checks.py), on the CPU: an fp32 emulation of the pixel-column engine's arithmetic -- bf16
operands, fp32 accumulation, the epilogue's rational-exponential CDF in fp32, one rounding to bf16 -- stays inside
``bf16_elementwise`` with the derived slack, and three small defects of the kind a ragged tile produces do not."""
import math

import pytest
import torch

import kernel_checks as kc

SHAPES = [(73, 600, 264, 2), (1536, 768, 136, 1), (384, 384, 1000, 2), (16, 8, 2048, 2)]     # (M, K, P, B)


def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def _cdf_pdf(x):
    """normal_cdf_pdf of csrc/pce_common.h in fp32: Phi through erfc(|x| / sqrt 2) in the Abramowitz-Stegun 7.1.26 form."""
    one = torch.ones_like(x)
    z = x.abs() * torch.tensor(0.70710678118654752, dtype=torch.float32)
    t = one / _fma(torch.full_like(x, 0.3275911), z, one)
    q = _fma(torch.full_like(x, 1.061405429), t, torch.full_like(x, -1.453152027))
    for c in (1.421413741, -0.284496736, 0.254829592):
        q = _fma(q, t, torch.full_like(x, c))
    e = torch.exp2(torch.tensor(-1.4426950408889634, dtype=torch.float32) * z * z)
    half_erfc = torch.tensor(0.5, dtype=torch.float32) * q * t * e
    return torch.where(x < 0, half_erfc, one - half_erfc), torch.tensor(0.3989422804014327, dtype=torch.float32) * e


def _emulated(M, K, P, B):
    """Operands, the three emulated bf16 outputs and their float64 references with slack."""
    torch.manual_seed(M * 7 + K)
    w = (torch.randn(M, K) / math.sqrt(K)).bfloat16()
    x = torch.randn(B, K, P).bfloat16()
    bias = torch.randn(M)
    aux = torch.randn(B, M, P).bfloat16()
    acc = torch.matmul(w.float(), x.float())                       # fp32 accumulation of exact products
    pre = acc + bias.view(1, -1, 1)
    Phi, _ = _cdf_pdf(pre)
    Pa, pa = _cdf_pdf(aux.float())
    out = {"plain": acc.bfloat16(), "gelu": (pre * Phi).bfloat16(), "gelu_grad": (acc * _fma(aux.float(), pa, Pa)).bfloat16()}
    w64, x64 = w.double(), x.double()
    acc64 = torch.matmul(w64, x64)
    pre64 = acc64 + bias.double().view(1, -1, 1)
    gamma = kc.gemm_gamma(w64, x64)
    ref = {"plain": (acc64, kc.slack_plain(gamma)), "gelu": (kc.gelu64(pre64), kc.slack_gelu(gamma, pre64)),
           "gelu_grad": (acc64 * kc.gelu_grad64(aux.double()), kc.slack_aux(gamma))}
    return w, x, out, ref


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "x".join(map(str, s)))
def case(request):
    return _emulated(*request.param)


def test_emulated_engine_passes_the_bound(case):
    _, _, out, ref = case
    for name in ("plain", "gelu", "gelu_grad"):
        worst = kc.bf16_elementwise(out[name], *ref[name], what=name)
        # measured 0.45 ... 0.50: half an ulp of the final rounding, the accumulation error far below its worst case
        print(f"[kernel_checks] emulated {name} {tuple(out[name].shape)}: worst |err| / bound {worst:.2f}")


def test_three_ulp_nudge_fails(case):
    _, _, out, ref = case
    y = out["plain"].clone()
    flat = int(torch.argmax(ref["plain"][0].abs()))                 # an element well above the rms / 256 floor
    v = y.flatten()[flat].double()
    y.view(-1)[flat] = (v + 3 * kc.bf16_ulp(v.abs())).to(torch.bfloat16)
    assert float((y.view(-1)[flat].double() - v).abs()) >= 3 * float(kc.bf16_ulp(v.abs()))
    with pytest.raises(AssertionError, match="worst"):
        kc.bf16_elementwise(y, *ref["plain"], what="nudged")


def test_dropped_k_term_fails(case):
    w, x, out, ref = case
    m, k = w.shape[0] // 2, w.shape[1] - 1
    w2 = w.float().clone()
    w2[m, k] = 0.0
    y = out["plain"].clone()
    y[:, m, :] = torch.matmul(w2[m:m + 1], x.float())[:, 0, :].bfloat16()
    assert int((y != out["plain"]).any(-1).sum()) <= y.shape[0]           # one row per batch item changed, nothing else
    with pytest.raises(AssertionError, match="worst"):
        kc.bf16_elementwise(y, *ref["plain"], what="dropped k term")


def test_shifted_column_fails(case):
    _, _, out, ref = case
    y = out["plain"].clone()
    p = y.shape[-1] - 9
    y[..., p] = out["plain"][..., p + 1]
    with pytest.raises(AssertionError, match="worst"):
        kc.bf16_elementwise(y, *ref["plain"], what="shifted column")


def test_non_finite_output_fails(case):
    _, _, out, ref = case
    y = out["plain"].clone()
    y.view(-1)[5] = float("nan")
    with pytest.raises(AssertionError, match="NaN or Inf"):
        kc.bf16_elementwise(y, *ref["plain"], what="nan")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.float64, torch.complex64])
def test_guarded_detects_one_byte(dtype):
    for shape in ((3, 5, 7), (1,), (2, 1031)):
        view, check = kc.guarded(shape, dtype, "cpu")
        lo, hi = check.span
        item = view.element_size()
        assert view.data_ptr() % 16 == 0 and view.is_contiguous() and tuple(view.shape) == shape
        assert lo * item >= 4096 and (check.buffer.numel() - hi) * item >= 4096
        fill = kc.SENTINEL_C if dtype.is_complex else kc.SENTINEL
        assert bool((view == fill).all())
        view.zero_()                                         # writing the tensor itself leaves the bands alone
        check("untouched")
        raw = kc._bits(check.buffer)                         # a view: shares the buffer's storage
        for byte in (lo * item - 1, hi * item, 0, raw.numel() - 1):
            old = int(raw[byte])
            raw[byte] = old ^ 1
            with pytest.raises(AssertionError, match="guard band"):
                check("one byte")
            raw[byte] = old
            check("restored")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.complex64])
def test_poisoned_is_bit_equal(dtype):
    torch.manual_seed(1)
    t = torch.randn(3, 7, 11, dtype=torch.float32).to(dtype) if not dtype.is_complex else torch.randn(3, 7, 11, dtype=dtype)
    p = kc.poisoned(t)
    assert p.data_ptr() % 16 == 0 and p.is_contiguous() and p.shape == t.shape and p.dtype == t.dtype
    assert torch.equal(kc._bits(p), kc._bits(t))
    assert bool(torch.isfinite(torch.view_as_real(p) if dtype.is_complex else p).all())
    # the elements next to the view, on both sides, are NaN
    base = p.as_strided((p.numel() + 2,), (1,), p.storage_offset() - 1)
    ends = torch.view_as_real(base[[0, -1]]) if dtype.is_complex else base[[0, -1]]
    assert bool(torch.isnan(ends).all())
