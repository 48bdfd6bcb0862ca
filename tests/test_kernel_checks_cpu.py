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


# ---------------------------------------------------------------------------------------------------------------------
# the fp32-result criterion of the bf16x3 engine: an emulation of x3_tile's arithmetic, and seeded defects
# ---------------------------------------------------------------------------------------------------------------------
X3_K = [4, 12, 36, 70, 131, 260, 280]     # the contraction lengths of tests/test_x3_guard_gpu.py (280: 140 rows of a weight gradient)
X3_M, X3_N = 64, 96
PA, PB = (2, 0, 1, 1, 0, 0), (0, 2, 1, 0, 1, 0)      # x3_mfma_step: piece indices (0 = h, 1 = m, 2 = l), smallest products first
DROPS = {"al*bh": 0, "ah*bl": 1, "am*bm": 2}          # the three 2^-16-weight products, by their place in PA / PB


def _f32_add(acc, term64):
    """One fp32 addition: ``acc`` (fp32 values held in float64) plus an exactly known term, rounded to fp32."""
    return (acc + term64).float().double()


def x3_emulate(a, b, order, drop=None, exact_split=True):
    """``a [M, K] @ b [K, N]`` (fp32) as ``x3_tile`` evaluates it: K zero-padded to a multiple of 32, both operands split into
    three bf16 pieces, per 16-k sub-step the six piece products in the order of PA / PB, accumulated in fp32.  Every piece
    product is exact in fp32 (8 x 8 significant bits) and a sum of 16 of them is exact in float64, so the emulation only
    rounds where the accumulator does: ``order`` "group" rounds once per 16-k piece product (the matrix core adding the
    whole group to the accumulator), "sequential" once per scalar product.  ``drop``: a product (index into PA / PB) that is
    never issued.  ``exact_split=False``: the split as the kernel does it for any input (see ``kc.x3_split``).  Returns fp32."""
    M, K = a.shape
    KP = (K + 31) // 32 * 32
    ap, bp = torch.zeros(M, KP), torch.zeros(KP, b.shape[1])
    ap[:, :K], bp[:K] = a, b
    sa, sb = [p.double() for p in kc.x3_split(ap, exact_split)], [p.double() for p in kc.x3_split(bp, exact_split)]
    acc = torch.zeros(M, b.shape[1], dtype=torch.float64)
    for k0 in range(0, KP, 16):
        for t in range(6):
            if t == drop:
                continue
            pa, pb = sa[PA[t]][:, k0:k0 + 16], sb[PB[t]][k0:k0 + 16]
            if order == "group":
                acc = _f32_add(acc, pa @ pb)
            else:
                for k in range(16):
                    acc = _f32_add(acc, pa[:, k:k + 1] * pb[k:k + 1])
    return acc.float()


def f32_emulate(a, b, fused=True):
    """The fp32 MFMA of csrc/gemm.hip, without a split: a chain over k of fused multiply-adds (``fused``: the 48-bit product
    enters the addition unrounded) or of a rounded product and a rounded addition."""
    acc = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float64)
    a64, b64 = a.double(), b.double()
    for k in range(a.shape[1]):
        p = a64[:, k:k + 1] * b64[k:k + 1]
        acc = _f32_add(acc, p if fused else p.float().double())
    return acc.float()


def _real_case(K):
    g = torch.Generator().manual_seed(1000 + K)
    a, b = torch.randn(X3_M, K, generator=g), torch.randn(K, X3_N, generator=g)
    return a, b, a.double() @ b.double(), kc.absdot("mk,kn->mn", a, b)


def _complex_case(K, conj):
    """K / 2 complex terms as the engine sees them: the A image interleaves (re, im) along k, the B image holds
    (re, -im) / (im, re) rows (``CplxStager<false>``) or, conjugated, (re, im) / (-im, re) (``DgradStager``)."""
    g = torch.Generator().manual_seed(2000 + K + int(conj))
    H = (K + 1) // 2
    x = torch.complex(torch.randn(X3_M, H, generator=g), torch.randn(X3_M, H, generator=g))
    w = torch.complex(torch.randn(H, X3_N // 2, generator=g), torch.randn(H, X3_N // 2, generator=g))
    a = torch.view_as_real(x).reshape(X3_M, 2 * H)
    wr, wi = w.real, (-w.imag if conj else w.imag)
    b = torch.stack([torch.stack([wr, wi], -1), torch.stack([-wi, wr], -1)], 1).reshape(2 * H, X3_N)   # rows (i, re / im), columns (o, re / im)
    w128 = w.to(torch.complex128)
    ref = x.to(torch.complex128) @ (w128.conj() if conj else w128)
    return a.contiguous(), b.contiguous(), ref, kc.absdot("mk,kn->mn", x, w)


def _as(y, ref):
    return torch.view_as_complex(y.reshape(X3_M, -1, 2).contiguous()) if ref.is_complex() else y


def _rel(y, ref):
    return float(torch.linalg.norm(kc._components(y) - kc._components(ref)) / torch.linalg.norm(kc._components(ref)))


@pytest.fixture(scope="module")
def x3_cases():
    cases = {("real", K): _real_case(K) for K in X3_K}
    cases[("complex", 36)] = _complex_case(36, False)
    cases[("complex conj", 260)] = _complex_case(260, True)
    return cases


def test_x3_split_is_exact():
    g = torch.Generator().manual_seed(3)
    t = torch.cat([torch.randn(4096, generator=g) * s for s in (1e-20, 1.0, 1e20)] + [torch.tensor([0.0, -0.0, 1.0, -1.0, 2.0 ** -100])])
    h, m, lo = kc.x3_split(t)
    for p in (h, m, lo):
        assert torch.equal(p.bfloat16().float(), p)              # bf16 numbers
    assert bool((h.abs() <= t.abs()).all()) and bool((m.abs() <= 2.0 ** -7 * t.abs()).all()) and bool((lo.abs() <= 2.0 ** -15 * t.abs()).all())
    with pytest.raises(AssertionError):
        kc.x3_split(torch.tensor([float("nan")]))


def test_absdot_components():
    g = torch.Generator().manual_seed(4)
    x = torch.complex(torch.randn(5, 7, generator=g), torch.randn(5, 7, generator=g))
    w = torch.complex(torch.randn(7, 3, generator=g), torch.randn(7, 3, generator=g))
    mag = kc.absdot("mk,kn->mn", x, w)
    xr, xi, wr, wi = (t.double().abs() for t in (x.real, x.imag, w.real, w.imag))
    assert torch.equal(mag.real, xr @ wr + xi @ wi) and torch.equal(mag.imag, xr @ wi + xi @ wr)
    assert torch.equal(kc.absdot("mk,kn->mn", x, w.conj()), mag)
    assert torch.equal(kc.absdot("mk,kn->mn", x, w.real), torch.complex(xr @ wr, xi @ wr))      # complex rows, real weights
    assert torch.equal(kc.absdot("mk,kn->mn", x.real, w.real), xr @ wr)


def test_x3_emulation_inside_c(x3_cases):
    """Both accumulation orders pass with the chosen c, and c is twice the worst ratio of the sequential order (rounded to the
    next integer)."""
    worst = {"group": 0.0, "sequential": 0.0}
    for (kind, K), (a, b, ref, mag) in x3_cases.items():
        for order in worst:
            y = _as(x3_emulate(a, b, order), ref)
            r = kc.x3_elementwise(y, ref, mag, what=f"{kind} K={K} {order}")
            print(f"[kernel_checks] x3 emulation {kind} K={K} {order}: worst ratio {r:.2f}, whole-tensor rel {_rel(y, ref):.2e}")
            worst[order] = max(worst[order], r)
    print(f"[kernel_checks] x3 emulation worst ratios {worst}, X3_C = {kc.X3_C}")
    assert worst["group"] <= worst["sequential"]
    assert math.ceil(2 * worst["sequential"]) == kc.X3_C


def test_f32_emulation_inside_c(x3_cases):
    worst = 0.0
    for (kind, K), (a, b, ref, mag) in x3_cases.items():
        for fused in (True, False):
            r = kc.x3_elementwise(_as(f32_emulate(a, b, fused), ref), ref, mag, c=kc.F32_C, what=f"fp32 {kind} K={K} fused={fused}")
            print(f"[kernel_checks] fp32 emulation {kind} K={K} fused={fused}: worst ratio {r:.2f}")
            worst = max(worst, r)
    print(f"[kernel_checks] fp32 emulation worst ratio {worst:.2f}, F32_C = {kc.F32_C}")
    assert math.ceil(2 * worst) == kc.F32_C


def test_x3_dropped_piece_fails(x3_cases):
    """A kernel that never issues one of the three 2^-16-weight products fails, each product on its own, at every contraction
    length and in both orders -- and the whole-tensor 1e-5 norm the suite used before passes some of them (al*bh and ah*bl
    land at 9.7e-6 ... 1.0e-5, am*bm at 1.1e-5), which is why this criterion exists."""
    passes_old = []
    for piece, drop in DROPS.items():
        for (kind, K), (a, b, ref, mag) in x3_cases.items():
            for order in ("group", "sequential"):
                y = _as(x3_emulate(a, b, order, drop=drop), ref)
                with pytest.raises(AssertionError, match="worst") as e:
                    kc.x3_elementwise(y, ref, mag, what=f"dropped {piece}")
                if _rel(y, ref) < 1e-5:
                    passes_old.append((piece, kind, K, order))
                print(f"[kernel_checks] dropped {piece} {kind} K={K} {order}: rel {_rel(y, ref):.2e}; {str(e.value).split(' at ')[0]}")
    print(f"[kernel_checks] dropped pieces that pass rel < 1e-5: {len(passes_old)} of {6 * len(x3_cases)}")
    assert passes_old, "the old criterion caught every case: the record of why the new one exists is gone"


def test_x3_dropped_k_term_fails(x3_cases):
    for (kind, K), (a, b, ref, mag) in x3_cases.items():
        y = x3_emulate(a, b, "group")
        a2 = a.clone()
        a2[X3_M // 2, a.shape[1] - 1] = 0.0
        y2 = y.clone()
        y2[X3_M // 2, 5] = x3_emulate(a2, b, "group")[X3_M // 2, 5]
        assert int((y2 != y).sum()) == 1
        with pytest.raises(AssertionError, match="worst") as e:
            kc.x3_elementwise(_as(y2, ref), ref, mag, what="dropped k term")
        print(f"[kernel_checks] {kind} K={K}: rel {_rel(_as(y2, ref), ref):.2e}; {str(e.value).split(' at ')[0]}")


def test_x3_shifted_column_fails(x3_cases):
    for (kind, K), (a, b, ref, mag) in x3_cases.items():
        y = _as(x3_emulate(a, b, "group"), ref).clone()
        y[:, -2] = y[:, -1]
        with pytest.raises(AssertionError, match="worst"):
            kc.x3_elementwise(y, ref, mag, what="shifted column")


def test_x3_non_finite_fails(x3_cases):
    a, b, ref, mag = x3_cases[("real", 36)]
    y = x3_emulate(a, b, "group")
    y[3, 7] = float("nan")
    with pytest.raises(AssertionError, match="NaN or Inf"):
        kc.x3_elementwise(y, ref, mag, what="nan")
    a, b, ref, mag = x3_cases[("complex", 36)]
    y = _as(x3_emulate(a, b, "group"), ref).clone()
    y[3, 7] = complex(0.0, float("inf"))
    with pytest.raises(AssertionError, match="NaN or Inf"):
        kc.x3_elementwise(y, ref, mag, what="inf")


def test_x3_slack_and_zero_magnitude():
    """The slack is subtracted from the error before the ratio; an element whose products are all zero must be exact."""
    ref = torch.tensor([1.0, 0.0], dtype=torch.float64)
    mag = torch.tensor([1.0, 0.0], dtype=torch.float64)
    assert kc.x3_elementwise(torch.tensor([1.0, 0.0]), ref, mag) == 0.0
    with pytest.raises(AssertionError, match="worst"):
        kc.x3_elementwise(torch.tensor([1.0, 1e-30]), ref, mag)
    y = torch.tensor([1.0 + 40 * 2.0 ** -23, 0.0])
    with pytest.raises(AssertionError, match="worst"):
        kc.x3_elementwise(y, ref, mag)
    assert kc.x3_elementwise(y, ref, mag, slack64=kc.x3_slack_sum(35, mag)) <= 5.0 + 1e-6
    assert torch.equal(kc.x3_slack_add(ref), 2.0 ** -23 * ref.abs())


def test_x3_underflow_needs_its_slack():
    """An A operand that falls from 1e-33 through the subnormals (the Legendre synthesis table of a high mode next to a pole):
    the pieces below 2^-133 are lost, the element misses ``c`` by an order of magnitude -- the finding of the first run of
    tests/test_x3_guard_gpu.py on an MI355X -- and lies inside it with ``x3_slack_underflow``, which for operands of order 1 is
    too small to let a dropped piece pass."""
    g = torch.Generator().manual_seed(77)
    K = 131
    a = torch.randn(X3_M, K, generator=g) * torch.exp2(-110.0 - 40.0 * torch.rand(X3_M, K, generator=g))      # 2^-110 ... 2^-150
    b = torch.randn(K, X3_N, generator=g)
    assert bool((a.abs() < 2.0 ** -126).any()) and bool((a.abs() > 2.0 ** -120).any())
    ref, mag = a.double() @ b.double(), kc.absdot("mk,kn->mn", a, b)
    y = x3_emulate(a, b, "group", exact_split=False)
    with pytest.raises(AssertionError, match="worst"):
        kc.x3_elementwise(y, ref, mag, what="tiny operand")
    worst = kc.x3_elementwise(y, ref, mag, slack64=kc.x3_slack_underflow("mk,kn->mn", a, b), what="tiny operand, with the slack")
    print(f"[kernel_checks] operand in the subnormal range: worst ratio {worst:.2f} with the underflow slack")
    a, b, ref, mag = _real_case(280)
    slack = kc.x3_slack_underflow("mk,kn->mn", a, b)
    assert float(slack.max()) < 1e-35
    with pytest.raises(AssertionError, match="worst"):
        kc.x3_elementwise(x3_emulate(a, b, "group", drop=0), ref, mag, slack64=slack, what="dropped piece, with the slack")
