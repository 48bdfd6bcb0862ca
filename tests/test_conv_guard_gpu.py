"""The two 1x1-convolution GEMM families (csrc/conv_gemm.hip: bf16 weight gradient; csrc/x3_conv.hip: fp32 fields on the bf16x3
engine) through the C ABI under the relative-L2 limits tests/test_kernels_gpu.py already holds them to, now with sentinel bands
around every output and NaN bands (and NaN gap columns) around the streamed operand: a store past a ragged tile or a read past
the logical end of a row fails the test."""
import pytest
import torch

import kernel_checks as kc

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _rel(a, b):
    return float(torch.linalg.norm(a.double() - b) / torch.linalg.norm(b))


def _row_rel(got, want):
    return float(kc.row_rel(got.double().cpu().numpy(), want.cpu().numpy()).max())


# ----------------------------------------------------------------------------------------------- bf16 weight gradient
WGRAD = [(3, 5, 7, 24), (1, 129, 65, 520), (2, 73, 384, 1000), (1, 384, 73, 16384 + 8)]          # (B, O, I, P)
WGRAD_ACT = WGRAD + [(2, 96, 40, 392), (1, 200, 130, 520), (1, 384, 136, 1032)]                   # one O in each dispatch range


def _wgrad_case(dev, B, O, I, P, scale=1.0):
    g = torch.Generator().manual_seed(9)
    gy = torch.randn(B, O, P, generator=g).to(torch.bfloat16)
    x = (torch.randn(B, I, P, generator=g) * scale).to(torch.bfloat16)
    gw, check = kc.guarded((O, I), torch.float32, dev)
    gw.zero_()
    return kc.poisoned(gy, dev), kc.poisoned(x, dev), gw, check


@pytest.mark.parametrize("B,O,I,P", WGRAD)
def test_conv1x1_wgrad_guarded(dev, B, O, I, P):
    from makani_amd import _lib, ops
    gy, x, gw, check = _wgrad_case(dev, B, O, I, P)
    _lib.check(_lib.load().mk_conv1x1_wgrad(gy.data_ptr(), x.data_ptr(), gw.data_ptr(), B, O, I, P, ops._stream()), "mk_conv1x1_wgrad")
    torch.cuda.synchronize()
    check(f"mk_conv1x1_wgrad {(B, O, I, P)}")
    assert bool(torch.isfinite(gw).all())
    want = torch.einsum("bop,bip->oi", gy.double(), x.double())
    e = _rel(gw, want)
    print(f"[conv guard] wgrad {(B, O, I, P)}: {e:.2e}, worst row {_row_rel(gw, want):.2e}")
    assert e < 2e-6      # exact bf16 products, fp32 accumulation


@pytest.mark.parametrize("B,O,I,P", WGRAD_ACT)
def test_conv1x1_wgrad_act_guarded(dev, B, O, I, P):
    """x_act = 1: the second operand is GELU(x), exact erf form, rounded to bf16 while it is staged (include/makani_amd.h), so
    the reference is the float64 einsum of gy with the float64 GELU of x rounded to bf16 at the same point.  From there on the
    products are exact and the accumulation is fp32 as in the plain kernel, and the limit is the plain kernel's 2e-6, with
    x_act = 1 and with x_act = 0 through the same entry point.  The kernel's CDF (Abramowitz-Stegun 7.1.26, under 1.5e-7
    absolute) can put a value whose GELU lies that close to a rounding midpoint on the neighbouring bf16 number; what that
    adds is part of the error held to the limit (3.5e-7 ... 4.0e-7 in all, against 1.1e-7 ... 1.7e-7 for x_act = 0)."""
    from makani_amd import _lib, ops
    lib = _lib.load()
    gy, x, gw, check = _wgrad_case(dev, B, O, I, P, scale=1.5)
    for x_act in (1, 0):
        gw.zero_()
        _lib.check(lib.mk_conv1x1_wgrad_act(gy.data_ptr(), x.data_ptr(), gw.data_ptr(), B, O, I, P, x_act, ops._stream()),
                   "mk_conv1x1_wgrad_act")
        torch.cuda.synchronize()
        check(f"mk_conv1x1_wgrad_act {(B, O, I, P)} x_act={x_act}")
        assert bool(torch.isfinite(gw).all())
        h = kc.gelu64(x.double()).to(torch.bfloat16).double() if x_act else x.double()
        want = torch.einsum("bop,bip->oi", gy.double(), h)
        e = _rel(gw, want)
        print(f"[conv guard] wgrad_act {(B, O, I, P)} x_act={x_act}: {e:.2e}, worst row {_row_rel(gw, want):.2e}")
        assert e < 2e-6


# ----------------------------------------------------------------------------------------------- fp32 fields, bf16x3 engine
X3 = [(3, 5, 7, 24), (1, 200, 130, 2050), (2, 73, 384, 2112), (1, 384, 73, 4104)]                  # (B, M, K, N)
GAP = 8          # ldb = N + GAP, ldc = N + GAP: strided rows


def _strided_nan(t, dev):
    """``t`` [.., rows, n] as rows of length n + GAP whose gap columns are NaN, between NaN bands."""
    full = torch.full(tuple(t.shape[:-1]) + (t.shape[-1] + GAP,), float("nan"), dtype=t.dtype)
    full[..., :t.shape[-1]] = t
    return kc.poisoned(full, dev)


def _check_rows(name, c, check, n, want):
    """Guard bands, sentinel gap columns, finite values, and both limits: 2e-6 over the tensor (as before) and TOL per row."""
    torch.cuda.synchronize()
    check(name)
    assert bool((c[..., n:] == kc.SENTINEL).all()), f"{name}: a gap column of c was written"
    got = c[..., :n]
    assert bool(torch.isfinite(got).all()), f"{name}: NaN or Inf in the output"
    e, er = _rel(got, want), _row_rel(got, want)
    print(f"[conv guard] {name}: {e:.2e}, worst row {er:.2e}")
    assert e < 2e-6 and er < TOL


@pytest.mark.parametrize("B,M,K,N", X3)
def test_conv1x1_x3_guarded(dev, B, M, K, N):
    from makani_amd import _lib, ops
    lib = _lib.load()
    g = torch.Generator().manual_seed(5)
    w = torch.randn(M, K, generator=g) / K ** 0.5
    x = torch.randn(B, K, N, generator=g)
    add = torch.randn(B, M, N, generator=g)
    gy = torch.randn(B, M, N, generator=g)
    bias = torch.randn(M, generator=g)
    k4 = (K + 3) // 4 * 4
    a = torch.zeros(M, k4)
    a[:, :K] = w
    a, b, biasd = a.to(dev), _strided_nan(x, dev), kc.poisoned(bias, dev)
    ldb = ldc = N + GAP
    w64, x64 = w.double().to(dev), x.double().to(dev)
    want = torch.matmul(w64, x64)
    pre = want + bias.double().to(dev).view(1, -1, 1)
    for mode, ref in ((0, want), (1, want + add.double().to(dev))):
        c, check = kc.guarded((B, M, ldc), torch.float32, dev)
        if mode == 1:
            c[..., :N] = add.to(dev)
        _lib.check(lib.mk_conv1x1_x3(a.data_ptr(), k4, b.data_ptr(), ldb, c.data_ptr(), ldc, M, K, N, B, 0, K * ldb, M * ldc, mode,
                                     ops._stream()), "mk_conv1x1_x3")
        _check_rows(f"x3 mode {mode} {(B, M, K, N)}", c, check, N, ref)
    for act, ref in ((0, pre), (1, kc.gelu64(pre))):
        c, check = kc.guarded((B, M, ldc), torch.float32, dev)
        _lib.check(lib.mk_conv1x1_x3_bias_act(a.data_ptr(), k4, b.data_ptr(), ldb, c.data_ptr(), ldc, M, K, N, B, K * ldb, M * ldc,
                                              biasd.data_ptr(), act, ops._stream()), "mk_conv1x1_x3_bias_act")
        _check_rows(f"x3 bias act={act} {(B, M, K, N)}", c, check, N, ref)
    # mode 2, the weight gradient gw[m][k] = sum_{b, n} gy[b][m][n] x[b][k][n]: the contraction runs over the N pixels, the
    # rows of both operands; x keeps its strided NaN-gapped rows, gw [M][K] gets strided rows too
    ldg = K + GAP
    gw, check = kc.guarded((M, ldg), torch.float32, dev)
    gw[:, :K] = 0.0
    gyd = kc.poisoned(gy, dev)
    rc = lib.mk_conv1x1_x3(gyd.data_ptr(), N, b.data_ptr(), ldb, gw.data_ptr(), ldg, M, N, K, B, M * N, K * ldb, 0, 2, ops._stream())
    if N % 4:
        # documented: the weight gradient needs a contraction length that is a multiple of 4; the refusal leaves gw alone
        torch.cuda.synchronize()
        check(f"x3 mode 2 {(B, M, K, N)} refused")
        assert rc != 0 and "the contraction length must be multiples of 4" in lib.mk_last_error().decode()
        assert bool((gw[:, :K] == 0).all()) and bool((gw[:, K:] == kc.SENTINEL).all())
        return
    _lib.check(rc, "mk_conv1x1_x3 mode 2")
    _check_rows(f"x3 mode 2 {(B, M, K, N)}", gw, check, K, torch.einsum("bmn,bkn->mk", gy.double().to(dev), x64))
