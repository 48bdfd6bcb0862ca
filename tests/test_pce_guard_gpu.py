"""The pixel-column engine (csrc/pce.hip) through the C ABI with the three criteria of tests/kernel_checks.py: every output
element within one bf16 ulp (plus the derived accumulation slack) of a float64 GEMM on the same bf16 operands, sentinel bands
around every output, NaN bands around every input.  The shapes reach every (KSP, NPH, TH, npass) the dispatch table builds."""
import math

import numpy as np
import pytest
import torch

import kernel_checks as kc

pytestmark = pytest.mark.gpu

# (M, K, P, batch) -> what it reaches
SHAPES = [
    (800, 96, 136, 1),                # npass 3 with a ragged last pass, one phase
    (1536, 768, 72, 1),               # npass 4 full, six phases
    (1300, 600, 200, 2),              # npass 4 ragged, five phases padded to six
    (385, 385, 520, 1),               # one row in the second pass, four phases padded to six
    (129, 129, 392, 1),               # TH 6 nearly empty, nearly empty second phase
    (65, 32, 136, 2),                 # TH 1 / 2 and KSP 2 / 4 boundaries
    (64, 33, 264, 1),
    (100, 520, 8, 3),                 # TH 2, P = 8 (the least the entry point takes)
    (73, 73, 1048, 1),                # production row counts
    (768, 384, 128 * 140 + 40, 2),    # two passes on workgroup pairs, ragged second half
]


class Engine:
    """One GEMM shape: operands between NaN bands, every launch into guarded outputs."""

    def __init__(self, dev, M, K, P, B, reference=True):
        from makani_amd import _lib
        self.lib, self.dev, self.dims = _lib.load(), dev, (M, K, P, B)
        torch.manual_seed(M * 7 + K)
        self.w = (torch.randn(M, K, device=dev) / math.sqrt(K))
        self.x = kc.poisoned(torch.randn(B, K, P, device=dev).bfloat16())
        if not reference:
            return
        self.w64, self.x64 = self.w.bfloat16().double(), self.x.double()
        self.acc = torch.matmul(self.w64, self.x64)
        self.gamma = kc.gemm_gamma(self.w64, self.x64)

    def pack(self, w, transpose):
        from makani_amd import _lib, ops
        M, K, _, _ = self.dims
        n = self.lib.mk_pce_image_bytes(M, K)
        assert n > 0
        img, check = kc.guarded((n,), torch.uint8, self.dev, fill=0xA5)
        _lib.check(self.lib.mk_pce_pack(w.data_ptr(), 0 if w.dtype == torch.float32 else 1, int(transpose), M, K, w.stride(0),
                                        img.data_ptr(), ops._stream()), "mk_pce_pack")
        torch.cuda.synchronize()
        check(f"mk_pce_pack {self.dims}")
        return img

    def launch(self, img, bias=None, addend=None, aff=None, aux_in=None, want_pre=False, gelu=False, stats=False, expect_rc0=True):
        """Returns (rc, y, pre, sums); after a launch every guard band is intact and no output element is NaN or Inf."""
        from makani_amd import ops
        M, K, P, B = self.dims
        y, cy = kc.guarded((B, M, P), torch.bfloat16, self.dev)
        pre, cp = kc.guarded((B, M, P), torch.bfloat16, self.dev) if want_pre else (None, None)
        sums, cs = kc.guarded((B * M, 2), torch.float64, self.dev) if stats else (None, None)
        ptr = lambda t: None if t is None else t.data_ptr()
        rc = self.lib.mk_pce_gemm_ex(self.x.data_ptr(), img.data_ptr(), y.data_ptr(), ptr(bias), ptr(addend), ptr(aff), ptr(aux_in),
                                     ptr(pre), int(gelu), ptr(sums), B, M, K, P, ops._stream())
        torch.cuda.synchronize()
        what = f"mk_pce_gemm_ex {self.dims} bias={bias is not None} gelu={gelu} pre={want_pre} addend={addend is not None} " \
               f"affine={aff is not None} aux_in={aux_in is not None} stats={stats}"
        for c in (cy, cp, cs):
            if c is not None:
                c(what)
        if expect_rc0:
            assert rc == 0, f"{what}: {self.lib.mk_last_error().decode()}"
            for t in (y, pre, sums):
                assert t is None or bool(torch.isfinite(t).all()), f"{what}: NaN or Inf in an output"
        return rc, y, pre, sums

    def record(self, name, y, ref, slack):
        worst = kc.bf16_elementwise(y, ref, slack, what=f"{name} {self.dims}")
        print(f"[pce guard] {self.dims} {name}: worst |err| / bound {worst:.3f}")

    def check_sums(self, y, sums):
        """Row sums against the sums of the stored y, under the tolerances of tests/test_pce_gpu.py::test_pce_row_sums."""
        _, _, P, _ = self.dims
        yd = y.double().view(-1, P)
        np.testing.assert_allclose(sums[:, 0].cpu().numpy(), yd.sum(1).cpu().numpy(), rtol=1e-4, atol=1e-3 * math.sqrt(P))
        np.testing.assert_allclose(sums[:, 1].cpu().numpy(), (yd * yd).sum(1).cpu().numpy(), rtol=1e-4)


@pytest.mark.parametrize("M,K,P,B", SHAPES)
def test_pce_every_element_guarded(dev, M, K, P, B):
    e = Engine(dev, M, K, P, B)
    img = e.pack(e.w, False)
    # plain GEMM; fp32 or bf16 weights, given as W or as W^T (the data gradient's A = W^T), give the same bits
    _, y0, _, _ = e.launch(img)
    e.record("plain", y0, e.acc, kc.slack_plain(e.gamma))
    wt = e.w.t().contiguous()
    for name, w, transpose in (("bf16 weights", e.w.bfloat16(), False), ("transposed fp32 image", wt, True),
                               ("transposed bf16 image", wt.bfloat16(), True)):
        _, yt, _, _ = e.launch(e.pack(w, transpose))
        e.record(f"plain, {name}", yt, e.acc, kc.slack_plain(e.gamma))
        assert torch.equal(yt, y0), name

    torch.manual_seed(11)
    bias = kc.poisoned(torch.randn(M, device=dev))
    add = kc.poisoned(torch.randn(B, M, P, device=dev).bfloat16())
    aux = kc.poisoned(torch.randn(B, M, P, device=dev).bfloat16())
    aff = kc.poisoned(torch.randn(B * M, 2, device=dev))
    pre64 = e.acc + bias.double().view(1, -1, 1)
    term64 = aff[:, 0].double().view(B, M, 1) * add.double() + aff[:, 1].double().view(B, M, 1)
    variants = [        # name, launch arguments, reference of y, slack of y
        ("bias + GELU", dict(bias=bias, gelu=True, want_pre=True), kc.gelu64(pre64), kc.slack_gelu(e.gamma, pre64)),
        ("addend", dict(addend=add), e.acc + add.double(), kc.slack_addend(e.gamma, add.double(), e.acc + add.double())),
        ("aux_in", dict(aux_in=aux), e.acc * kc.gelu_grad64(aux.double()), kc.slack_aux(e.gamma)),
        ("addend, affine", dict(addend=add, aff=aff), e.acc + term64, kc.slack_addend(e.gamma, term64, e.acc + term64)),
    ]
    for name, kw, ref, slack in variants:
        _, y, pre, _ = e.launch(img, **kw)
        e.record(name, y, ref, slack)
        if pre is not None:
            e.record("pre-activation", pre, pre64, kc.slack_pre(e.gamma, pre64))
        if M <= 768:        # with the row statistics: the same bits, and the sums of what was stored
            _, ys, pres, sums = e.launch(img, stats=True, **kw)
            assert torch.equal(ys, y) and (pre is None or torch.equal(pres, pre))
            e.check_sums(ys, sums)
    if M <= 768:
        _, ys, _, sums = e.launch(img, stats=True)
        assert torch.equal(ys, y0)
        e.check_sums(ys, sums)
        # bias + GELU without a stored pre-activation, with and without the statistics
        _, yg, _, _ = e.launch(img, bias=bias, gelu=True)
        e.record("bias + GELU, no pre-activation", yg, variants[0][2], variants[0][3])
        _, ys, _, sums = e.launch(img, bias=bias, gelu=True, stats=True)
        assert torch.equal(ys, yg)
        e.check_sums(ys, sums)


def test_pce_refusals_leave_the_output_alone(dev):
    """Row statistics with M > 768, K = 769 and M = 1537 are refused with a message; a refused call writes nothing."""
    from makani_amd import ops
    for (M, K, stats) in ((800, 96, True), (64, 769, False), (1537, 64, False)):
        e = Engine(dev, M, K, 136, 1, reference=False)
        img = torch.zeros(max(e.lib.mk_pce_image_bytes(M, K), 4096), dtype=torch.uint8, device=dev)
        rc, y, _, sums = e.launch(img, stats=stats, expect_rc0=False)
        assert rc != 0 and e.lib.mk_last_error().decode() != "", (M, K, stats)
        assert bool((y == kc.SENTINEL).all()) and (sums is None or bool((sums == kc.SENTINEL).all()))
    assert ops.pce_supported(1536, 768) and not ops.pce_supported(1537, 768) and not ops.pce_supported(1536, 769)

