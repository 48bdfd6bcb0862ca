"""The channels-last AFNO on the device: the two layout kernels, the block MLP's forward with biases and the latitude DFT on
window tables through the C ABI (guard bands, poisoned inputs, per-element bounds: the helpers of ``tests/kernel_checks.py`` and
``tests/test_x3_guard_gpu.py``); ``ops.spec_block_mlp`` with biases and ``AFNO2D`` (v1) on its fused path against the float64 chains
of ``tests/test_afnov1_cpu.py``; fused against the torch path; the recorded reference run of the tiny net (fp32, bf16 autocast, with
the token norm and token linear kernels); a captured step.

Criterion for the chains: relative L2 error <= 1e-5 forward and <= 5e-5 for gradients against float64 (``tests/test_afno_gpu.py``).
Every float64 reference asserts that no masked argument lies within 1e-5 rms of its edge."""
import gc

import pytest
import torch

import kernel_checks as kc
from kernel_checks import node_kinds as _graph_kinds
from test_afno_gpu import CHAIN_CASES, EDGE, GRAD_TOL, TOL, _count_calls
from test_afnov1_cpu import (LAM, block_chain64, build, check_against_fixture, make_filter, ref, window_chain64,  # noqa: F401
                             window_matrix)
from test_afno_cpu import rel as trel
from test_x3_guard_gpu import _c128, _check, _crand, _gen, _relu_parts, _shrink

pytestmark = pytest.mark.gpu


def _hip(monkeypatch):
    monkeypatch.setenv("MK_AFNOV1", "hip")
    monkeypatch.setenv("MK_PLANAR_FFT", "hip")


# ---------------------------------------------------------------------------------------------------------------------
# 1. the layout kernels through the C ABI
# ---------------------------------------------------------------------------------------------------------------------
# (B, N, C): below, at and above the 64-wide tile in each axis, rows that are and are not whole 16-byte vectors.  The last two take
# the vector path with ragged tiles: (2, 72, 136) in both dtypes, (1, 68, 12) in fp32 only (12 bf16 are no whole vector).
LAYOUT = [(1, 1, 1), (2, 33, 31), (2, 63, 65), (1, 64, 64), (2, 130, 24), (1, 37, 8), (2, 72, 136), (1, 68, 12)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,N,C", LAYOUT)
def test_layout_kernels(dev, B, N, C, dtype):
    """Bit-equal to ``x.transpose(1, 2).contiguous()`` and to ``r.transpose(1, 2) + addend``; outputs between guard bands, inputs
    between NaN bands (a read outside an operand would carry a NaN into the result or leave the sentinel)."""
    from makani_amd import _lib, ops
    lib, st, code = _lib.load(), ops._stream(), 0 if dtype == torch.float32 else 1
    g = _gen(21, B, N, C)
    tok, fld, add = (torch.randn(*s, generator=g).to(dtype) for s in ((B, N, C), (B, C, N), (B, N, C)))
    tokd, fldd, addd = (kc.poisoned(t, dev) for t in (tok, fld, add))
    bits = torch.int32 if dtype == torch.float32 else torch.int16

    def same(out, want, check, what):
        torch.cuda.synchronize()
        check(what)
        assert torch.equal(out.cpu().view(bits), want.contiguous().view(bits)), what

    out, check = kc.guarded((B, C, N), dtype, dev)
    _lib.check(lib.mk_tokens_to_fields(tokd.data_ptr(), out.data_ptr(), code, B, N, C, st), "mk_tokens_to_fields")
    same(out, tok.transpose(1, 2), check, f"tokens_to_fields {(B, N, C)}")
    out, check = kc.guarded((B, N, C), dtype, dev)
    _lib.check(lib.mk_fields_to_tokens(fldd.data_ptr(), None, out.data_ptr(), code, B, N, C, st), "mk_fields_to_tokens")
    same(out, fld.transpose(1, 2), check, f"fields_to_tokens {(B, N, C)}")
    out, check = kc.guarded((B, N, C), dtype, dev)
    _lib.check(lib.mk_fields_to_tokens(fldd.data_ptr(), addd.data_ptr(), out.data_ptr(), code, B, N, C, st), "mk_fields_to_tokens")
    same(out, fld.transpose(1, 2) + add, check, f"fields_to_tokens + addend {(B, N, C)}")


def test_layout_ops_and_their_gradients(dev):
    """The autograd pair on the device: each one's backward is the other kernel; the addend's gradient is the incoming one."""
    from makani_amd import ops
    g = _gen(22)
    x, a = (torch.randn(2, 70, 12, generator=g).to(dev).requires_grad_(True) for _ in range(2))
    r = torch.randn(2, 12, 70, generator=g).to(dev).requires_grad_(True)
    gf, gt = torch.randn(2, 12, 70, generator=g).to(dev), torch.randn(2, 70, 12, generator=g).to(dev)
    f = ops.tokens_to_fields(x)
    f.backward(gf)
    assert torch.equal(f, x.detach().transpose(1, 2)) and torch.equal(x.grad, gf.transpose(1, 2))
    t = ops.fields_to_tokens(r, a)
    t.backward(gt)
    assert torch.equal(t, r.detach().transpose(1, 2) + a.detach())
    assert torch.equal(r.grad, gt.transpose(1, 2)) and torch.equal(a.grad, gt)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the block MLP's forward with a bias
# ---------------------------------------------------------------------------------------------------------------------
BD = [(1, 1, 2, 2), (129, 3, 6, 34), (70, 2, 130, 66)]       # (rows, nb, ib, ob)


@pytest.mark.parametrize("rows,nb,ib,ob", BD)
def test_bdmlp_fwd_bias(dev, rows, nb, ib, ob):
    """Per element against float64 with ``kc.X3_C``; one ``x3_slack_add`` term per fp32 addition of the epilogue, each from the
    float64 value that addition produces: the bias (``pre + bias``), and for act 3 the threshold (the soft-shrink's result).
    ``bias = NULL`` gives the bits of ``mk_spec_bdmlp_fwd``."""
    from makani_amd import _lib, ops
    lib = _lib.load()
    case, st = (rows, nb, ib, ob), ops._stream()
    g = _gen(23, *case)
    x, w, b = _crand(g, rows, nb, ib), _crand(g, nb, ib, ob), _crand(g, nb, ob)
    xd, wd, bd = (kc.poisoned(t, dev) for t in (x, w, b))
    x64, w64, b64 = (_c128(t) for t in (x, w, b))
    pre, mag = torch.einsum("rki,kio->rko", x64, w64) + b64, kc.absdot("rki,kio->rko", x64, w64)
    lam32 = float(torch.tensor(LAM, dtype=torch.float32))
    for act in (0, 2, 3):
        ref = {0: pre, 2: _relu_parts(pre, True, True), 3: torch.complex(_shrink(pre.real, lam32), _shrink(pre.imag, lam32))}[act]
        slack = kc.x3_slack_add(pre) + (kc.x3_slack_add(ref) if act == 3 else 0)
        y, check = kc.guarded((rows, nb, ob), torch.complex64, dev)
        _lib.check(lib.mk_spec_bdmlp_fwd_bias(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), *case, act, LAM, st),
                   "mk_spec_bdmlp_fwd_bias")
        _check(f"bdmlp fwd bias {case} act={act}", y, check, ref, mag, slack=slack)
        plain, check0 = kc.guarded((rows, nb, ob), torch.complex64, dev)
        _lib.check(lib.mk_spec_bdmlp_fwd(xd.data_ptr(), wd.data_ptr(), plain.data_ptr(), *case, act, LAM, st), "mk_spec_bdmlp_fwd")
        nobias, check1 = kc.guarded((rows, nb, ob), torch.complex64, dev)
        _lib.check(lib.mk_spec_bdmlp_fwd_bias(xd.data_ptr(), wd.data_ptr(), None, nobias.data_ptr(), *case, act, LAM, st),
                   "mk_spec_bdmlp_fwd_bias")
        torch.cuda.synchronize()
        check0("plain"), check1("null bias")
        assert torch.equal(torch.view_as_real(nobias), torch.view_as_real(plain)), f"act={act}: NULL bias differs from mk_spec_bdmlp_fwd"


# ---------------------------------------------------------------------------------------------------------------------
# 3. the latitude DFT on window tables
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlat,lmax,ncols,first", [(70, 33, 33, 20), (131, 130, 65, 100)])
def test_latdft_with_window_tables(dev, nlat, lmax, ncols, first):
    """As ``test_x3_guard_gpu.test_latdft`` holds the plain table: forward and inverse against the float64 matrix of the window's
    frequencies (the second case wraps past ``nlat``); the epilogue's sum of two accumulators is the slack."""
    from makani_amd import _lib, ops
    lib = _lib.load()
    W = window_matrix(nlat, lmax, first)
    tab = kc.poisoned(ops.latdft_table(nlat, lmax, first), dev)
    g = _gen(24, nlat, lmax, ncols)
    xf, cs = _crand(g, nlat, ncols), _crand(g, lmax, ncols)
    xfd, csd = kc.poisoned(xf, dev), kc.poisoned(cs, dev)
    ref64, mag = W @ _c128(xf), kc.absdot("lk,kj->lj", W, xf)
    c, check = kc.guarded((lmax, ncols), torch.complex64, dev)
    _lib.check(lib.mk_latdft_fwd(xfd.data_ptr(), tab.data_ptr(), c.data_ptr(), nlat, lmax, ncols, ops._stream()), "mk_latdft_fwd")
    _check(f"window latdft fwd {(nlat, lmax, ncols, first)}", c, check, ref64, mag, slack=kc.x3_slack_add(ref64))
    ref64, mag = W.conj().T @ _c128(cs), kc.absdot("lk,lj->kj", W, cs)
    x, check = kc.guarded((nlat, ncols), torch.complex64, dev)
    _lib.check(lib.mk_latdft_inv(csd.data_ptr(), tab.data_ptr(), x.data_ptr(), nlat, lmax, ncols, ops._stream()), "mk_latdft_inv")
    _check(f"window latdft inv {(nlat, lmax, ncols, first)}", x, check, ref64, mag, slack=kc.x3_slack_add(ref64))


# ---------------------------------------------------------------------------------------------------------------------
# 4. ops.spec_block_mlp with biases against the float64 chain
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,nb,L,M,f,seed", CHAIN_CASES)
def test_spec_block_mlp_with_biases_against_float64_chain(dev, B, C, nb, L, M, f, seed):
    from makani_amd import ops
    gen = torch.Generator().manual_seed(seed)
    bs = C // nb
    hb = bs * f

    def crand(*s):
        return torch.complex(torch.randn(*s, generator=gen), torch.randn(*s, generator=gen))

    c, g = crand(L, M, B * C), crand(L, M, B * C)
    params = [torch.randn(nb, bs, hb, 2, generator=gen) / bs ** 0.5, torch.randn(nb, hb, bs, 2, generator=gen) / hb ** 0.5,
              0.3 * torch.randn(nb * hb, 2, generator=gen), 0.3 * torch.randn(nb * bs, 2, generator=gen)]
    r = [c.to(torch.complex128).requires_grad_(True)] + [t.double().requires_grad_(True) for t in params]
    yo, m1, m2 = block_chain64(r[0].view(L, M, B, nb, bs), torch.view_as_complex(r[1]), torch.view_as_complex(r[3]).view(nb, hb),
                               torch.view_as_complex(r[2]), torch.view_as_complex(r[4]).view(nb, bs), LAM)
    print(f"[afnov1] chain {(B, C, nb, L, M)}: margins {m1:.1e} {m2:.1e}")
    assert min(m1, m2) > EDGE
    yo = yo.reshape(L, M, B * C)
    yo.backward(g.to(torch.complex128))
    runs = []
    for _ in range(2):
        leaves = [t.to(dev).requires_grad_(True) for t in [c] + params]
        y = ops.spec_block_mlp(leaves[0], leaves[1], leaves[2], B, nb, LAM, leaves[3], leaves[4])
        y.backward(g.to(dev))
        runs.append([y.detach()] + [t.grad for t in leaves])
    e = trel(torch.view_as_real(y).cpu(), torch.view_as_real(yo))
    print(f"[afnov1] chain y {e:.2e}")
    assert e < TOL
    for name, a, b in zip(("c", "w1", "w2", "b1", "b2"), leaves, r):
        ga, gb = (torch.view_as_real(t.grad) if t.grad.is_complex() else t.grad for t in (a, b))
        e = trel(ga.cpu(), gb)
        print(f"[afnov1] chain grad {name} {e:.2e}")
        assert ga.shape == gb.shape and e < GRAD_TOL, name
    for a, b in zip(*runs):
        assert torch.equal(torch.view_as_real(a) if a.is_complex() else a, torch.view_as_real(b) if b.is_complex() else b)


# ---------------------------------------------------------------------------------------------------------------------
# 5. AFNO2D on its fused path against the float64 window chain
# ---------------------------------------------------------------------------------------------------------------------
# (B, C, nb, H, W, fraction)
MODULE_CASES = [(2, 24, 3, 12, 16, 1.0), (2, 24, 3, 12, 16, 0.5), (2, 8, 2, 12, 6, 1.0), (2, 24, 2, 10, 12, 0.25)]


@pytest.mark.parametrize("B,C,nb,H,W,frac", MODULE_CASES)
def test_afno2d_fused_against_float64_chain(dev, monkeypatch, B, C, nb, H, W, frac):
    _hip(monkeypatch)
    mod = make_filter(C, nb, frac)
    x, g = torch.randn(B, H, W, C), torch.randn(B, H, W, C)
    yo, _, gxo, gpo, margins = window_chain64(mod, x, g)
    print(f"[afnov1] module {(B, C, nb, H, W, frac)}: margins {margins}")
    assert min(margins) > EDGE
    mod = mod.to(dev)
    calls = [_count_calls(monkeypatch, n) for n in ("spec_block_mlp", "tokens_to_fields", "fields_to_tokens")]
    xd = x.to(dev).requires_grad_(True)
    y = mod(xd)
    assert [len(c) for c in calls] == [1, 1, 1], "not a run of the fused path"
    y.backward(g.to(dev))
    errs = {"x.grad": trel(xd.grad.cpu(), gxo)}
    for n, p in mod.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, n
        errs[n] = trel(p.grad.cpu(), gpo[n])
    e = trel(y.cpu(), yo)
    print(f"[afnov1] module y {e:.2e}, " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert e < TOL
    worst = max(errs, key=errs.get)
    assert errs[worst] < GRAD_TOL, (worst, errs[worst])


def test_afno2d_bf16_input(dev, monkeypatch):
    """A bf16 field: the inverse FFT's fp32 rows are rounded to bf16 once (r) and ``r + x`` once more, so an entry is within half
    a bf16 ulp of r plus half an ulp of the result of the float64 chain on ``x.float()``: one ulp at the larger of the two (for
    entries below rms / 256 the ulp at rms / 256), as in ``tests/test_afno_gpu.py::test_afno2d_bf16_input``."""
    _hip(monkeypatch)
    B, C, nb, H, W = 2, 24, 3, 12, 16
    mod = make_filter(C, nb, seed=2)
    x = torch.randn(B, H, W, C).to(torch.bfloat16)
    yo, ro, _, _, margins = window_chain64(mod, x.float())
    assert min(margins) > EDGE
    mod = mod.to(dev)
    calls = _count_calls(monkeypatch, "spec_block_mlp")
    with torch.no_grad():
        y = mod(x.to(dev))
    assert len(calls) == 1 and y.dtype == torch.bfloat16
    y = y.cpu().double()
    rms = yo.square().mean().sqrt()
    tol = kc.bf16_ulp(torch.maximum(torch.maximum(y.abs(), yo.abs()), torch.maximum(ro.abs(), rms / 256)))
    worst = ((y - yo).abs() / tol).max().item()
    print(f"[afnov1] bf16 input: worst difference {worst:.2f} ulp")
    assert worst <= 1.0


@pytest.mark.parametrize("C,nb,H,W,frac", [(18, 2, 12, 16, 1.0), (24, 3, 12, 15, 1.0), (24, 3, 6, 8, 0.2)],
                         ids=["odd-block", "odd-width", "empty-window"])
def test_afno2d_cases_the_kernels_do_not_take(dev, monkeypatch, C, nb, H, W, frac):
    _hip(monkeypatch)
    mod = make_filter(C, nb, frac).to(dev)
    calls = [_count_calls(monkeypatch, n) for n in ("spec_block_mlp", "tokens_to_fields", "fields_to_tokens")]
    x = torch.randn(2, H, W, C, device=dev)
    with torch.no_grad():
        assert torch.equal(mod(x), mod._forward_torch(x)) and not any(calls)


def test_fused_equals_torch_path(dev, monkeypatch):
    B, C, nb, H, W = 2, 24, 3, 12, 16
    mod = make_filter(C, nb, 0.5)
    x, g = torch.randn(B, H, W, C), torch.randn(B, H, W, C)
    assert min(window_chain64(mod, x)[4]) > EDGE
    mod = mod.to(dev)
    calls = _count_calls(monkeypatch, "spec_block_mlp")
    res = {}
    for knob in ("hip", "torch"):
        monkeypatch.setenv("MK_PLANAR_FFT", "hip")
        monkeypatch.setenv("MK_AFNOV1", knob)
        del calls[:]
        mod.zero_grad(set_to_none=True)
        xd = x.to(dev).requires_grad_(True)
        y = mod(xd)
        assert len(calls) == (1 if knob == "hip" else 0)
        y.backward(g.to(dev))
        res[knob] = [y.detach(), xd.grad] + [p.grad.clone() for p in mod.parameters()]
    errs = [trel(a, b) for a, b in zip(res["hip"], res["torch"])]
    print("[afnov1] fused vs torch: " + ", ".join(f"{e:.2e}" for e in errs))
    assert max(errs) < TOL


# ---------------------------------------------------------------------------------------------------------------------
# 6. the tiny net on the device
# ---------------------------------------------------------------------------------------------------------------------
def test_net_on_the_device_against_the_reference_run(dev, monkeypatch, ref):  # noqa: F811
    _hip(monkeypatch)
    net = build(ref, "net").to(dev)
    calls = _count_calls(monkeypatch, "spec_block_mlp")
    check_against_fixture(ref, "net", net, dev, TOL, GRAD_TOL, "device fp32")
    assert len(calls) == 2, "one fused filter per block"


@pytest.mark.parametrize("token_kernels", [False, True], ids=["torch-norm-linear", "hip-norm-linear"])
def test_net_under_bf16_autocast(dev, monkeypatch, ref, token_kernels):  # noqa: F811
    """The bound of ``tests/test_model_gpu.py::test_sfno_bf16_autocast_runs_and_is_close``: 3e-2 on the output, every parameter
    with a finite gradient.  With ``MK_TOKEN_NORM=hip MK_TOKEN_LINEAR=hip`` a block's graph holds the package's nodes -- two token
    layer norms, one token MLP -- and neither ``F.layer_norm`` nor a vendor GEMM for its linears (the nodes' names say so)."""
    _hip(monkeypatch)
    if token_kernels:
        monkeypatch.setenv("MK_TOKEN_NORM", "hip")
        monkeypatch.setenv("MK_TOKEN_LINEAR", "hip")
    net = build(ref, "net").to(dev)
    calls = _count_calls(monkeypatch, "spec_block_mlp")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = net(ref["net.x"].to(dev))
    assert len(calls) == 2
    y.float().backward(ref["net.g"].to(dev))
    e = trel(y.float().cpu(), ref["net.y"])
    print(f"[afnov1] net bf16 autocast (token kernels {token_kernels}): y {e:.2e}")
    assert e < 3e-2
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())
    if token_kernels:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            kinds = _graph_kinds(net.blocks[0](torch.randn(2, 6, 10, 16, device=dev, requires_grad=True)))
        assert sum(k.startswith("_TokenLayerNorm") for k in kinds) == 2 and sum(k.startswith("_TokenMLP") for k in kinds) == 1, kinds
        assert not any("LayerNorm" in k and not k.startswith("_TokenLayerNorm") for k in kinds), kinds
        assert not any("Addmm" in k or "MmBackward" in k for k in kinds), kinds


# ---------------------------------------------------------------------------------------------------------------------
# 7. a captured step
# ---------------------------------------------------------------------------------------------------------------------
def test_net_step_captured_and_replayed(dev, monkeypatch, ref):  # noqa: F811
    """Forward + backward of the tiny net captured in a HIP graph (the sequence of ``tests/test_afno_gpu.py``); the replay gives the
    bits of the eager step for the output and for every parameter gradient: the filter, the layout passes, the bias gradients
    (float64, fixed order) and the torch linears of the fp32 path have no atomics in them."""
    _hip(monkeypatch)
    net = build(ref, "net").to(dev)
    x, g = ref["net.x"].to(dev), ref["net.g"].to(dev)
    static_inp = x.clone()
    calls = _count_calls(monkeypatch, "spec_block_mlp")
    capture_stream = torch.cuda.Stream()
    capture_stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(capture_stream):
        for _ in range(3):
            net.zero_grad(set_to_none=True)
            y = net(static_inp)
            y.backward(g)
        capture_stream.synchronize()
        assert len(calls) == 3 * 2
        eager_y = y.detach().clone()
        eager = {n: p.grad.clone() for n, p in net.named_parameters()}
        gc.collect()
        torch.cuda.empty_cache()
        graph = torch.cuda.CUDAGraph()
        net.zero_grad(set_to_none=True)
        graph.capture_begin()
        static_y = net(static_inp)
        static_y.backward(g)
        graph.capture_end()
    torch.cuda.current_stream().wait_stream(capture_stream)
    static_inp.copy_(x)
    graph.replay()
    torch.cuda.synchronize()
    differ = [n for n, p in net.named_parameters() if not torch.equal(p.grad, eager[n])]
    print(f"[afnov1] replay: {len(eager)} gradients; not bit-equal to the eager step: {differ}")
    assert torch.equal(static_y, eager_y)
    filt = {f"blocks.{i}.filter.{w}" for i in (0, 1) for w in ("w1", "b1", "w2", "b2")}
    front = {"pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias", "blocks.0.norm1.weight", "blocks.0.norm1.bias"}
    assert filt | front <= set(eager) and not (filt | front) & set(differ), differ
    for n in differ:        # anything else (vendor GEMMs of the linears' weight gradients) is held to the eager step at 1e-5
        assert trel(net.get_parameter(n).grad, eager[n]) < 1e-5, n
