"""AFNO on the ``mk_spec_bdmlp_*`` kernels: each kernel alone through the raw wrappers against float64 block einsums,
``ops.spec_block_mlp`` and ``AFNO2D`` on its fused path against the float64 chain written out here, fused against the torch
path, the recorded reference run of the tiny net on the device (fp32 and bf16 autocast), and a captured step.

Criterion: relative L2 error <= 1e-5 forward and <= 5e-5 for module gradients against float64 (the project's fp32 criterion;
the reference's own fp32 run sits at 2-3e-7 / <= 2.4e-7 on these shapes).  ReLU and soft-shrink masks are discontinuous, so every
float64 reference asserts that no masked argument lies within 1e-5 rms of its edge (seeds checked on the CPU): otherwise a
flipped mask entry, not an error, would decide the comparison."""
import gc
import os

import numpy as np
import pytest
import torch

from kernel_checks import bf16_ulp as _bf16_ulp
from test_afno_cpu import NET_KW, build, check_against_fixture, ref, rel as trel  # noqa: F401  (ref: the fixture)

pytestmark = pytest.mark.gpu

TOL, GRAD_TOL, EDGE = 1e-5, 5e-5, 1e-5
LAM = 0.5


def nrel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def comps(z):
    return np.stack([z.real, z.imag])


def margin(z, edge=0.0):
    """Smallest distance of a component of ``z`` from +-``edge`` in units of the components' rms."""
    v = comps(np.asarray(z))
    return float(np.abs(np.abs(v) - edge).min() / np.sqrt(np.mean(v * v)))


def relu_c(z):
    return np.maximum(z.real, 0) + 1j * np.maximum(z.imag, 0)


def shrink_c(z, lam):
    def f(v):
        return np.where(v > lam, v - lam, np.where(v < -lam, v + lam, 0.0))
    return f(z.real) + 1j * f(z.imag)


def pass_c(g, mask):
    """``g`` where the same component of ``mask`` holds, else 0."""
    return np.where(mask.real, g.real, 0) + 1j * np.where(mask.imag, g.imag, 0)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernels alone
# ---------------------------------------------------------------------------------------------------------------------
# (L, M, B, nb, ib, ob):  216 rows = two row tiles with a ragged edge, and a k-step (32 floats) that would run into the next
# block's channels (ib = 6: 12 floats);  > 1 k-step (ragged) and > 1 column tile (ragged);  fewer rows than a tile;  one block,
# also against the dense kernel;  odd block size: the refusal
KERNEL_CASES = [(12, 9, 2, 3, 6, 10), (12, 9, 2, 2, 34, 66), (5, 4, 1, 4, 4, 4), (16, 9, 1, 1, 8, 16), (4, 4, 1, 2, 3, 4)]


def kernel_reference(L, M, B, nb, ib, ob):
    """Operands (complex64) and the float64 results of one kernel case."""
    rng = np.random.default_rng(17)

    def crand(*s):
        return (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(np.complex64)

    R = L * M * B
    o = dict(x=crand(R, nb, ib), gy=crand(R, nb, ob), a=crand(R, nb, ib), w=(crand(nb, ib, ob) / np.sqrt(ib)).astype(np.complex64))
    o["s"] = shrink_c(crand(R, nb, ob), 0.7).astype(np.complex64)       # a saved soft-shrink output: exact zeros where it cut
    x, gy, w = (o[k].astype(np.complex128) for k in ("x", "gy", "w"))
    o["pre"] = np.einsum("rki,kio->rko", x, w)
    smask = (o["s"].real != 0) + 1j * (o["s"].imag != 0)
    amask = (o["a"].real > 0) + 1j * (o["a"].imag > 0)
    for tag, g in (("", gy), ("_s", pass_c(gy, smask))):
        full = np.einsum("rko,kio->rki", g, np.conj(w))
        o["gx" + tag], o["gx_a" + tag] = full, pass_c(full, amask)
        o["gw" + tag] = np.einsum("rki,rko->kio", np.conj(x), g)
    # (the masks of the data gradient are read off operands, exactly: only the forward's own arguments have an edge to keep off)
    o["margins"] = (margin(o["pre"]), margin(o["pre"], LAM))
    return o


@pytest.mark.parametrize("L,M,B,nb,ib,ob", KERNEL_CASES)
def test_kernels_alone(dev, L, M, B, nb, ib, ob):
    """Forward with act 0 / 2 / 3, data gradient with and without each mask, weight gradient with and without ``s`` and with
    equal bits on two runs.  Odd block sizes are the launcher's refusal."""
    from makani_amd import ops
    o = kernel_reference(L, M, B, nb, ib, ob)

    def field(t):       # [R, nb, c] -> the private layout [L, M, B * nb * c]
        return torch.from_numpy(t.reshape(L, M, -1)).to(dev)

    x, gy, a, s, w = field(o["x"]), field(o["gy"]), field(o["a"]), field(o["s"]), torch.from_numpy(o["w"]).to(dev)
    if ib % 2 or ob % 2:
        for call in (lambda: ops.spec_bdmlp_fwd_raw(x, w, 0), lambda: ops.spec_bdmlp_dgrad_raw(gy, w),
                     lambda: ops.spec_bdmlp_wgrad_raw(x, gy, B, nb)):
            with pytest.raises(RuntimeError, match="even block sizes"):
                call()
        return
    print(f"[afno] case {(L, M, B, nb, ib, ob)}: margins {o['margins']}")
    assert min(o["margins"]) > EDGE, "another seed: a masked argument of the float64 reference sits on an edge"

    def got(t, c):
        return t.cpu().numpy().reshape(-1, nb, c)

    for act, want in ((0, o["pre"]), (2, relu_c(o["pre"])), (3, shrink_c(o["pre"], LAM))):
        y = ops.spec_bdmlp_fwd_raw(x, w, act, LAM)
        assert tuple(y.shape) == (L, M, B * nb * ob)
        e = nrel(got(y, ob), want)
        print(f"[afno] fwd act={act}: {e:.2e}")
        assert e < TOL
    if nb == 1:     # the same panel through the dense channel-MLP kernel (degree offset M: no triangle)
        dense = ops.spec_cmlp_fwd_raw(x, w[0].contiguous(), None, B, 0, M, 0)
        assert trel(torch.view_as_real(ops.spec_bdmlp_fwd_raw(x, w, 0)), torch.view_as_real(dense)) < TOL
    for am, sm in ((None, None), (a, None), (None, s), (a, s)):
        gx = ops.spec_bdmlp_dgrad_raw(gy, w, a=am, s=sm)
        key = "gx" + ("_a" if am is not None else "") + ("_s" if sm is not None else "")
        e = nrel(got(gx, ib), o[key])
        print(f"[afno] dgrad {key}: {e:.2e}")
        assert tuple(gx.shape) == (L, M, B * nb * ib) and e < TOL
    for sm, key in ((None, "gw"), (s, "gw_s")):
        gw = ops.spec_bdmlp_wgrad_raw(x, gy, B, nb, s=sm)
        e = nrel(gw.cpu().numpy(), o[key])
        print(f"[afno] wgrad {key}: {e:.2e}")
        assert tuple(gw.shape) == (nb, ib, ob) and e < TOL
        assert torch.equal(gw, ops.spec_bdmlp_wgrad_raw(x, gy, B, nb, s=sm))


# ---------------------------------------------------------------------------------------------------------------------
# 2. / 3. the chain and the module against float64
# ---------------------------------------------------------------------------------------------------------------------
def block_chain64(c, w1, w2, lam):
    """float64 torch: ``c`` complex128 [..., nb, bs] (any leading axes) -> (y [..., nb, bs], margin of the ReLU arguments, of the
    soft-shrink arguments)."""
    p1 = torch.einsum("...ki,kio->...ko", c, torch.view_as_complex(w1))
    h = torch.complex(torch.relu(p1.real), torch.relu(p1.imag))
    p2 = torch.view_as_real(torch.einsum("...ki,kio->...ko", h, torch.view_as_complex(w2)))
    y = torch.where(p2 > lam, p2 - lam, torch.where(p2 < -lam, p2 + lam, torch.zeros_like(p2)))
    m1 = margin(p1.detach().numpy())
    m2 = float((p2.detach().abs() - lam).abs().min() / p2.detach().square().mean().sqrt())
    return torch.view_as_complex(y), m1, m2


# (B, C, nb, L, M, hidden factor, seed); the second has block size 68: more than 64 complex columns
CHAIN_CASES = [(2, 24, 3, 12, 16, 1, 0), (1, 136, 2, 6, 8, 1, 0)]


@pytest.mark.parametrize("B,C,nb,L,M,f,seed", CHAIN_CASES)
def test_spec_block_mlp_against_float64_chain(dev, B, C, nb, L, M, f, seed):
    from makani_amd import ops
    gen = torch.Generator().manual_seed(seed)
    bs = C // nb

    def crand(*s):
        return torch.complex(torch.randn(*s, generator=gen), torch.randn(*s, generator=gen))

    c, g = crand(L, M, B * C), crand(L, M, B * C)
    w1 = torch.randn(nb, bs, bs * f, 2, generator=gen) / bs ** 0.5
    w2 = torch.randn(nb, bs * f, bs, 2, generator=gen) / (bs * f) ** 0.5
    r = [c.to(torch.complex128).requires_grad_(True), w1.double().requires_grad_(True), w2.double().requires_grad_(True)]
    yo, m1, m2 = block_chain64(r[0].view(L, M, B, nb, bs), r[1], r[2], LAM)
    print(f"[afno] chain {(B, C, nb, L, M)}: margins {m1:.1e} {m2:.1e}")
    assert min(m1, m2) > EDGE
    yo = yo.reshape(L, M, B * C)
    yo.backward(g.to(torch.complex128))
    leaves = [t.to(dev).requires_grad_(True) for t in (c, w1, w2)]
    y = ops.spec_block_mlp(leaves[0], leaves[1], leaves[2], B, nb, LAM)
    y.backward(g.to(dev))
    e = trel(torch.view_as_real(y).cpu(), torch.view_as_real(yo))
    print(f"[afno] chain y {e:.2e}")
    assert e < TOL
    for name, a, b in zip(("c", "w1", "w2"), leaves, r):
        ga, gb = (torch.view_as_real(t.grad) if t.grad.is_complex() else t.grad for t in (a, b))
        e = trel(ga.cpu(), gb)
        print(f"[afno] chain grad {name} {e:.2e}")
        assert ga.shape == gb.shape and a.grad.stride() == a.stride() and e < TOL, name


def afno_chain64(mod, x, g=None):
    """``AFNO2D`` in float64 torch from the module's parameters: (y, filter term alone, x.grad, parameter gradients, margins)."""
    p = {n: t.detach().cpu().double().requires_grad_(True) for n, t in mod.named_parameters()}
    xo = x.detach().cpu().double().requires_grad_(True)
    B, C, H, W = xo.shape
    nb, bs = mod.num_blocks, mod.block_size
    th, tw = H // 2 + 1, W // 2 + 1
    kh, kw = int(th * mod.hard_thresholding_fraction), int(tw * mod.hard_thresholding_fraction)
    c = torch.fft.rfft2(xo, dim=(-2, -1), norm="ortho").view(B, nb, bs, H, tw)[..., :kw]
    if kh != th:
        c = torch.cat([c[:, :, :, :kh], c[:, :, :, -kh:]], dim=3)
    y, m1, m2 = block_chain64(c.permute(0, 3, 4, 1, 2), p["w1"], p["w2"], mod.sparsity_threshold)
    y = y.permute(0, 3, 4, 1, 2)        # [B, nb, bs, rows, kw]
    if kh != th:
        y = torch.cat([y[:, :, :, :kh], torch.zeros(B, nb, bs, H - 2 * kh, kw, dtype=y.dtype), y[:, :, :, kh:]], dim=3)
    y = torch.nn.functional.pad(torch.view_as_real(y), (0, 0, 0, tw - kw))
    r = torch.fft.irfft2(torch.view_as_complex(y).reshape(B, C, H, tw), s=(H, W), dim=(-2, -1), norm="ortho")
    out = r + p["b1"] + xo
    grads = None
    if g is not None:
        out.backward(g.double())
        grads = {n: t.grad for n, t in p.items()}
    return out.detach(), r.detach(), xo.grad, grads, (m1, m2)


def _filter(C, nb, frac=1.0, f=1, seed=0):
    from makani_amd.afnonet import AFNO2D
    torch.manual_seed(seed)
    mod = AFNO2D(C, num_blocks=nb, sparsity_threshold=LAM, hard_thresholding_fraction=frac, hidden_size_factor=f)
    with torch.no_grad():       # the init's 0.02 against the threshold would cut every coefficient (see make_afno_golden.py)
        mod.w1.copy_(torch.randn_like(mod.w1) * 0.8 / mod.block_size ** 0.5)
        mod.w2.copy_(torch.randn_like(mod.w2) * 0.8 / (mod.block_size * f) ** 0.5 * 2.0)
    return mod


def _count_calls(monkeypatch, name):
    from makani_amd import ops
    calls, real = [], getattr(ops, name)
    monkeypatch.setattr(ops, name, lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def _hip(monkeypatch):
    monkeypatch.setenv("MK_AFNO", "hip")
    monkeypatch.setenv("MK_PLANAR_FFT", "hip")


# (B, C, nb, H, W, fraction, hidden factor, seed)
MODULE_CASES = [(2, 24, 3, 12, 16, 1.0, 1, 0), (2, 24, 3, 12, 16, 0.5, 1, 0), (2, 24, 2, 10, 12, 1.0, 2, 0)]


@pytest.mark.parametrize("B,C,nb,H,W,frac,f,seed", MODULE_CASES)
def test_afno2d_fused_against_float64_chain(dev, monkeypatch, B, C, nb, H, W, frac, f, seed):
    _hip(monkeypatch)
    mod = _filter(C, nb, frac, f, seed)
    x, g = torch.randn(B, C, H, W), torch.randn(B, C, H, W)
    yo, _, gxo, gpo, margins = afno_chain64(mod, x, g)
    print(f"[afno] module {(B, C, nb, H, W, frac, f)}: margins {margins}")
    assert min(margins) > EDGE
    mod = mod.to(dev)
    calls = _count_calls(monkeypatch, "spec_block_mlp")
    xd = x.to(dev).requires_grad_(True)
    y = mod(xd)
    assert len(calls) == 1, "not a run of the fused path"
    y.backward(g.to(dev))
    errs = {"x.grad": trel(xd.grad.cpu(), gxo)}
    for n, p in mod.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, n
        errs[n] = trel(p.grad.cpu(), gpo[n])
    e = trel(y.cpu(), yo)
    print(f"[afno] module y {e:.2e}, " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert e < TOL
    worst = max(errs, key=errs.get)
    assert errs[worst] < GRAD_TOL, (worst, errs[worst])




def test_afno2d_bf16_input(dev, monkeypatch):
    """A bf16 field: the inverse FFT's fp32 rows are rounded to bf16 once (r) and ``r + b1 + x`` once more, so an entry is
    within half a bf16 ulp of r plus half an ulp of the result of the float64 chain on ``x.float()``: one ulp at the larger of
    the two (for entries below rms / 256 the ulp at rms / 256, as in ``tests/test_specattn_gpu.py``)."""
    _hip(monkeypatch)
    B, C, nb, H, W = 2, 24, 3, 12, 16
    mod = _filter(C, nb, seed=2)
    x = torch.randn(B, C, H, W).to(torch.bfloat16)
    yo, ro, _, _, margins = afno_chain64(mod, x.float())
    assert min(margins) > EDGE
    mod = mod.to(dev)
    calls = _count_calls(monkeypatch, "spec_block_mlp")
    with torch.no_grad():
        y = mod(x.to(dev))
    assert len(calls) == 1 and y.dtype == torch.bfloat16
    y = y.cpu().double()
    rms = yo.square().mean().sqrt()
    tol = _bf16_ulp(torch.maximum(torch.maximum(y.abs(), yo.abs()), torch.maximum(ro.abs(), rms / 256)))
    worst = ((y - yo).abs() / tol).max().item()
    print(f"[afno] bf16 input: worst difference {worst:.2f} ulp")
    assert worst <= 1.0


@pytest.mark.parametrize("C,nb,H,W", [(18, 2, 12, 16), (24, 3, 12, 15)], ids=["odd-block", "odd-width"])
def test_afno2d_cases_the_kernels_do_not_take(dev, monkeypatch, C, nb, H, W):
    _hip(monkeypatch)
    mod = _filter(C, nb).to(dev)
    calls = _count_calls(monkeypatch, "spec_block_mlp")
    x = torch.randn(2, C, H, W, device=dev)
    with torch.no_grad():
        assert torch.equal(mod(x), mod._forward_torch(x)) and not calls


# ---------------------------------------------------------------------------------------------------------------------
# 4. fused against the torch path
# ---------------------------------------------------------------------------------------------------------------------
def test_fused_equals_torch_path(dev, monkeypatch):
    B, C, nb, H, W = 2, 24, 3, 12, 16
    mod = _filter(C, nb, 0.5)
    x, g = torch.randn(B, C, H, W), torch.randn(B, C, H, W)
    assert min(afno_chain64(mod, x)[4]) > EDGE
    mod = mod.to(dev)
    calls = _count_calls(monkeypatch, "spec_block_mlp")
    res = {}
    for knob in ("hip", "torch"):
        monkeypatch.setenv("MK_PLANAR_FFT", "hip")
        monkeypatch.setenv("MK_AFNO", knob)
        del calls[:]
        mod.zero_grad(set_to_none=True)
        xd = x.to(dev).requires_grad_(True)
        y = mod(xd)
        assert len(calls) == (1 if knob == "hip" else 0)
        y.backward(g.to(dev))
        res[knob] = [y.detach(), xd.grad] + [p.grad.clone() for p in mod.parameters()]
    errs = [trel(a, b) for a, b in zip(res["hip"], res["torch"])]
    print("[afno] fused vs torch: " + ", ".join(f"{e:.2e}" for e in errs))
    assert max(errs) < TOL


# ---------------------------------------------------------------------------------------------------------------------
# 5. the recorded reference run of the tiny net
# ---------------------------------------------------------------------------------------------------------------------
def test_net_on_the_device_against_the_reference_run(dev, monkeypatch, ref):  # noqa: F811
    _hip(monkeypatch)
    net = build(ref, "net").to(dev)
    calls = _count_calls(monkeypatch, "spec_block_mlp")
    check_against_fixture(ref, "net", net, dev, TOL, GRAD_TOL, "device fp32")
    assert len(calls) == 2, "one fused filter per block"


def test_net_under_bf16_autocast(dev, monkeypatch, ref):  # noqa: F811
    """The bound of ``tests/test_model_gpu.py::test_sfno_bf16_autocast_runs_and_is_close``: 3e-2 on the output, every parameter
    with a finite gradient."""
    _hip(monkeypatch)
    net = build(ref, "net").to(dev)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = net(ref["net.x"].to(dev))
    y.float().backward(ref["net.g"].to(dev))
    e = trel(y.float().cpu(), ref["net.y"])
    print(f"[afno] net bf16 autocast: y {e:.2e}")
    assert e < 3e-2
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())


# ---------------------------------------------------------------------------------------------------------------------
# 6. a captured step
# ---------------------------------------------------------------------------------------------------------------------
def test_net_step_captured_and_replayed(dev, monkeypatch, ref):  # noqa: F811
    """Forward + backward of the tiny net captured in a HIP graph (the sequence of ``tests/test_specattn_gpu.py``); the replay
    gives the bits of the eager step: the output (the whole forward) and every parameter gradient but the weights of the fp32
    1x1 convolutions (skip, MLP, head), whose gradient kernel adds its pixel slabs with fp32 atomics (DESIGN 2.6:
    ``conv_x3_kernel`` MODE 2) and so gives other last bits from one eager run to the next too, whatever the blocks hold; those
    are held to 1e-5 of the eager step, as in ``tests/test_specattn_gpu.py::test_net_step_captured_and_replayed``.
    Everything the filter computes -- ``w1`` / ``w2`` / ``b1`` and the data gradient every parameter in front of it receives
    (norms, biases, position and patch embedding) -- is in the bit-equal set."""
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
    from makani_amd.layers import Conv1x1
    atomic = {f"{mn}.weight" for mn, m in net.named_modules() if isinstance(m, Conv1x1)}
    names = {n for n, _ in net.named_parameters()}
    differ = [n for n, p in net.named_parameters() if not torch.equal(p.grad, eager[n])]
    print(f"[afno] replay: {len(names)} gradients, {len(atomic)} of them atomic sums; not bit-equal to the eager step: {differ}")
    assert torch.equal(static_y, eager_y)
    assert atomic < names and all(f"blocks.{i}.filter.{w}" in names - atomic for i in (0, 1) for w in ("w1", "b1", "w2"))
    assert set(differ) <= atomic, differ
    for n in differ:
        assert trel(net.get_parameter(n).grad, eager[n]) < 1e-5, n
