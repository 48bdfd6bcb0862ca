"""Patch rows on the MI355X: ``mk_patchify`` / ``mk_unpatchify`` through the C ABI bit for bit against the torch formulation
(a permutation and at most one rounding: no tolerance), ``ops.patch_embed`` against float64 on the bf16-rounded operands under
the derived bounds of ``toklinear_checks``, the dispatch, both recorded networks and one captured training step."""
import gc

import pytest
import torch

import kernel_checks as kc
import test_afnov1_cpu as av1
import test_vit_cpu as vit
import toklinear_checks as tc
from test_afnov1_cpu import ref as afnov1_ref      # noqa: F401  (module-scoped fixtures)
from test_vit_cpu import ref as vit_ref            # noqa: F401

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
CODE = {F32: 0, BF16: 1}
CASES = [(1, 1, 7, 8, 7, 8), (2, 3, 14, 24, 7, 8), (1, 5, 6, 10, 3, 5), (2, 8, 16, 32, 8, 8), (1, 73, 14, 16, 7, 8), (1, 2, 9, 260, 3, 4)]
# geometries that leave a single tile in every direction (tests/test_patch_cpu.py asserts from ``mk_patch_tile_info`` that they do):
# three tiles across with a ragged last one, five channel chunks (order 0) and seven patch-row parts (order 1), the cuts of
# ``vit_73ch``; two patch-row parts, 5 rows and a ragged 3, the cut of AFNOv1 at 26 channels; a patch wider than 1024 columns, cut
# along j, ragged; the same with nothing vectorisable; channels beyond the tile in order 1, a multiple of 8 and not
CUT_CASES = [(1, 73, 14, 160, 7, 8), (1, 26, 16, 168, 8, 8), (1, 1, 1, 2600, 1, 1300), (1, 2, 2, 2082, 2, 1041), (1, 160, 2, 136, 1, 8),
             (1, 150, 1, 136, 1, 8)]
EMBED = [(2, 3, 14, 24, 7, 8, 16), (1, 73, 14, 16, 7, 8, 384), (1, 2, 63, 136, 7, 8, 16), (3, 4, 16, 64, 8, 8, 24)]


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def stream():
    return torch.cuda.current_stream().cuda_stream


def c_patchify(lib, img, tok, ldt, geom, order):
    B, C, H, W, p0, p1 = geom
    rc = lib.mk_patchify(img.data_ptr(), CODE[img.dtype], tok.data_ptr(), CODE[tok.dtype], ldt, B, C, H, W, p0, p1, order, stream())
    assert rc == 0, lib.mk_last_error().decode()


def c_unpatchify(lib, tok, ldt, img, geom, order):
    B, C, H, W, p0, p1 = geom
    rc = lib.mk_unpatchify(tok.data_ptr(), CODE[tok.dtype], ldt, img.data_ptr(), CODE[img.dtype], B, C, H, W, p0, p1, order, stream())
    assert rc == 0, lib.mk_last_error().decode()


def sentinel_like(t):
    return torch.full_like(t, kc.SENTINEL)


@pytest.mark.parametrize("geom", CASES + CUT_CASES)
def test_kernels_are_the_permutation_bit_for_bit(dev, geom):
    from makani_amd import _lib, ops
    lib = _lib.load()
    B, C, H, W, p0, p1 = geom
    R, F = B * (H // p0) * (W // p1), C * p0 * p1
    gen = torch.Generator().manual_seed(sum(geom))
    x32 = torch.randn(B, C, H, W, generator=gen)
    t32 = torch.randn(R, F, generator=gen)
    for order in (0, 1):
        for src_dt in (F32, BF16):
            x, t = x32.to(src_dt), t32.to(src_dt)
            xd = kc.poisoned(x, dev)
            for dst_dt in (F32, BF16):
                want_rows = ops._patchify_torch(x, (p0, p1), order).to(dst_dt).reshape(R, F)
                want_img = ops._unpatchify_torch(t, (p0, p1), C, H, W, order).to(dst_dt)
                for ldt in (F, F + 8):
                    what = f"{geom} order {order} {src_dt} -> {dst_dt} ldt {ldt}"
                    out, check = kc.guarded((R, ldt), dst_dt, dev)
                    c_patchify(lib, xd, out, ldt, geom, order)
                    torch.cuda.synchronize()
                    check("patchify " + what)
                    assert same_bits(out[:, :F].cpu(), want_rows), "patchify " + what
                    assert same_bits(out[:, F:].cpu(), sentinel_like(out[:, F:]).cpu()), "patchify wrote the gap columns: " + what
                    # the way back, from rows whose gap columns are NaN
                    padded = torch.full((R, ldt), float("nan"), dtype=src_dt)
                    padded[:, :F] = t
                    td = kc.poisoned(padded, dev)
                    img, check = kc.guarded((B, C, H, W), dst_dt, dev)
                    c_unpatchify(lib, td, ldt, img, geom, order)
                    torch.cuda.synchronize()
                    check("unpatchify " + what)
                    assert same_bits(img.cpu(), want_img), "unpatchify " + what
                    # and the round trip of the rows patchify wrote
                    if src_dt == dst_dt:
                        back, check = kc.guarded((B, C, H, W), src_dt, dev)
                        c_unpatchify(lib, out, ldt, back, geom, order)
                        torch.cuda.synchronize()
                        check("round trip " + what)
                        assert same_bits(back.cpu(), x), "round trip " + what


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_bases_one_element_off_take_single_elements(dev, order, dtype):
    from makani_amd import _lib, ops
    lib = _lib.load()
    geom = B, C, H, W, p0, p1 = (2, 8, 16, 32, 8, 8)
    R, F = B * (H // p0) * (W // p1), C * p0 * p1
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(B, C, H, W, generator=gen).to(dtype)
    src = kc.poisoned(torch.cat([torch.full((1,), float("nan"), dtype=dtype), x.flatten()]), dev)[1:]
    flat, check = kc.guarded((R * F + 1,), dtype, dev)
    assert src.data_ptr() % 16 != 0 and flat[1:].data_ptr() % 16 != 0
    c_patchify(lib, src, flat[1:], F, geom, order)
    torch.cuda.synchronize()
    check("patchify")
    assert float(flat[0]) == kc.SENTINEL
    assert same_bits(flat[1:].cpu().view(R, F), ops._patchify_torch(x, (p0, p1), order).reshape(R, F))
    back, check = kc.guarded((x.numel() + 1,), dtype, dev)
    c_unpatchify(lib, flat[1:], F, back[1:], geom, order)
    torch.cuda.synchronize()
    check("unpatchify")
    assert float(back[0]) == kc.SENTINEL
    assert same_bits(back[1:].cpu().view(x.shape), x)


def test_ops_layout_functions_and_their_gradients(dev, monkeypatch):
    """``ops.patchify`` / ``ops.unpatchify`` on the device: the kernels, the cast in the same pass, each one's backward the other."""
    from makani_amd import ops
    monkeypatch.setenv("MK_PATCH", "hip")
    calls = Calls(monkeypatch)
    B, C, H, W, p0, p1 = 2, 3, 14, 24, 7, 8
    gen = torch.Generator().manual_seed(12)
    for order in (0, 1):
        x = torch.randn(B, C, H, W, generator=gen).to(dev).requires_grad_()
        rows = ops.patchify(x, (p0, p1), order, dtype=BF16)
        assert same_bits(rows.detach().cpu(), ops._patchify_torch(x.detach().cpu(), (p0, p1), order).to(BF16))
        g = torch.randn(rows.shape, generator=gen).to(dev).bfloat16()
        (gx,) = torch.autograd.grad(rows, [x], g)
        assert same_bits(gx.cpu(), ops._unpatchify_torch(g.cpu(), (p0, p1), C, H, W, order).float())
        t = torch.randn(B, H // p0, W // p1, C * p0 * p1, generator=gen).to(dev).bfloat16().requires_grad_()
        img = ops.unpatchify(t, (p0, p1), C, (H, W), order)
        assert same_bits(img.detach().cpu(), ops._unpatchify_torch(t.detach().cpu(), (p0, p1), C, H, W, order))
        gi = torch.randn(img.shape, generator=gen).to(dev)                  # an fp32 gradient, as the loss hands it back
        (gt,) = torch.autograd.grad(img, [t], gi)
        assert gt.shape == t.shape and same_bits(gt.cpu().reshape(B, -1, C * p0 * p1), ops._patchify_torch(gi.cpu(), (p0, p1), order).to(BF16))
    assert (calls.patchify, calls.unpatchify) == (4, 4)
    for bad in (t[..., :-8], t.reshape(-1)[: t.numel() // 2].reshape(-1, C * p0 * p1)[:5]):
        with pytest.raises(ValueError):
            ops.unpatchify(bad, (p0, p1), C, (H, W), 1)                 # as the torch formulation refuses them
    monkeypatch.setenv("MK_PATCH", "torch")
    ops.unpatchify(ops.patchify(x, (p0, p1), 1), (p0, p1), C, (H, W), 1)
    assert (calls.patchify, calls.unpatchify) == (4, 4)


class Calls:
    """Counts the launches of the raw entry points and the uses of the embedding node."""

    def __init__(self, monkeypatch):
        from makani_amd import ops
        self.patchify = self.unpatchify = self.embed = self.gemm = self.wgrad = 0
        orig = {n: getattr(ops, n) for n in ("patchify_raw", "unpatchify_raw", "token_linear_fwd_raw", "token_linear_wgrad_raw")}
        orig_embed = ops._PatchEmbed.apply

        def counted(name, field):
            def f(*a, **k):
                setattr(self, field, getattr(self, field) + 1)
                return orig[name](*a, **k)
            return f

        def embed(*a):
            self.embed += 1
            return orig_embed(*a)

        for name, field in (("patchify_raw", "patchify"), ("unpatchify_raw", "unpatchify"), ("token_linear_fwd_raw", "gemm"),
                            ("token_linear_wgrad_raw", "wgrad")):
            monkeypatch.setattr(ops, name, counted(name, field))
        monkeypatch.setattr(ops._PatchEmbed, "apply", embed)


def _embed_case(shape, img_dtype, dev):
    B, C, H, W, p0, p1, E = shape
    N, F = (H // p0) * (W // p1), C * p0 * p1
    gen = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(B, C, H, W, generator=gen).to(img_dtype)
    w = torch.randn(E, C, p0, p1, generator=gen) / F ** 0.5
    b = torch.randn(E, generator=gen)
    pos = torch.randn(1, N, E, generator=gen)
    g = torch.randn(B, N, E, generator=gen)
    return tuple(t.to(dev) for t in (x, w, b, pos, g))


@pytest.mark.parametrize("shape", EMBED)
@pytest.mark.parametrize("img_dtype", [F32, BF16])
@pytest.mark.parametrize("with_pos", [False, True])
def test_patch_embed_every_element(dev, shape, img_dtype, with_pos, monkeypatch):
    from makani_amd import ops
    monkeypatch.setenv("MK_PATCH", "hip")
    monkeypatch.setenv("MK_TOKEN_LINEAR", "torch")                  # the embedding does not depend on that knob
    B, C, H, W, p0, p1, E = shape
    N, F = (H // p0) * (W // p1), C * p0 * p1
    R = B * N
    x, w, b, pos, g = _embed_case(shape, img_dtype, dev)
    calls = Calls(monkeypatch)

    def step():
        xi, wi, bi, pi = (t.detach().clone().requires_grad_() for t in (x, w, b, pos))
        with torch.autocast("cuda", dtype=BF16):
            assert ops.patch_embed_supported(xi, wi, bi)
            y = ops.patch_embed(xi, wi, bi, pi if with_pos else None)
        grads = torch.autograd.grad(y, [xi, wi, bi] + ([pi] if with_pos else []), g.to(y.dtype))
        return [y.detach()] + list(grads)

    first = step()
    assert (calls.embed, calls.patchify, calls.unpatchify, calls.wgrad) == (1, 1, 1, 1)
    assert calls.gemm == (B if with_pos else 1) + 1                 # one launch per sample with the position addend; one for dx
    y, dx, dw, db = first[:4]
    rows = ops._patchify_torch(x.cpu(), (p0, p1), 0).to(BF16).reshape(R, F)
    wb = w.cpu().reshape(E, F).to(BF16)
    ref = tc.Ref(rows, wb, b.cpu())
    if with_pos:
        assert y.dtype == F32 and y.shape == (B, N, E)
        print("[patch] addend", tc.check_addend(y.cpu().reshape(R, E), pos.cpu().expand(B, N, E).reshape(R, E), ref, "out"))
        assert same_bits(first[4], g.sum(0, keepdim=True))
    else:
        assert y.dtype == BF16 and y.shape == (B, N, E)
        print("[patch] plain", tc.check_plain(y.cpu().reshape(R, E), ref, "y"))
    gr = g.cpu().to(BF16).reshape(R, E)                              # the gradient of the bf16 result
    assert dw.dtype == F32 and dw.shape == w.shape and db.dtype == F32
    print("[patch] dw", tc.check_wgrad(dw.cpu().reshape(E, F), gr, rows, "dw"))
    print("[patch] db", tc.check_dbias(db.cpu(), gr, "db"))
    assert dx.dtype == img_dtype and dx.shape == x.shape
    dx_rows = ops._patchify_torch(dx.cpu(), (p0, p1), 0).reshape(R, F)       # the exact permutation back
    assert same_bits(dx_rows.to(BF16).to(img_dtype), dx_rows), "dx is not a bf16 value"
    print("[patch] dx", tc.check_plain(dx_rows.to(BF16), tc.Ref(gr, wb.T.contiguous()), "dx"))
    second = step()
    for a, c in zip(first, second):
        assert same_bits(a, c), "a second run gave other bits"


def test_bf16_module_without_autocast_and_an_image_without_gradient(dev, monkeypatch):
    """Without autocast the node takes what ``nn.Conv2d`` takes, a bf16 image with bf16 parameters, and refuses mixed dtypes as
    the convolution does; an image that asks for no gradient costs no data-gradient GEMM and no un-patchify."""
    from makani_amd import ops
    monkeypatch.setenv("MK_PATCH", "hip")
    shape = EMBED[0]
    B, C, H, W, p0, p1, E = shape
    x, w, b, pos, g = _embed_case(shape, BF16, dev)
    assert not ops.patch_embed_supported(x, w, b) and not ops.patch_embed_supported(x, w.bfloat16(), b)
    with pytest.raises(RuntimeError):
        ops.patch_embed(x, w, b)                                     # the torch expression, which refuses bf16 with fp32
    wb, bb = w.bfloat16().requires_grad_(), b.bfloat16().requires_grad_()
    pos.requires_grad_()
    assert ops.patch_embed_supported(x, wb, bb)
    calls = Calls(monkeypatch)
    y = ops.patch_embed(x, wb, bb, pos)
    dw, db, dpos = torch.autograd.grad(y, [wb, bb, pos], g)
    assert (calls.embed, calls.unpatchify, calls.wgrad, calls.gemm) == (1, 0, 1, B)
    assert y.dtype == F32 and dw.dtype == BF16 and db.dtype == BF16 and same_bits(dpos, g.sum(0, keepdim=True))
    R, F = y.shape[0] * y.shape[1], C * p0 * p1
    rows = ops._patchify_torch(x.cpu(), (p0, p1), 0).reshape(R, F)
    ref = tc.Ref(rows, wb.detach().cpu().reshape(E, F), bb.detach().float().cpu())
    tc.check_addend(y.detach().cpu().reshape(R, E), pos.detach().cpu().expand(B, -1, E).reshape(R, E), ref, "out")


@pytest.mark.parametrize("case", ["F not a multiple of 8", "fp32 without autocast", "MK_PATCH=torch"])
def test_cases_the_kernels_do_not_take_run_the_torch_expression(dev, case, monkeypatch):
    from makani_amd.layers import PatchEmbed
    monkeypatch.setenv("MK_PATCH", "torch" if case == "MK_PATCH=torch" else "hip")
    patch = (5, 5) if case == "F not a multiple of 8" else (4, 4)
    torch.manual_seed(13)
    pe = PatchEmbed(img_size=(20, 40), patch_size=patch, in_chans=3 if patch == (5, 5) else 4, embed_dim=16).to(dev)
    x = torch.randn(2, pe.proj.in_channels, 20, 40, device=dev)
    pos = torch.randn(1, pe.num_patches, 16, device=dev)
    calls = Calls(monkeypatch)
    with torch.autocast("cuda", dtype=BF16, enabled=case != "fp32 without autocast"):
        got = pe.forward_tokens(x, pos)
        want = pe.proj(x).flatten(2).transpose(1, 2) + pos
    got.sum().backward()
    assert (calls.embed, calls.patchify, calls.unpatchify, calls.gemm, calls.wgrad) == (0, 0, 0, 0, 0)
    assert got.dtype == want.dtype == F32 and got.shape == want.shape == (2, pe.num_patches, 16)
    assert torch.allclose(got, want, rtol=0, atol=2.0 ** -7 * float(want.detach().abs().max()))      # the same torch ops twice: a bf16 ulp at most
    assert pe.proj.weight.grad is not None


def _net_errors(run, wanted, monkeypatch, calls):
    errs, used = {}, {}
    for mode in ("hip", "torch"):
        monkeypatch.setenv("MK_PATCH", mode)
        before = (calls.embed, calls.unpatchify, calls.patchify)
        with torch.autocast("cuda", dtype=BF16):
            got = run()
        used[mode] = tuple(a - b for a, b in zip((calls.embed, calls.unpatchify, calls.patchify), before))
        errs[mode] = {n: vit.rel(t.float().cpu(), wanted(n)) for n, t in got.items()}
    for n in errs["hip"]:
        print(f"[patch] {n}: hip {errs['hip'][n]:.3e} torch {errs['torch'][n]:.3e}")
    # the image asks for a gradient: embed, then its dx through unpatchify, plus the head's unpatchify and its backward
    assert used["hip"] == (1, 2, 2) and used["torch"] == (0, 0, 0), f"the HIP path did not run: {used}"
    for n in errs["hip"]:
        assert errs["hip"][n] <= 2 * errs["torch"][n], (n, errs["hip"][n], errs["torch"][n])


def _vit_run(ref, net, dev):
    y, grads = vit.run(ref, net, dev)
    return dict(grads, y=y.detach())


def _afnov1_run(ref, net, dev):
    x = ref["net.x"].detach().clone().to(dev).requires_grad_(True)
    y = net(x)
    y.backward(ref["net.g"].to(dev).to(y.dtype))
    out = {n: p.grad for n, p in net.named_parameters()}
    out.update(x=x.grad, y=y.detach())
    net.zero_grad(set_to_none=True)
    return out


def test_recorded_vit_under_bf16_autocast(dev, vit_ref, monkeypatch):
    net = vit.build(vit_ref).to(dev)
    wanted = lambda n: vit_ref["y"] if n == "y" else vit.wanted(vit_ref, n)
    _net_errors(lambda: _vit_run(vit_ref, net, dev), wanted, monkeypatch, Calls(monkeypatch))


def test_recorded_afnov1_under_bf16_autocast(dev, afnov1_ref, monkeypatch):
    net = av1.build(afnov1_ref, "net").to(dev)
    wanted = lambda n: afnov1_ref["net.y"] if n == "y" else (afnov1_ref["net.gx"] if n == "x" else afnov1_ref["net.grad." + n])
    _net_errors(lambda: _afnov1_run(afnov1_ref, net, dev), wanted, monkeypatch, Calls(monkeypatch))


@pytest.mark.parametrize("which", ["vit", "afnov1"])
def test_fp32_runs_change_only_the_unpatchify(dev, which, vit_ref, afnov1_ref, monkeypatch):
    if which == "vit":
        net = vit.build(vit_ref).to(dev)
        run = lambda: _vit_run(vit_ref, net, dev)
    else:
        net = av1.build(afnov1_ref, "net").to(dev)
        run = lambda: _afnov1_run(afnov1_ref, net, dev)
    calls = Calls(monkeypatch)
    monkeypatch.setenv("MK_PATCH", "torch")
    want = run()
    assert (calls.embed, calls.unpatchify, calls.patchify) == (0, 0, 0)
    monkeypatch.setenv("MK_PATCH", "hip")
    got = run()
    assert (calls.embed, calls.unpatchify, calls.patchify) == (0, 1, 1)      # the head's un-patchify and its backward; nn.Conv2d stays
    for n in want:
        assert got[n].dtype == F32 and same_bits(got[n], want[n]), n


def test_captured_vit_step_replays_the_eager_bits(dev, vit_ref, monkeypatch):
    """One forward + backward of the small ViT under bf16 autocast with ``MK_PATCH=hip``, captured and replayed twice."""
    monkeypatch.setenv("MK_PATCH", "hip")
    net = vit.build(vit_ref).to(dev)
    params = list(net.parameters())
    x, g = vit_ref["x"].to(dev), vit_ref["g"].to(dev)
    calls = Calls(monkeypatch)

    def step(inp):
        with torch.autocast("cuda", dtype=BF16):
            y = net(inp)
        return [y] + list(torch.autograd.grad(y, [inp] + params, g.to(y.dtype)))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        static = x.clone().requires_grad_()
        eager = [t.detach().clone() for t in step(static)]
        step(static)                                                    # a second warm-up on the capture stream
        assert calls.embed == 2 and calls.unpatchify == 4
        gc.collect()
        torch.cuda.empty_cache()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            outs = step(static)
        for _ in range(2):
            graph.replay()
            side.synchronize()
            for a, b in zip(outs, eager):
                assert same_bits(a.detach(), b)
    torch.cuda.current_stream().wait_stream(side)
    assert float(eager[0].float().abs().max()) > 0
