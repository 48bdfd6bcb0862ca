"""Patch rows without a device: the declarations and refusals of ``mk_patchify`` / ``mk_unpatchify``, the torch formulations of
``ops.patchify`` / ``ops.unpatchify`` against ``F.conv2d`` and both networks' own rearrangements, ``PatchEmbed.forward_tokens``
against the expression it replaces, and both recorded networks bit for bit under every value of ``MK_PATCH``."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

import test_afnov1_cpu as av1
import test_vit_cpu as vit
from test_afnov1_cpu import ref as afnov1_ref      # noqa: F401  (module-scoped fixtures)
from test_vit_cpu import ref as vit_ref            # noqa: F401

CASES = [(1, 1, 7, 8, 7, 8), (2, 3, 14, 24, 7, 8), (1, 5, 6, 10, 3, 5), (2, 8, 16, 32, 8, 8), (1, 2, 9, 260, 3, 4)]


def test_header_declares_and_library_exports():
    from makani_amd import _lib
    lib = _lib.load()
    ll, i, p = ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p
    assert _lib.SIGNATURES["mk_patchify"] == (i, [p, i, p, i, ll, i, i, i, i, i, i, i, p])
    assert _lib.SIGNATURES["mk_unpatchify"] == (i, [p, i, ll, p, i, i, i, i, i, i, i, i, p])
    assert _lib.SIGNATURES["mk_patch_tile_info"] == (i, [i, i, i, i, i, i, ll, p])
    assert lib.mk_patchify is not None and lib.mk_unpatchify is not None
    from makani_amd import build
    assert "patch.hip" in build.SOURCES


def test_launchers_validate_before_launching():
    """Code 1 and a message; nothing is launched (the pointers are never dereferenced, there need be no device)."""
    from makani_amd import _lib
    lib = _lib.load()
    P = 4096
    F_ = 3 * 7 * 8

    def pat(img=P, idt=0, tok=P, tdt=1, ldt=F_, B=2, C=3, H=14, W=24, p0=7, p1=8, order=0):
        return lib.mk_patchify(img, idt, tok, tdt, ldt, B, C, H, W, p0, p1, order, None)

    def unp(tok=P, tdt=1, ldt=F_, img=P, idt=0, B=2, C=3, H=14, W=24, p0=7, p1=8, order=0):
        return lib.mk_unpatchify(tok, tdt, ldt, img, idt, B, C, H, W, p0, p1, order, None)

    for name, fn in (("mk_patchify", pat), ("mk_unpatchify", unp)):
        msg = lambda: lib.mk_last_error().decode()
        assert fn(img=None) == 1 and name in msg() and "null" in msg()
        assert fn(tok=None) == 1 and "null" in msg()
        for bad in (2, -1):
            assert fn(idt=bad) == 1 and "dtype" in msg()
            assert fn(tdt=bad) == 1 and "dtype" in msg()
            assert fn(order=bad) == 1 and "order" in msg()
        assert fn(H=15) == 1 and "divide" in msg()
        assert fn(W=25) == 1 and "divide" in msg()
        assert fn(ldt=F_ - 1) == 1 and "ldt" in msg()
        for key in ("B", "C", "p0", "p1"):
            assert fn(**{key: 0}) == 1 and "sizes" in msg(), key
            assert fn(**{key: -1}) == 1, key
        assert fn(H=0) == 1 and fn(W=0) == 1
        assert fn(img=P + 2, idt=0) == 1 and "aligned" in msg()
        assert fn(tok=P + 1, tdt=1) == 1 and "aligned" in msg()


@pytest.mark.parametrize("case", CASES)
def test_order_0_is_the_convolution_s(case):
    from makani_amd import ops
    B, C, H, W, p0, p1 = case
    torch.manual_seed(0)
    x = torch.randn(B, C, H, W, dtype=torch.float64)
    w = torch.randn(6, C, p0, p1, dtype=torch.float64)
    b = torch.randn(6, dtype=torch.float64)
    rows = ops.patchify(x, (p0, p1), order=0)
    assert rows.shape == (B, (H // p0) * (W // p1), C * p0 * p1)
    got = rows @ w.view(6, -1).T + b
    want = F.conv2d(x, w, b, stride=(p0, p1)).flatten(2).transpose(1, 2)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    assert torch.equal(ops.patch_embed(x, w, b), want)          # the torch expression itself


@pytest.mark.parametrize("case", CASES)
def test_order_1_is_both_heads(case):
    from makani_amd import ops
    B, C, H, W, p0, p1 = case
    hp, wp = H // p0, W // p1
    torch.manual_seed(1)
    t = torch.randn(B, hp, wp, p0 * p1 * C)
    got = ops.unpatchify(t, (p0, p1), C, (H, W), order=1)
    vit_way = torch.einsum("nhwpqc->nchpwq", t.reshape(B, hp, wp, p0, p1, C)).reshape(B, C, H, W)
    afno_way = torch.permute(t.view(B, hp, wp, p0, p1, -1), (0, 5, 1, 3, 2, 4)).contiguous().view(B, -1, hp * p0, wp * p1)
    assert torch.equal(got, vit_way) and torch.equal(got, afno_way)
    assert torch.equal(ops.unpatchify(t.reshape(B, hp * wp, -1), (p0, p1), C, (H, W), order=1), got)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("order", [0, 1])
def test_inverse_pairs_adjoints_and_casts(case, order):
    from makani_amd import ops
    B, C, H, W, p0, p1 = case
    torch.manual_seed(2)
    x = torch.randn(B, C, H, W, requires_grad=True)
    rows = ops.patchify(x, (p0, p1), order)
    assert torch.equal(ops.unpatchify(rows, (p0, p1), C, (H, W), order), x)
    t = torch.randn_like(rows).requires_grad_(True)
    img = ops.unpatchify(t, (p0, p1), C, (H, W), order)
    assert torch.equal(ops.patchify(img, (p0, p1), order), t)
    # autograd of one is the other
    g = torch.randn_like(rows)
    rows.backward(g)
    assert torch.equal(x.grad, ops.unpatchify(g, (p0, p1), C, (H, W), order))
    gi = torch.randn_like(img)
    img.backward(gi)
    assert torch.equal(t.grad, ops.patchify(gi, (p0, p1), order))
    # the cast is torch's
    with torch.no_grad():
        assert torch.equal(ops.patchify(x, (p0, p1), order, dtype=torch.bfloat16), rows.detach().to(torch.bfloat16))
        assert ops.unpatchify(t.bfloat16(), (p0, p1), C, (H, W), order, dtype=torch.float32).dtype == torch.float32
    with pytest.raises(ValueError):
        ops.patchify(x, (p0, p1), order=2)
    with pytest.raises(ValueError):
        ops.patchify(x, (p0 + 1, p1), order)
    with pytest.raises(ValueError):
        ops.unpatchify(rows.detach()[..., :-1], (p0, p1), C, (H, W), order)
    if rows.shape[1] > 1:
        with pytest.raises(ValueError):
            ops.unpatchify(rows.detach()[0, :-1], (p0, p1), C, (H, W), order)


@pytest.mark.parametrize("mode", [None, "hip", "torch"])
def test_forward_tokens_is_the_old_expression(mode, monkeypatch):
    from makani_amd.layers import PatchEmbed
    if mode is None:
        monkeypatch.delenv("MK_PATCH", raising=False)
    else:
        monkeypatch.setenv("MK_PATCH", mode)
    torch.manual_seed(3)
    pe = PatchEmbed(img_size=(14, 24), patch_size=(7, 8), in_chans=3, embed_dim=16)
    assert set(pe.state_dict()) == {"proj.weight", "proj.bias"}
    assert pe.proj.weight.is_shared_mp == ["spatial"] and pe.proj.bias.is_shared_mp == ["spatial"]
    pos = torch.randn(1, pe.num_patches, 16)
    x = torch.randn(2, 3, 14, 24)
    old = pe(x).transpose(1, 2)
    assert old.shape == (2, 6, 16)
    assert torch.equal(pe.forward_tokens(x), old)
    assert torch.equal(pe.forward_tokens(x, pos), old + pos)
    with pytest.raises(AssertionError):
        pe.forward_tokens(torch.randn(2, 3, 14, 16))


def test_knob_and_default(monkeypatch):
    from makani_amd import ops
    from makani_amd.layers import PatchEmbed
    assert ops.PATCH_DEFAULT in ("hip", "torch")
    monkeypatch.delenv("MK_PATCH", raising=False)
    assert ops.patch_hip() == (ops.PATCH_DEFAULT == "hip")
    monkeypatch.setenv("MK_PATCH", "hip")
    assert ops.patch_hip()
    monkeypatch.setenv("MK_PATCH", "torch")
    assert not ops.patch_hip()
    monkeypatch.setenv("MK_PATCH", "bogus")
    with pytest.raises(ValueError, match="MK_PATCH"):
        ops.patch_hip()
    with pytest.raises(ValueError, match="MK_PATCH"):
        PatchEmbed(img_size=(14, 24), patch_size=(7, 8), in_chans=3, embed_dim=16).forward_tokens(torch.randn(1, 3, 14, 24))
    with pytest.raises(ValueError, match="MK_PATCH"):
        ops.unpatchify(torch.randn(1, 6, 168), (7, 8), 3, (14, 24), order=1)
    # no device tensor is ever supported here, whatever the knob says
    monkeypatch.setenv("MK_PATCH", "hip")
    assert not ops.patch_embed_supported(torch.randn(1, 8, 8, 8).bfloat16(), torch.randn(8, 8, 4, 4), torch.randn(8))


def _net_runs(monkeypatch, make, run):
    out = {}
    for mode in (None, "hip", "torch"):
        if mode is None:
            monkeypatch.delenv("MK_PATCH", raising=False)
        else:
            monkeypatch.setenv("MK_PATCH", mode)
        out[mode] = run(make())
    monkeypatch.setenv("MK_PATCH", "bogus")
    with pytest.raises(ValueError, match="MK_PATCH"):
        run(make())
    monkeypatch.delenv("MK_PATCH")
    return out


def test_vit_on_the_cpu_is_bit_equal_under_every_knob_value(vit_ref, monkeypatch):
    def run(net):
        y, grads = vit.run(vit_ref, net)
        return dict(grads, y=y.detach())

    out = _net_runs(monkeypatch, lambda: vit.build(vit_ref), run)
    for mode in ("hip", "torch"):
        for n, t in out[None].items():
            assert torch.equal(out[mode][n], t), (mode, n)
    # and it is the function of the expressions this replaces
    net = vit.build(vit_ref)
    x = vit_ref["x"]
    tok = net.prepare_tokens(x)
    assert torch.equal(tok, net.pos_drop(net.patch_embed(x).transpose(1, 2) + net.pos_embed))
    B, (h, w), (ph, pw) = x.shape[0], net.patch_embed.red_img_size, net.patch_size
    z = net.head(tok.reshape(B, h, w, net.embed_dim)).reshape(B, h, w, ph, pw, net.out_ch)
    assert torch.equal(net.forward_head(tok), torch.einsum("nhwpqc->nchpwq", z).reshape(B, net.out_ch, *net.img_size))


def test_afnov1_on_the_cpu_is_bit_equal_under_every_knob_value(afnov1_ref, monkeypatch):
    def run(net):
        x = afnov1_ref["net.x"].detach().clone().requires_grad_(True)
        y = net(x)
        y.backward(afnov1_ref["net.g"])
        out = {n: p.grad for n, p in net.named_parameters()}
        out.update(x=x.grad, y=y.detach())
        return out

    out = _net_runs(monkeypatch, lambda: av1.build(afnov1_ref, "net"), run)
    for mode in ("hip", "torch"):
        for n, t in out[None].items():
            assert torch.equal(out[mode][n], t), (mode, n)
    net = av1.build(afnov1_ref, "net")
    x = afnov1_ref["net.x"]
    t = net.head(net.forward_features(x))
    b = t.shape[0]
    xv = t.view(b, net.h, net.w, net.patch_size[0], net.patch_size[1], -1)
    old = torch.permute(xv, (0, 5, 1, 3, 2, 4)).contiguous().view(b, -1, net.h * net.patch_size[0], net.w * net.patch_size[1])
    assert torch.equal(net(x), old)


# ---------------------------------------------------------------------------------------------------------------------
# the tile choice of csrc/patch.hip (``mk_patch_tile_info``, no device) under a model of the kernels' index maps
# ---------------------------------------------------------------------------------------------------------------------
TILE_FIELDS = ("CC", "IT", "TX", "JT", "pitch", "nct", "nit", "nxt", "njt", "words", "ivec4", "ivec8", "tvec4", "tvec8")
# (C, H, W, p0, p1): the geometries of tests/test_patch_gpu.py, then extremes no GPU test needs to hold
GPU_CUT_CASES = [(73, 14, 160, 7, 8), (26, 16, 168, 8, 8), (1, 1, 2600, 1, 1300), (2, 2, 2082, 2, 1041), (160, 2, 136, 1, 8), (150, 1, 136, 1, 8)]
MODEL_CASES = [c[1:] for c in CASES] + [(73, 14, 16, 7, 8)] + GPU_CUT_CASES + [(3, 4, 2080, 2, 1040), (2, 2, 600, 1, 300), (200, 2, 16, 2, 8),
                                                                              (2, 400, 8, 200, 4), (16, 4, 64, 2, 4), (1, 3, 258, 3, 129)]


def tile_info(C, H, W, p0, p1, order, ldt=None):
    from makani_amd import _lib
    out = (ctypes.c_int * len(TILE_FIELDS))()
    rc = _lib.load().mk_patch_tile_info(C, H, W, p0, p1, order, C * p0 * p1 if ldt is None else ldt, ctypes.addressof(out))
    assert rc == 0
    return dict(zip(TILE_FIELDS, out))


def model_patchify(C, H, W, p0, p1, order, ldt, g, VI, VT):
    """``patch_kernel<PATCHIFY>`` of one sample in Python, workgroup by workgroup and lane by lane, on an image that holds its own
    flat indices: the rows it writes (-1: never written).  ``VI`` / ``VT``: elements per access on the image / token side.
    Asserts what the kernel relies on: every LDS index inside the tile and filled before it is drained, every vector aligned,
    inside one image row or one run of consecutive features, and no destination element written twice."""
    import numpy as np
    hp, wp = H // p0, W // p1
    tok = -np.ones(hp * wp * ldt, dtype=np.int64)
    for bid0 in range(hp * g["nit"] * g["nct"] * g["nxt"] * g["njt"]):
        bid, jt = divmod(bid0, g["njt"])
        bid, xt = divmod(bid, g["nxt"])
        bid, ct = divmod(bid, g["nct"])
        y, it = divmod(bid, g["nit"])
        c0, i0, j0, x0 = ct * g["CC"], it * g["IT"], jt * g["JT"], xt * g["TX"]
        CCe, ITe, TXe, Je = min(g["CC"], C - c0), min(g["IT"], p0 - i0), min(g["TX"], wp - x0), min(g["JT"], p1 - j0)
        assert min(CCe, ITe, TXe, Je) >= 1
        ibase = (c0 * H + y * p0 + i0) * W + x0 * p1 + j0
        tbase = (y * wp + x0) * ldt
        rows, cols = CCe * ITe, TXe * Je
        per_tok = rows * Je
        assert cols % VI == 0 and per_tok % VT == 0
        tile = -np.ones(g["words"], dtype=np.int64)
        for e in range(rows * (cols // VI)):
            row, col = divmod(e, cols // VI)
            col *= VI
            c_l, i_l = divmod(row, ITe)
            off = ibase + (c_l * H + i_l) * W + col
            assert off % VI == 0 and (off + VI - 1) // W == off // W and off + VI <= C * H * W
            for q in range(VI):
                tile[row * g["pitch"] + col + q] = off + q
        for e in range(TXe * (per_tok // VT)):
            x_l, k = divmod(e, per_tok // VT)
            k *= VT
            if order == 0:
                row, jj = divmod(k, Je)
                c_l, i_l = divmod(row, ITe)
            else:
                t, c_l = divmod(k, CCe)
                i_l, jj = divmod(t, Je)
            first = None
            for q in range(VT):
                c, i, j = c0 + c_l, i0 + i_l, j0 + jj
                feat = (c * p0 + i) * p1 + j if order == 0 else (i * p1 + j) * C + c
                first = feat if first is None else first
                assert feat == first + q and feat < C * p0 * p1, "a vector leaves its run of consecutive features"
                off = tbase + x_l * ldt + feat
                assert (off - q) % VT == 0
                lds = (c_l * ITe + i_l) * g["pitch"] + x_l * Je + jj
                assert 0 <= lds < g["words"] and tile[lds] >= 0 and tok[off] == -1
                tok[off] = tile[lds]
                if order == 0:
                    jj += 1
                    if jj == Je:
                        jj, i_l = 0, i_l + 1
                        if i_l == ITe:
                            i_l, c_l = 0, c_l + 1
                else:
                    c_l += 1
                    if c_l == CCe:
                        c_l, jj = 0, jj + 1
                        if jj == Je:
                            jj, i_l = 0, i_l + 1
    return tok.reshape(hp * wp, ldt)


@pytest.mark.parametrize("geom", MODEL_CASES)
def test_tile_choice_under_a_model_of_the_index_maps(geom):
    """Every destination element exactly once and equal to the torch formulation, for the tile the library chooses, with single
    elements and with every vector width the library would take (the unpatchify kernel runs the same two maps the other way)."""
    import numpy as np
    from makani_amd import ops
    C, H, W, p0, p1 = geom
    F_ = C * p0 * p1
    img = torch.arange(C * H * W, dtype=torch.int64).reshape(1, C, H, W)
    for order in (0, 1):
        want = ops._patchify_torch(img, (p0, p1), order)[0].numpy()
        for ldt in (F_, F_ + 8):
            g = tile_info(C, H, W, p0, p1, order, ldt)
            assert g["TX"] * g["JT"] <= g["pitch"] and g["CC"] * g["IT"] * g["pitch"] <= g["words"]
            assert (g["nct"], g["nit"], g["nxt"], g["njt"]) == tuple(-(-a // b) for a, b in ((C, g["CC"]), (p0, g["IT"]), (W // p1, g["TX"]), (p1, g["JT"])))
            widths = [(1, 1)] + [(vi, vt) for vi, vt in ((4, 4), (8, 8), (4, 8), (8, 4), (4, 1), (1, 8))
                                 if (vi == 1 or g[f"ivec{vi}"]) and (vt == 1 or g[f"tvec{vt}"])]
            if C * H * W > 50000:                       # the large geometries: single elements and the widest vectors only
                widths = widths[:1] + [w for w in widths[1:3] if w[0] == w[1]][-1:]
            for vi, vt in widths:
                got = model_patchify(C, H, W, p0, p1, order, ldt, g, vi, vt)
                assert np.array_equal(got[:, :F_], want) and (got[:, F_:] == -1).all(), (geom, order, ldt, vi, vt)


def test_the_gpu_cases_leave_a_single_tile_in_every_direction():
    """What tests/test_patch_gpu.py relies on for its cutting geometries, and what the production shapes use."""
    t = tile_info(73, 14, 160, 7, 8, 0)
    assert t["nxt"] == 3 and 20 % t["TX"] != 0 and t["nct"] == 5 and t["ivec8"] and t["tvec8"]
    t = tile_info(73, 14, 160, 7, 8, 1)
    assert t["nxt"] == 3 and (t["CC"], t["IT"], t["nit"]) == (73, 1, 7) and t["tvec8"]        # 16-byte stores at C = 73
    t = tile_info(26, 16, 168, 8, 8, 1)
    assert (t["IT"], t["nit"]) == (5, 2) and t["nxt"] == 3
    for geom in ((1, 1, 2600, 1, 1300), (2, 2, 2082, 2, 1041)):
        for order in (0, 1):
            t = tile_info(*geom, order)
            assert t["njt"] == 2 and geom[4] % t["JT"] != 0 and t["nxt"] == 2
    assert tile_info(1, 1, 2600, 1, 1300, 0)["ivec4"] and not any(tile_info(2, 2, 2082, 2, 1041, 0)[k] for k in TILE_FIELDS[10:])
    t = tile_info(160, 2, 136, 1, 8, 1)
    assert t["nct"] == 2 and t["CC"] % 8 == 0 and t["tvec8"] and t["nxt"] == 3
    t = tile_info(150, 1, 136, 1, 8, 1)
    assert t["nct"] == 2 and not t["tvec8"] and not t["tvec4"]            # C beyond the tile and no multiple of 8: single elements
    assert tile_info(160, 2, 136, 1, 8, 0)["nct"] == 2
    # the production shapes: vit_73ch and AFNOv1 at 26 channels
    t = tile_info(73, 721, 1440, 7, 8, 0)
    assert t["nxt"] == 23 and 180 % t["TX"] == 4 and t["nct"] == 5 and t["ivec4"] and t["ivec8"] and t["tvec8"]
    t = tile_info(73, 721, 1440, 7, 8, 1)
    assert (t["CC"], t["nit"], t["nxt"]) == (73, 7, 23) and t["tvec8"] and t["tvec4"]
    t = tile_info(26, 720, 1440, 8, 8, 1)
    assert (t["IT"], t["nit"]) == (5, 2)
    # the refusals of the query itself
    from makani_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_int * 14)()
    assert lib.mk_patch_tile_info(3, 14, 24, 7, 8, 0, 168, None) == 1
    assert lib.mk_patch_tile_info(3, 14, 24, 7, 8, 2, 168, ctypes.addressof(out)) == 1
    assert lib.mk_patch_tile_info(3, 15, 24, 7, 8, 0, 168, ctypes.addressof(out)) == 1
    assert lib.mk_patch_tile_info(3, 14, 24, 7, 8, 0, 167, ctypes.addressof(out)) == 1
