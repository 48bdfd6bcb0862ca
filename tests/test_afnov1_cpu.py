"""The channels-last AFNO modules (``makani_amd/afnonet_v1.py``) on the CPU against ``tests/golden/ref_afnov1.npz``, the recorded run
of the reference's own ``networks/afnonet.py`` (``tests/golden/make_afnov1_golden.py``; weights, biases and threshold chosen there so
that the filter is active and no mask sits on its edge); the window arithmetic; ``mk_latdft_table_window`` through the C ABI;
``ops.spec_block_mlp`` with biases and the layout ops in their torch formulations; the fused path's formulation -- a latitude DFT
over the window's frequencies -- written out in float64 (``window_chain64``, which ``tests/test_afnov1_gpu.py`` holds the kernels
to) against the module; the launchers' validation and the dispatch.

Bound: relative L2 error <= 2e-6, the project's CPU bound (``tests/test_modules_cpu.py``)."""
import math
import os

import numpy as np
import pytest
import torch

from test_afno_cpu import rel

BOUND = 2e-6
LAM = 0.5
NET_KW = dict(inp_shape=(24, 40), patch_size=(4, 4), inp_chans=3, out_chans=2, embed_dim=16, num_layers=2, num_blocks=4,
              mlp_ratio=2, sparsity_threshold=LAM)
# (H, W, fraction) -> (first, lmax, mmax)
WINDOWS = [((8, 12, 0.5), (3, 4, 2)), ((8, 12, 1.0), (0, 8, 5)), ((9, 10, 0.7), (2, 6, 3)), ((6, 20, 1.0), (0, 6, 4)),
           ((12, 6, 1.0), (0, 12, 4)), ((10, 16, 0.25), (5, 2, 1)), ((90, 180, 1.0), (0, 90, 46))]


@pytest.fixture(scope="module")
def ref(golden_dir):
    with np.load(os.path.join(golden_dir, "ref_afnov1.npz")) as z:
        return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}


def build(ref, which):
    """The module of fixture entry ``which`` with the recorded state loaded (strictly)."""
    from makani_amd.afnonet_v1 import AFNO2D, AdaptiveFourierNeuralOperatorNet
    if which == "net":
        mod = AdaptiveFourierNeuralOperatorNet(**NET_KW)
    elif which == "afno":
        mod = AFNO2D(12, num_blocks=3, sparsity_threshold=LAM, hard_thresholding_fraction=0.5)
    else:
        mod = AFNO2D(8, num_blocks=2, sparsity_threshold=LAM, hard_thresholding_fraction=1.0)
    state = {k[len(which) + 7:]: v for k, v in ref.items() if k.startswith(which + ".state.")}
    assert {k: tuple(v.shape) for k, v in mod.state_dict().items()} == {k: tuple(v.shape) for k, v in state.items()}
    mod.load_state_dict(state, strict=True)
    return mod


def check_against_fixture(ref, which, mod, dev="cpu", fwd_bound=BOUND, grad_bound=BOUND, tag="cpu"):
    """Forward and every gradient against the recorded run.  No recorded gradient of these runs is cancellation noise (the
    smallest, ``norm2``'s, are 2e-2 in norm: layer norms over the channels remove no parameter's effect), so all are held
    relative to themselves."""
    x = ref[which + ".x"].detach().clone().to(dev).requires_grad_(True)      # a copy: the fixture is shared
    y = mod(x)
    assert y.shape == ref[which + ".y"].shape
    y.backward(ref[which + ".g"].to(dev).to(y.dtype))
    errs = {"x.grad": rel(x.grad.cpu(), ref[which + ".gx"])}
    for n, p in mod.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, n
        want = ref[f"{which}.grad.{n}"]
        assert torch.linalg.norm(want) > 1e-3, f"{n}: a recorded gradient that is noise"
        errs[n] = rel(p.grad.cpu(), want)
    e_y = rel(y.cpu(), ref[which + ".y"])
    worst = max(errs, key=errs.get)
    print(f"[afnov1] {which} {tag}: y {e_y:.2e}, worst gradient {worst} {errs[worst]:.2e}")
    assert e_y <= fwd_bound
    assert errs[worst] <= grad_bound, (worst, errs[worst])


# ---------------------------------------------------------------------------------------------------------------------
# float64 references
# ---------------------------------------------------------------------------------------------------------------------
def window_matrix(nlat, lmax, first):
    """W[l][k] = exp(-2 pi i f_l k / nlat) / sqrt(nlat), f_l = (first + l) mod nlat, the angle reduced modulo nlat in integers."""
    f = (first + torch.arange(lmax)) % nlat
    ang = ((f[:, None] * torch.arange(nlat)[None, :]) % nlat).double() * (-2.0 * math.pi / nlat)
    return torch.complex(torch.cos(ang), torch.sin(ang)) / math.sqrt(nlat)


def block_chain64(c, w1, b1, w2, b2, lam):
    """float64 torch: ``c`` complex128 [..., nb, bs]; ``w*`` complex128 [nb, i, o], ``b*`` complex128 [nb, o] -> (y, margin of the
    ReLU arguments from 0, of the soft-shrink arguments from +-lam, both in units of the components' rms)."""
    p1 = torch.view_as_real(torch.einsum("...ki,kio->...ko", c, w1) + b1)
    h = torch.view_as_complex(torch.relu(p1))
    p2 = torch.view_as_real(torch.einsum("...ki,kio->...ko", h, w2) + b2)
    y = torch.where(p2 > lam, p2 - lam, torch.where(p2 < -lam, p2 + lam, torch.zeros_like(p2)))
    m1 = float(p1.detach().abs().min() / p1.detach().square().mean().sqrt())
    m2 = float((p2.detach().abs() - lam).abs().min() / p2.detach().square().mean().sqrt())
    return torch.view_as_complex(y), m1, m2


def window_chain64(mod, x, g=None):
    """The fused path's formulation of ``AFNO2D`` (v1) in float64 from the module's parameters: longitudinal ``rfft`` truncated to
    ``mmax``, the latitude DFT matrix of the window's frequencies, the block MLP with biases on ``[L, M, B, nb, bs]``, the adjoint
    matrix, ``irfft`` with its implicit zero padding, plus the input.  -> (y, the filter term alone, x.grad, parameter
    gradients, margins)."""
    from makani_amd.afnonet_v1 import kept_window
    p = {n: t.detach().cpu().double().requires_grad_(True) for n, t in mod.named_parameters()}
    xo = x.detach().cpu().double().requires_grad_(True)
    B, H, W, C = xo.shape
    nb, bs = mod.num_blocks, mod.block_size
    first, lmax, mmax = kept_window(H, W, mod.hard_thresholding_fraction)
    Wm = window_matrix(H, lmax, first)
    xf = torch.fft.rfft(xo, dim=2, norm="ortho")[:, :, :mmax]
    c = torch.einsum("lk,bkmc->lmbc", Wm, xf).reshape(lmax, mmax, B, nb, bs)
    w1, b1, w2, b2 = (torch.complex(p[n][0], p[n][1]) for n in ("w1", "b1", "w2", "b2"))
    y, m1, m2 = block_chain64(c, w1, b1, w2, b2, mod.sparsity_threshold)
    back = torch.einsum("lk,lmbc->bkmc", Wm.conj(), y.reshape(lmax, mmax, B, C))
    r = torch.fft.irfft(back, n=W, dim=2, norm="ortho")
    out = r + xo
    grads = None
    if g is not None:
        out.backward(g.detach().cpu().double())
        grads = {n: t.grad for n, t in p.items()}
    return out.detach(), r.detach(), xo.grad, grads, (m1, m2)


def make_filter(C, nb, frac=1.0, f=1, seed=0):
    """A v1 filter with the fixture generator's settings: weights std 0.4-like (scaled with the block size), biases std 0.3."""
    from makani_amd.afnonet_v1 import AFNO2D
    torch.manual_seed(seed)
    mod = AFNO2D(C, num_blocks=nb, sparsity_threshold=LAM, hard_thresholding_fraction=frac, hidden_size_factor=f)
    with torch.no_grad():
        mod.w1.copy_(torch.randn_like(mod.w1) * 0.8 / mod.block_size ** 0.5)
        mod.w2.copy_(torch.randn_like(mod.w2) * 1.6 / (mod.block_size * f) ** 0.5)
        mod.b1.copy_(torch.randn_like(mod.b1) * 0.3)
        mod.b2.copy_(torch.randn_like(mod.b2) * 0.3)
    return mod


# ---------------------------------------------------------------------------------------------------------------------
# state, recorded runs
# ---------------------------------------------------------------------------------------------------------------------
def test_state_dict_keys_are_the_reference_s(ref):
    net = build(ref, "net")
    keys = set(net.state_dict())
    want = {"pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias", "head.weight"}
    for i in (0, 1):
        want |= {f"blocks.{i}.{n}" for n in ("norm1.weight", "norm1.bias", "filter.w1", "filter.b1", "filter.w2", "filter.b2",
                                            "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight",
                                            "mlp.fc2.bias")}
    assert keys == want == {k[len("net.state."):] for k in ref if k.startswith("net.state.")}
    assert not any("_pairs" in k or "twiddles" in k or "dft_table" in k for k in keys)
    assert net.no_weight_decay() == {"pos_embed", "cls_token"}
    assert (net.h, net.w, net.patch_embed.num_patches) == (6, 10, 60) and tuple(net.pos_embed.shape) == (1, 60, 16)
    f = net.blocks[0].filter
    assert [tuple(t.shape) for t in (f.w1, f.b1, f.w2, f.b2)] == [(2, 4, 4, 4), (2, 4, 4), (2, 4, 4, 4), (2, 4, 4)]
    assert (f.hidden_size, f.num_blocks, f.block_size, f.hidden_size_factor, f.scale) == (16, 4, 4, 1, 0.02)
    assert net.blocks[0].double_skip is True


@pytest.mark.parametrize("which", ["net", "afno", "afno_clip"])
def test_forward_and_gradients_against_the_reference_run(ref, which):
    check_against_fixture(ref, which, build(ref, which))


def test_keywords_and_variants(monkeypatch):
    """``double_skip=False``, active dropout and stochastic depth, unknown keywords tolerated, model-parallel sizes refused."""
    from makani_amd import comm
    from makani_amd.afnonet_v1 import AFNO2D, AdaptiveFourierNeuralOperatorNet, Block, Mlp
    x = torch.randn(1, 3, 24, 40)
    for extra in (dict(some_future_keyword=3, drop_path_rate=0.1, drop_rate=0.1), dict(hard_thresholding_fraction=0.5)):
        net = AdaptiveFourierNeuralOperatorNet(**dict(NET_KW, num_layers=2, **extra))
        assert tuple(net(x).shape) == (1, 2, 24, 40)
    t = torch.randn(2, 6, 10, 16)
    torch.manual_seed(0)
    blk = Block(16, mlp_ratio=2, num_blocks=4, double_skip=False).eval()
    h = blk.filter(blk.norm1(t))
    assert rel(blk(t), blk.mlp(blk.norm2(h)) + t) <= BOUND
    blk.double_skip = True
    assert rel(blk(t), blk.mlp(blk.norm2(h + t)) + (h + t)) <= BOUND
    plain = Block(16, mlp_ratio=2, num_blocks=4, norm_layer=lambda dim: torch.nn.Identity())      # any factory of `dim`
    assert tuple(plain(t).shape) == tuple(t.shape)
    m = Mlp(16, 32, drop=0.5)
    assert tuple(m(t).shape) == tuple(t.shape)       # training: every module singly
    f = AFNO2D(8, num_blocks=2, hidden_size_factor=3)
    assert tuple(f.w1.shape) == (2, 2, 4, 12) and tuple(f.b1.shape) == (2, 2, 12) and tuple(f.w2.shape) == (2, 2, 12, 4)
    with pytest.raises(AssertionError):
        AFNO2D(10, num_blocks=4)
    monkeypatch.setattr(comm, "get_size", lambda name: 2 if name == "h" else 1)
    with pytest.raises(NotImplementedError):
        AdaptiveFourierNeuralOperatorNet(**NET_KW)
    monkeypatch.setattr(comm, "get_size", lambda name: 2 if name == "data" else 1)
    AdaptiveFourierNeuralOperatorNet(**NET_KW)


# ---------------------------------------------------------------------------------------------------------------------
# the window and its table
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,want", WINDOWS)
def test_window_arithmetic(case, want):
    """``kept_window`` gives the issue's table, and those rows / columns are exactly where the reference's slices land."""
    from makani_amd.afnonet_v1 import kept_window
    H, W, frac = case
    assert kept_window(H, W, frac) == want
    first, lmax, mmax = want
    t = H // 2 + 1
    k = int(t * frac)
    mark = torch.zeros(H, W // 2 + 1)
    mark[t - k:t + k, :k] = 1
    mine = torch.zeros(H, W // 2 + 1)
    mine[first:first + lmax, :mmax] = 1
    assert torch.equal(mark, mine)


def _table(lib, nlat, lmax, first=None):
    tab = torch.full((lib.mk_latdft_table_len(nlat, lmax),), float("nan"))
    rc = lib.mk_latdft_table(nlat, lmax, tab.data_ptr()) if first is None else lib.mk_latdft_table_window(nlat, lmax, first, tab.data_ptr())
    assert rc == 0
    return tab


@pytest.mark.parametrize("nlat,lmax,first", [(8, 4, 3), (9, 6, 2), (10, 2, 5), (70, 33, 20), (8, 4, 6)])
def test_latdft_table_window_against_the_formula(nlat, lmax, first):
    """Every entry is the float64 formula rounded once to fp32 (bit for bit up to libm's last float64 bit: held to half an fp32
    ulp of 1 / sqrt(nlat) plus 1e-15), the padding is zero, the second half is the transpose; (8, 4, 6) wraps: 6, 7, 0, 1."""
    from makani_amd import _lib, ops
    lib = _lib.load()
    tab = _table(lib, nlat, lmax, first)
    assert torch.equal(tab, ops.latdft_table(nlat, lmax, first))
    KP, LP = (nlat + 3) // 4 * 4, (lmax + 3) // 4 * 4
    fc, fs = tab[:lmax * KP].view(lmax, KP), tab[lmax * KP:2 * lmax * KP].view(lmax, KP)
    ic, isn = tab[2 * lmax * KP:2 * lmax * KP + nlat * LP].view(nlat, LP), tab[2 * lmax * KP + nlat * LP:].view(nlat, LP)
    W = window_matrix(nlat, lmax, first)
    if (nlat, lmax, first) == (8, 4, 6):
        assert ((first + torch.arange(lmax)) % nlat).tolist() == [6, 7, 0, 1]
    tol = 2.0 ** -25 / math.sqrt(nlat) * 2 + 1e-15
    assert (fc[:, :nlat].double() - W.real).abs().max() <= tol and (fs[:, :nlat].double() + W.imag).abs().max() <= tol
    assert not fc[:, nlat:].any() and not fs[:, nlat:].any() and not ic[:, lmax:].any() and not isn[:, lmax:].any()
    assert torch.equal(ic[:, :lmax], fc[:, :nlat].T) and torch.equal(isn[:, :lmax], fs[:, :nlat].T)


def test_latdft_table_window_full_equals_the_plain_table_and_refusals():
    from makani_amd import _lib, ops
    lib = _lib.load()
    for nlat in (2, 9, 90):
        assert torch.equal(_table(lib, nlat, nlat, 0), _table(lib, nlat, nlat))
    out = torch.zeros(1024)
    for nlat, lmax, first in ((8, 4, -1), (8, 4, 8), (8, 1, 0), (8, 9, 0), (1, 1, 0)):
        assert lib.mk_latdft_table_window(nlat, lmax, first, out.data_ptr()) == 1, (nlat, lmax, first)
        assert "mk_latdft_table_window" in lib.mk_last_error().decode()
    assert lib.mk_latdft_table_window(8, 4, 0, None) == 1
    assert not out.any()
    for bad in (-1, 8):
        with pytest.raises(ValueError):
            ops.latdft_table(8, 4, bad)
    with pytest.raises(ValueError):
        ops.latdft_table(8, 9, 0)


# ---------------------------------------------------------------------------------------------------------------------
# the ops' torch formulations
# ---------------------------------------------------------------------------------------------------------------------
def test_spec_block_mlp_with_biases_on_cpu_against_float64_chain():
    from makani_amd import ops
    L, M, B, nb, bs, hb = 5, 4, 2, 3, 4, 6
    gen = torch.Generator().manual_seed(3)

    def crand(*s):
        return torch.complex(torch.randn(*s, generator=gen), torch.randn(*s, generator=gen))

    c, g = crand(L, M, B * nb * bs), crand(L, M, B * nb * bs)
    params = [0.5 * torch.randn(nb, bs, hb, 2, generator=gen), 0.5 * torch.randn(nb, hb, bs, 2, generator=gen),
              0.3 * torch.randn(nb * hb, 2, generator=gen), 0.3 * torch.randn(nb * bs, 2, generator=gen)]
    leaves = [t.clone().requires_grad_(True) for t in [c] + params]
    y = ops.spec_block_mlp(leaves[0], leaves[1], leaves[2], B, nb, LAM, leaves[3], leaves[4])
    y.backward(g)
    r = [c.to(torch.complex128).requires_grad_(True)] + [t.double().requires_grad_(True) for t in params]
    w1, w2 = torch.view_as_complex(r[1]), torch.view_as_complex(r[2])
    b1, b2 = torch.view_as_complex(r[3]).view(nb, hb), torch.view_as_complex(r[4]).view(nb, bs)
    yo, m1, m2 = block_chain64(r[0].view(L, M, B, nb, bs), w1, b1, w2, b2, LAM)
    assert min(m1, m2) > 1e-5
    yo = yo.reshape(L, M, -1)
    yo.backward(g.to(torch.complex128))
    assert rel(torch.view_as_real(y), torch.view_as_real(yo)) <= BOUND
    for name, a, b in zip(("c", "w1", "w2", "b1", "b2"), leaves, r):
        ga, gb = (torch.view_as_real(t.grad) if t.grad.is_complex() else t.grad for t in (a, b))
        assert ga.shape == gb.shape and rel(ga, gb) <= BOUND, name
    # without biases: the former call, unchanged
    assert torch.equal(ops.spec_block_mlp(c, params[0], params[1], B, nb, LAM),
                       ops.spec_block_mlp(c, params[0], params[1], B, nb, LAM, None, None))
    with pytest.raises(AssertionError):
        ops.spec_block_mlp(c, params[0], params[1], B, nb, LAM, params[3], params[2])


@pytest.mark.parametrize("which,frac", [("afno", None), ("afno_clip", None), ("new", 0.7), ("new", 0.25)])
def test_window_chain_is_the_module_s_function(ref, which, frac):
    """The float64 window-DFT chain against the module's CPU forward (the reference's formulation) and its gradients."""
    if which == "new":
        mod, x = make_filter(8, 2, frac, f=2, seed=1), torch.randn(2, 9 if frac == 0.7 else 10, 10 if frac == 0.7 else 16, 8)
        g = torch.randn_like(x)
    else:
        mod, x, g = build(ref, which), ref[which + ".x"], ref[which + ".g"]
    yo, _, gxo, gpo, margins = window_chain64(mod, x, g)
    assert min(margins) > 1e-5
    xr = x.detach().clone().requires_grad_(True)
    y = mod(xr)
    y.backward(g)
    assert rel(y, yo) <= BOUND and rel(xr.grad, gxo) <= BOUND
    for n, p in mod.named_parameters():
        assert rel(p.grad, gpo[n]) <= BOUND, n


def test_layout_ops_on_cpu():
    from makani_amd import ops
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.randn(2, 7, 5).to(dtype).requires_grad_(True)
        a = torch.randn(2, 7, 5).to(dtype).requires_grad_(True)
        f = ops.tokens_to_fields(x)
        assert f.is_contiguous() and torch.equal(f, x.detach().transpose(1, 2))
        g = torch.randn(2, 5, 7).to(dtype)
        f.backward(g)
        assert torch.equal(x.grad, g.transpose(1, 2))
        r = torch.randn(2, 5, 7).to(dtype).requires_grad_(True)
        t = ops.fields_to_tokens(r, a)
        assert t.is_contiguous() and torch.equal(t, r.detach().transpose(1, 2) + a.detach())
        gt = torch.randn(2, 7, 5).to(dtype)
        t.backward(gt)
        assert torch.equal(r.grad, gt.transpose(1, 2)) and torch.equal(a.grad, gt)
        assert torch.equal(ops.fields_to_tokens(r.detach()), r.detach().transpose(1, 2)) and ops.fields_to_tokens(r.detach()).is_contiguous()
    with pytest.raises(AssertionError):
        ops.tokens_to_fields(torch.zeros(2, 3, 4, dtype=torch.float64))
    for call in (lambda: ops.tokens_to_fields_raw(torch.zeros(1, 2, 3)), lambda: ops.fields_to_tokens_raw(torch.zeros(1, 2, 3))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


# ---------------------------------------------------------------------------------------------------------------------
# validation and dispatch
# ---------------------------------------------------------------------------------------------------------------------
def test_launchers_validate_before_launching():
    """Code 1 and a message; nothing is launched (the pointers are never dereferenced, there need be no device)."""
    from makani_amd import _lib
    lib = _lib.load()
    P = 4096
    assert lib.mk_tokens_to_fields(None, P, 0, 1, 4, 4, None) == 1 and "mk_tokens_to_fields" in lib.mk_last_error().decode()
    assert lib.mk_tokens_to_fields(P, None, 0, 1, 4, 4, None) == 1
    assert lib.mk_tokens_to_fields(P, P, 0, 1, 0, 4, None) == 1 and "bad sizes" in lib.mk_last_error().decode()
    assert lib.mk_tokens_to_fields(P, P, 0, 1, 4, 0, None) == 1
    assert lib.mk_tokens_to_fields(P, P, 0, 0, 4, 4, None) == 1
    assert lib.mk_tokens_to_fields(P, P, 2, 1, 4, 4, None) == 1 and "dtype" in lib.mk_last_error().decode()
    assert lib.mk_tokens_to_fields(P + 2, P, 0, 1, 4, 4, None) == 1
    assert lib.mk_tokens_to_fields(P, P, 0, 1 << 20, 1 << 12, 1 << 12, None) == 1 and "grid" in lib.mk_last_error().decode()
    assert lib.mk_fields_to_tokens(None, None, P, 0, 1, 4, 4, None) == 1 and "mk_fields_to_tokens" in lib.mk_last_error().decode()
    assert lib.mk_fields_to_tokens(P, None, None, 1, 1, 4, 4, None) == 1
    assert lib.mk_fields_to_tokens(P, None, P, 0, 1, 0, 4, None) == 1
    assert lib.mk_fields_to_tokens(P, None, P, -1, 1, 4, 4, None) == 1
    assert lib.mk_fields_to_tokens(P, P + 1, P, 1, 1, 4, 4, None) == 1
    assert lib.mk_spec_bdmlp_fwd_bias(None, P, P, P, 8, 2, 4, 4, 0, 0.0, None) == 1
    assert lib.mk_spec_bdmlp_fwd_bias(P, P, P + 4, P, 8, 2, 4, 4, 0, 0.0, None) == 1 and "8-byte" in lib.mk_last_error().decode()
    assert lib.mk_spec_bdmlp_fwd_bias(P, P, P, P, 8, 2, 3, 4, 0, 0.0, None) == 1 and "even block sizes" in lib.mk_last_error().decode()
    assert lib.mk_spec_bdmlp_fwd_bias(P, P, P, P, 8, 2, 4, 5, 2, 0.0, None) == 1
    assert lib.mk_spec_bdmlp_fwd_bias(P, P, P, P, 8, 2, 4, 4, 1, 0.0, None) == 1
    assert lib.mk_spec_bdmlp_fwd_bias(P, P, P, P, 8, 2, 4, 4, 3, -0.5, None) == 1
    assert lib.mk_spec_bdmlp_fwd_bias(P, P, None, P, 8, 2, 3, 4, 0, 0.0, None) == 1     # NULL bias: mk_spec_bdmlp_fwd's checks


def test_unknown_knob_raises(ref, monkeypatch):
    monkeypatch.setenv("MK_AFNOV1", "bogus")
    with pytest.raises(ValueError, match="MK_AFNOV1"):
        build(ref, "afno")(ref["afno.x"])


def test_cases_the_kernels_do_not_take_run_on_the_torch_path(monkeypatch):
    """Odd block size, odd width, an empty window (and, here, CPU tensors at all)."""
    from makani_amd import ops
    from makani_amd.afnonet_v1 import AFNO2D
    monkeypatch.setenv("MK_AFNOV1", "hip")
    monkeypatch.setenv("MK_PLANAR_FFT", "hip")
    for name in ("spec_block_mlp", "tokens_to_fields", "fields_to_tokens"):
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("the fused path was taken"))
    for C, nb, H, W, frac in ((9, 3, 6, 8, 1.0), (8, 2, 6, 7, 1.0), (8, 2, 6, 8, 0.2)):
        f = AFNO2D(C, num_blocks=nb, sparsity_threshold=0.01, hard_thresholding_fraction=frac)
        x = torch.randn(2, H, W, C, requires_grad=True)
        assert not f._takes_fused(x)
        y = f(x)
        y.sum().backward()
        assert y.shape == x.shape and torch.isfinite(y).all() and x.grad is not None and f.w1.grad is not None
    f = AFNO2D(8, num_blocks=2, hard_thresholding_fraction=0.2)      # int(4 * 0.2) = 0 kept modes: the filter is the identity
    x = torch.randn(1, 6, 8, 8)
    assert torch.equal(f(x), x)


def test_file_path_registration_like_model_registry():
    """model_registry.py:63-79: 'path/to/afnonet_v1.py:Name' through spec_from_file_location, then instantiate."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("AdaptiveFourierNeuralOperatorNet", os.path.join(root, "makani_amd", "afnonet_v1.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    net = module.AdaptiveFourierNeuralOperatorNet(**dict(NET_KW, num_layers=1))
    assert isinstance(net, torch.nn.Module) and tuple(net(torch.zeros(1, 3, 24, 40)).shape) == (1, 2, 24, 40)
