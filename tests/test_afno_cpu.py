"""The AFNO modules on the CPU against ``tests/golden/ref_afno.npz``, the recorded run of the reference's own
``afnonet_v2.py`` (``tests/golden/make_afno_golden.py``; weights and threshold chosen there so that the filter is active and no
mask sits on its edge), and ``ops.spec_block_mlp``'s torch formulation against a float64 chain written out here.

Bound: relative L2 error <= 2e-6, the project's CPU bound (``tests/test_modules_cpu.py``)."""
import os

import numpy as np
import pytest
import torch

import capi_checks as capi

BOUND = 2e-6
NET_KW = dict(inp_shape=(24, 40), patch_size=(4, 4), inp_chans=3, out_chans=2, embed_dim=16, num_layers=2, num_blocks=4,
              mlp_ratio=2, normalization_layer="instance_norm", skip_fno="linear", sparsity_threshold=0.5)


@pytest.fixture(scope="module")
def ref(golden_dir):
    with np.load(os.path.join(golden_dir, "ref_afno.npz")) as z:
        return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}


# Gradients that are exactly zero in the net: a constant per channel in front of an instance norm without running statistics
# (norm2 of the same block) changes nothing behind it.  ``filter.b1`` and ``skip_layer.bias`` are such constants, and so is
# ``norm1.bias``: a constant input reaches only the (0, 0) coefficient of the filter, whose output is again a constant.
ZERO_GRADIENTS = ("norm1.bias", "skip_layer.bias", "filter.b1")
COMPANION = {"bias": "weight", "b1": "w1"}


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return (torch.linalg.norm(a - b) / torch.linalg.norm(b)).item()


def _sub(ref, prefix):
    return {k[len(prefix):]: v for k, v in ref.items() if k.startswith(prefix)}


def build(ref, which):
    """The module of fixture entry ``which`` with the recorded state loaded (strictly)."""
    from makani_amd.afnonet import AFNO2D, AdaptiveFourierNeuralOperatorNet
    from makani_amd.layers import PatchEmbed
    if which == "net":
        mod = AdaptiveFourierNeuralOperatorNet(**NET_KW)
    elif which == "afno":
        mod = AFNO2D(12, num_blocks=3, sparsity_threshold=0.5, hard_thresholding_fraction=0.5)
    else:
        mod = PatchEmbed(img_size=(8, 12), patch_size=(2, 3), in_chans=3, embed_dim=5)
    state = _sub(ref, which + ".state.")
    assert {k: tuple(v.shape) for k, v in mod.state_dict().items()} == {k: tuple(v.shape) for k, v in state.items()}
    mod.load_state_dict(state, strict=True)
    return mod


def check_against_fixture(ref, which, mod, dev="cpu", fwd_bound=BOUND, grad_bound=BOUND, tag="cpu"):
    x = ref[which + ".x"].to(dev).requires_grad_(True)
    y = mod(x)
    assert y.shape == ref[which + ".y"].shape
    y.backward(ref[which + ".g"].to(dev).to(y.dtype))
    errs = {"x.grad": rel(x.grad.cpu(), ref[which + ".gx"])}
    for n, p in mod.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, n
        want = ref[f"{which}.grad.{n}"]
        if which == "net" and n.endswith(ZERO_GRADIENTS):
            # the recorded values are the reference's own rounding noise (3e-9 against 1e-2 for the weight next to them): the
            # error is measured against that weight's gradient, the scale of what the sum cancels from
            scale = torch.linalg.norm(ref[f"{which}.grad.{n[:n.rindex('.')]}.{COMPANION[n[n.rindex('.') + 1:]]}"].double())
            assert torch.linalg.norm(want.double()) < 1e-5 * scale, n
            errs[n] = (torch.linalg.norm(p.grad.detach().cpu().double() - want.double()) / scale).item()
        else:
            errs[n] = rel(p.grad.cpu(), want)
    e_y = rel(y.cpu(), ref[which + ".y"])
    worst = max(errs, key=errs.get)
    print(f"[afno] {which} {tag}: y {e_y:.2e}, worst gradient {worst} {errs[worst]:.2e}")
    assert e_y <= fwd_bound
    assert errs[worst] <= grad_bound, (worst, errs[worst])


def test_state_dict_keys_are_the_reference_s(ref):
    net = build(ref, "net")
    keys = set(net.state_dict())
    for k in ("patch_embed.proj.weight", "patch_embed.proj.bias", "pos_embed", "blocks.1.norm1.weight", "blocks.0.norm2.bias",
              "blocks.0.filter.w1", "blocks.0.filter.b1", "blocks.1.filter.w2", "blocks.0.skip_layer.weight",
              "blocks.0.mlp.fwd.0.weight", "blocks.1.mlp.fwd.3.bias", "head.weight"):
        assert k in keys, k
    assert not any("_pairs" in k or "twiddles" in k or "dft_table" in k for k in keys)
    assert net.no_weight_decay() == {"pos_embed", "cls_token"}
    assert (net.h, net.w, net.patch_embed.num_patches) == (6, 10, 60)
    assert tuple(net.blocks[0].filter.w1.shape) == (4, 4, 4, 2) and tuple(net.blocks[0].filter.b1.shape) == (1, 16, 1, 1)


@pytest.mark.parametrize("which", ["net", "afno", "pe"])
def test_forward_and_gradients_against_the_reference_run(ref, which):
    check_against_fixture(ref, which, build(ref, which))


def test_complex_and_real_einsum_agree(ref):
    from makani_amd.afnonet import AFNO2D
    a = build(ref, "afno")
    b = AFNO2D(12, num_blocks=3, sparsity_threshold=0.5, hard_thresholding_fraction=0.5, use_complex_kernels=True)
    b.load_state_dict(a.state_dict())
    x = ref["afno.x"]
    assert rel(b(x), a(x)) <= BOUND


def test_keywords_and_variants():
    """identity / no skip, layer norm, unknown keywords tolerated, unknown normalization refused, hidden_size_factor."""
    from makani_amd.afnonet import AFNO2D, AdaptiveFourierNeuralOperatorNet
    kw = dict(NET_KW, num_layers=1)
    x = torch.randn(1, 3, 24, 40)
    for extra in (dict(skip_fno="identity"), dict(skip_fno=None), dict(normalization_layer="layer_norm", nested_skip_fno=False),
                  dict(some_future_keyword=3, drop_path_rate=0.1)):
        net = AdaptiveFourierNeuralOperatorNet(**dict(kw, **extra))
        assert tuple(net(x).shape) == (1, 2, 24, 40)
        has_skip = any("skip_layer" in k for k in net.state_dict())
        assert has_skip == (extra.get("skip_fno", "linear") == "linear")
    with pytest.raises(NotImplementedError):
        AdaptiveFourierNeuralOperatorNet(**dict(kw, normalization_layer="batch_norm"))
    f = AFNO2D(8, num_blocks=2, hidden_size_factor=3)
    assert tuple(f.w1.shape) == (2, 4, 12, 2) and tuple(f.w2.shape) == (2, 12, 4, 2)
    with pytest.raises(AssertionError):
        AFNO2D(10, num_blocks=4)


def test_spec_block_mlp_on_cpu_against_float64_chain():
    from makani_amd import ops
    L, M, B, nb, bs, hb, lam = 5, 4, 2, 3, 4, 6, 0.3
    gen = torch.Generator().manual_seed(3)
    c = torch.complex(torch.randn(L, M, B * nb * bs, generator=gen), torch.randn(L, M, B * nb * bs, generator=gen))
    w1, w2 = 0.5 * torch.randn(nb, bs, hb, 2, generator=gen), 0.5 * torch.randn(nb, hb, bs, 2, generator=gen)
    g = torch.complex(torch.randn(L, M, B * nb * bs, generator=gen), torch.randn(L, M, B * nb * bs, generator=gen))
    leaves = [t.clone().requires_grad_(True) for t in (c, w1, w2)]
    y = ops.spec_block_mlp(leaves[0], leaves[1], leaves[2], B, nb, lam)
    y.backward(g)
    # the chain, block by block, in float64
    r = [c.to(torch.complex128).requires_grad_(True), w1.double().requires_grad_(True), w2.double().requires_grad_(True)]
    x = r[0].view(L, M, B, nb, bs)
    outs = []
    for k in range(nb):
        p1 = x[:, :, :, k, :] @ torch.view_as_complex(r[1])[k]
        h = torch.complex(torch.clamp(p1.real, min=0), torch.clamp(p1.imag, min=0))
        p2 = torch.view_as_real(h @ torch.view_as_complex(r[2])[k])
        outs.append(torch.view_as_complex(torch.where(p2 > lam, p2 - lam, torch.where(p2 < -lam, p2 + lam, torch.zeros_like(p2)))))
    yo = torch.stack(outs, dim=3).reshape(L, M, -1)
    yo.backward(g.to(torch.complex128))
    assert rel(torch.view_as_real(y), torch.view_as_real(yo)) <= BOUND
    for name, a, b in zip(("c", "w1", "w2"), leaves, r):
        ga, gb = (torch.view_as_real(t.grad) if t.grad.is_complex() else t.grad for t in (a, b))
        assert ga.shape == gb.shape and rel(ga, gb) <= BOUND, name


def test_unknown_knob_raises(ref, monkeypatch):
    monkeypatch.setenv("MK_AFNO", "bogus")
    with pytest.raises(ValueError, match="MK_AFNO"):
        build(ref, "afno")(ref["afno.x"])


def test_odd_block_size_and_odd_width_run_on_the_torch_path(monkeypatch):
    from makani_amd import ops
    from makani_amd.afnonet import AFNO2D
    monkeypatch.setenv("MK_AFNO", "hip")
    monkeypatch.setattr(ops, "spec_block_mlp", lambda *a, **k: pytest.fail("the fused path was taken"))
    for C, nb, H, W in ((9, 3, 6, 8), (8, 2, 6, 7)):
        f = AFNO2D(C, num_blocks=nb, sparsity_threshold=0.01)
        x = torch.randn(2, C, H, W, requires_grad=True)
        y = f(x)
        y.sum().backward()
        assert y.shape == x.shape and torch.isfinite(y).all() and x.grad is not None and f.w1.grad is not None


def test_launchers_validate_before_launching():
    """Code 1 and a message for null, misaligned, odd-sized and too large operands; nothing is launched (the pointers are never
    dereferenced).  The production shape needs a workspace of a whole number of panels; a contraction of one row group none."""
    from makani_amd import _lib
    lib = _lib.load()
    P = 4096
    assert lib.mk_spec_bdmlp_fwd(None, P, P, 8, 2, 4, 4, 0, 0.0, None) == 1
    assert lib.mk_spec_bdmlp_fwd(P + 8, P, P, 8, 2, 4, 4, 0, 0.0, None) == 1
    assert lib.mk_spec_bdmlp_fwd(P, P, P, 8, 2, 3, 4, 0, 0.0, None) == 1 and "even block sizes" in lib.mk_last_error().decode()
    assert lib.mk_spec_bdmlp_fwd(P, P, P, 8, 2, 4, 4, 1, 0.0, None) == 1               # act 1 is not a mode of this family
    assert lib.mk_spec_bdmlp_fwd(P, P, P, 8, 2, 4, 4, 3, -0.5, None) == 1
    assert lib.mk_spec_bdmlp_fwd(P, P, P, 8, 1 << 20, 64, 64, 0, 0.0, None) == 1 and "2^31" in lib.mk_last_error().decode()
    assert lib.mk_spec_bdmlp_fwd(P, P, P, 8, 1, 1 << 14, 1 << 14, 0, 0.0, None) == 1   # one panel of 2^31 bytes
    assert lib.mk_spec_bdmlp_dgrad(P, P, None, P, 8, 2, 4, 5, 0, None) == 1 and "even block sizes" in lib.mk_last_error().decode()
    assert lib.mk_spec_bdmlp_dgrad(P, P, None, P, 8, 2, 4, 4, 2, None) == 1            # mask mode without its operand
    assert lib.mk_spec_bdmlp_dgrad(P, P, P, P, 8, 2, 4, 4, 0, None) == 1
    assert lib.mk_spec_bdmlp_dgrad(P, P, P + 4, P, 8, 2, 4, 4, 2, None) == 1
    assert lib.mk_spec_bdmlp_wgrad(P, P, P, None, 4096, 2, 4, 4, None) == 1            # several row groups, no workspace
    assert lib.mk_spec_bdmlp_wgrad(P, P, P, None, 8, 2, 6, 3, None) == 1 and "even block sizes" in lib.mk_last_error().decode()
    assert lib.mk_spec_bdmlp_mask(P, P, P, 6, None) == 1 and "mk_spec_bdmlp_mask" in lib.mk_last_error().decode()
    assert lib.mk_spec_bdmlp_wgrad_workspace(8, 2, 4, 4) == 0
    nbytes = lib.mk_spec_bdmlp_wgrad_workspace(90 * 91, 8, 96, 96)
    assert nbytes > 0 and nbytes % (8 * 96 * 96 * 8) == 0


def test_block_mlp_raw_wrappers_have_no_cpu_fallback():
    from makani_amd import ops
    x, w = torch.zeros(4, 5, 8, dtype=torch.complex64), torch.zeros(2, 4, 4, dtype=torch.complex64)
    for call in (lambda: ops.spec_bdmlp_fwd_raw(x, w), lambda: ops.spec_bdmlp_dgrad_raw(x, w), lambda: ops.spec_bdmlp_wgrad_raw(x, x, 1, 2),
                 lambda: ops.spec_bdmlp_mask_raw(x, x)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_file_path_registration_like_model_registry():
    """model_registry.py:63-79: 'path/to/afnonet.py:Name' through spec_from_file_location, then instantiate."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("AdaptiveFourierNeuralOperatorNet", os.path.join(root, "makani_amd", "afnonet.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    net = module.AdaptiveFourierNeuralOperatorNet(**dict(NET_KW, num_layers=1))
    assert isinstance(net, torch.nn.Module) and tuple(net(torch.zeros(1, 3, 24, 40)).shape) == (1, 2, 24, 40)


# ---------------------------------------------------------------------------------------------------------------------
# misaligned pointers: refused by the host checks, with the message of the check (tests/capi_checks.py)
# ---------------------------------------------------------------------------------------------------------------------
_A = capi.A
MISALIGNED = [      # entry point, its arguments in front of the stream with one pointer moved off its alignment, the refusal
    ("mk_spec_bdmlp_mask", (_A, _A + 8, _A, 8), "operands must be 16-byte aligned"),
    ("mk_spec_bdmlp_wgrad", (_A, _A + 8, _A, _A, 4096, 2, 4, 4), "operands must be 16-byte aligned", "spec_bdmlp_check"),
    ("mk_spec_bdmlp_wgrad", (_A, _A, _A, _A + 8, 4096, 2, 4, 4), "the block weight gradient needs its 16-byte aligned workspace"),
]


@pytest.mark.parametrize("case", MISALIGNED, ids=capi.case_ids(MISALIGNED))
def test_misaligned_pointer_is_refused_before_any_launch(case):
    capi.assert_refused(*case)
