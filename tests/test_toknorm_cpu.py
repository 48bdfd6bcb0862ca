"""The trailing-axis layer norm (csrc/toknorm.hip, ``ops.token_layer_norm``, ``layers.LayerNorm``) without a GPU: the
constants of toknorm_checks.py against its emulation, the module on the CPU against ``nn.LayerNorm``, the ``state_dict`` keys
of the networks that took the module, the knob and the C ABI's validation."""
import pytest
import torch
import torch.nn as nn

import toknorm_checks as tc

import capi_checks as capi


def test_emulation_stays_within_half_of_each_constant():
    worst = tc.emulation_worst()
    print("[toknorm] emulation worst ratios: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    recorded = dict(y=tc.EMU_WORST_Y, gx=tc.EMU_WORST_GX, gw=tc.EMU_WORST_GW, gb=tc.EMU_WORST_GB, stat=tc.EMU_WORST_STAT)
    limits = dict(y=tc.C_Y, gx=tc.C_GX, gw=tc.C_GW, gb=tc.C_GB, stat=tc.C_STAT)
    for k, v in worst.items():
        assert v <= limits[k] / 2, (k, v, limits[k])
        assert v <= recorded[k] * 1.02 + 0.01, f"{k}: the emulation reaches {v:.3f}, the module records {recorded[k]}"


def test_a_defect_is_far_outside_the_bounds():
    """What the constants are there to catch: a one-pass variance, a dropped residual, a gradient without its projection."""
    t = tc.make_inputs(40, 384, "n50", 0)
    ref = tc.reference(t["x"], t["r"], t["w"], t["b"], 1e-5, t["gy"], t["gy2"], t["gs"])
    plain = tc.reference(t["x"], None, t["w"], t["b"], 1e-5)
    s = t["x"]
    mean = s.mean(1, keepdim=True)
    var = (s * s).mean(1, keepdim=True) - mean * mean                      # E[s^2] - mean^2 in fp32 at mean / std = 500
    y = t["w"] * (s - mean) / torch.sqrt(var.clamp_min(0) + 1e-5) + t["b"]
    assert float(tc.excess_ratio(y, plain["y"], plain["unit_y"]).max()) > 20 * tc.C_Y
    emu = tc.emulate(t["x"], None, t["w"], t["b"], 1e-5)
    assert float(tc.excess_ratio(emu["y"], ref["y"], ref["unit_y"]).max()) > 1000 * tc.C_Y
    emu = tc.emulate(t["x"], t["r"], t["w"], t["b"], 1e-5, t["gy"], t["gy2"], None)
    assert float(tc.excess_ratio(emu["gx"], ref["gx"], ref["unit_gx"]).max()) > 1000 * tc.C_GX


@pytest.mark.parametrize("shape,normalized", [((3, 5, 48), 48), ((2, 4, 6, 10), (6, 10))])
def test_module_on_cpu_is_nn_layernorm(shape, normalized, monkeypatch):
    from makani_amd.layers import LayerNorm
    torch.manual_seed(1)
    a, b = LayerNorm(normalized, eps=1e-6), nn.LayerNorm(normalized, eps=1e-6)
    with torch.no_grad():
        a.weight.add_(0.3 * torch.randn_like(a.weight))
        a.bias.add_(0.3 * torch.randn_like(a.bias))
    assert list(a.state_dict()) == list(b.state_dict()) == ["weight", "bias"]
    b.load_state_dict(a.state_dict(), strict=True)
    x = torch.randn(*shape)
    for mode in ("hip", "torch", None):
        if mode is None:
            monkeypatch.delenv("MK_TOKEN_NORM", raising=False)
        else:
            monkeypatch.setenv("MK_TOKEN_NORM", mode)
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        ya, yb = a(xa), b(xb)
        assert torch.equal(ya, yb)
        ya.square().sum().backward()
        yb.square().sum().backward()
        assert torch.equal(xa.grad, xb.grad) and torch.equal(a.weight.grad, b.weight.grad) and torch.equal(a.bias.grad, b.bias.grad)
        a.zero_grad(), b.zero_grad()
        r = torch.randn(*shape)
        y, y2, s = a.forward_add(x, r, lowp=True, want_sum=True)
        assert torch.equal(s, x + r) and torch.equal(y, b(x + r)) and torch.equal(y2, y.bfloat16())
        (y,) = a.forward_add(x)
        assert torch.equal(y, b(x))


def test_module_without_parameters_on_cpu(monkeypatch):
    from makani_amd.layers import LayerNorm
    monkeypatch.setenv("MK_TOKEN_NORM", "hip")
    a, b = LayerNorm((6, 10), elementwise_affine=False), nn.LayerNorm((6, 10), elementwise_affine=False)
    x = torch.randn(2, 4, 6, 10)
    assert torch.equal(a(x), b(x)) and torch.equal(a.forward_add(x)[0], b(x)) and list(a.state_dict()) == []


def test_bad_knob_raises(monkeypatch):
    from makani_amd import ops
    from makani_amd.layers import LayerNorm
    monkeypatch.setenv("MK_TOKEN_NORM", "fast")
    with pytest.raises(ValueError, match="MK_TOKEN_NORM"):
        ops.token_norm_hip()
    with pytest.raises(ValueError, match="MK_TOKEN_NORM"):
        LayerNorm(8)(torch.zeros(2, 8))
    monkeypatch.setenv("MK_TOKEN_NORM", "torch")
    assert ops.token_norm_hip() is False
    monkeypatch.setenv("MK_TOKEN_NORM", "hip")
    assert ops.token_norm_hip() is True
    assert ops.TOKEN_NORM_DEFAULT in ("hip", "torch")


def test_supported_declines_what_the_kernels_do_not_take():
    from makani_amd import ops
    x = torch.zeros(4, 8)
    assert not ops.token_layer_norm_supported(x, (8,))                     # a CPU tensor
    assert not ops.token_layer_norm_supported(x, (4,))
    with pytest.raises(RuntimeError, match="no fallback"):
        ops.token_layer_norm(x, None, None, 1e-5)


def test_networks_keep_their_state_dict_keys():
    """ViT and AFNO (``layer_norm``) hold ``layers.LayerNorm`` where they held ``nn.LayerNorm``: the keys are those of the old
    modules, and a state dict of the old modules loads with ``strict=True``."""
    from makani_amd.afnonet import AdaptiveFourierNeuralOperatorNet
    from makani_amd.layers import LayerNorm
    from makani_amd.vit import VisionTransformer
    vit = VisionTransformer(inp_shape=[21, 40], patch_size=(7, 8), inp_chans=3, out_chans=2, embed_dim=64, depth=2, num_heads=2,
                            mlp_ratio=1.0, qkv_bias=True)
    afno = AdaptiveFourierNeuralOperatorNet(inp_shape=(24, 40), patch_size=(4, 4), inp_chans=3, out_chans=2, embed_dim=16, num_layers=2,
                                            num_blocks=4, normalization_layer="layer_norm", verbose=False)
    for net, norms in ((vit, ["blocks.0.norm1", "blocks.1.norm2", "norm"]), (afno, ["blocks.0.norm1", "blocks.1.norm2"])):
        mods = dict(net.named_modules())
        old = {}
        for name in norms:
            assert type(mods[name]) is LayerNorm, name
        for name, m in mods.items():                                       # the parameters an nn.LayerNorm in its place would hold
            if type(m) is LayerNorm:
                twin = nn.LayerNorm(m.normalized_shape, eps=m.eps)
                old.update({f"{name}.{k}": v + 0.25 for k, v in twin.state_dict().items()})
        state = net.state_dict()
        assert set(old) <= set(state) and all(k.endswith((".weight", ".bias")) for k in old)
        assert not any("normalized" in k or "hip" in k for k in state)
        net.load_state_dict({**state, **old}, strict=True)
        for k, v in old.items():
            assert torch.equal(net.state_dict()[k], v)
    assert afno.blocks[0].norm1.normalized_shape == (6, 10) and afno.blocks[0].norm1.eps == 1e-6
    a = vit.blocks[0].attn
    assert isinstance(a.q_norm, nn.Identity)


def test_qk_norm_stays_a_torch_module():
    from makani_amd.layers import LayerNorm
    from makani_amd.vit import Block
    b = Block(32, 2, qkv_bias=True)
    assert type(b.norm1) is LayerNorm and type(b.norm2) is LayerNorm
    from makani_amd.vit import Attention
    a = Attention(32, num_heads=2, qk_norm=True)
    assert type(a.q_norm) is nn.LayerNorm and type(a.k_norm) is nn.LayerNorm


def test_symbols_have_signatures_and_validate():
    from makani_amd import _lib
    lib = _lib.load()
    for n in ("mk_token_layernorm_fwd", "mk_token_layernorm_bwd", "mk_token_layernorm_workspace"):
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    assert lib.mk_token_layernorm_workspace(18540, 384) >= 2 * 384
    assert lib.mk_token_layernorm_workspace(768, 16200) >= 2 * 16200
    assert lib.mk_token_layernorm_workspace(0, 8) == 0
    p = 4096      # non-null and aligned, never dereferenced: validation returns before any launch

    def fwd(x=p, xd=0, xld=8, r=None, rd=0, rld=8, y=p, yd=0, yld=8, y2=None, rows=2, L=8, eps=1e-5):
        return lib.mk_token_layernorm_fwd(x, xd, xld, r, rd, rld, p, p, y, yd, yld, y2, 8, None, 0, 8, p, rows, L, eps, None)

    def bwd(x=p, xd=0, r=None, gr=None, gy=p, stats=p, ws=p, gwb=p, rows=2, L=8, gyld=8):
        return lib.mk_token_layernorm_bwd(x, xd, 8, r, 0, 8, gy, 0, gyld, None, 8, None, 0, 8, stats, p, p, gr, ws, gwb, rows, L, None)

    assert fwd(x=None) == 1 and fwd(y=None) == 1 and fwd(xd=2) == 1 and fwd(L=0) == 1 and fwd(rows=0) == 1
    assert fwd(xld=7) == 1 and fwd(yld=4) == 1 and fwd(eps=-1.0) == 1 and fwd(r=p, rd=3) == 1 and fwd(x=p + 2) == 1
    assert b"mk_token_layernorm_fwd" in lib.mk_last_error()
    assert bwd(stats=None) == 1 and bwd(ws=None) == 1 and bwd(gr=p) == 1 and bwd(gyld=7) == 1 and bwd(xd=5) == 1
    assert b"mk_token_layernorm_bwd" in lib.mk_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# misaligned pointers: refused by the host checks, with the message of the check (tests/capi_checks.py)
# ---------------------------------------------------------------------------------------------------------------------
_A = capi.A
MISALIGNED = [      # entry point, its arguments in front of the stream with one pointer moved off its alignment, the refusal
    ("mk_token_layernorm_bwd", (_A, 0, 8, None, 0, 8, _A + 2, 0, 8, None, 8, None, 0, 8, _A, _A, _A, None, _A, _A, 2, 8), "tensor not aligned to its element"),
    ("mk_token_layernorm_bwd", (_A, 0, 8, None, 0, 8, _A, 0, 8, None, 8, None, 0, 8, _A + 2, _A, _A, None, _A, _A, 2, 8), "fp32 stream not aligned"),
    ("mk_token_layernorm_fwd", (_A, 0, 8, None, 0, 8, _A, _A + 2, _A, 0, 8, None, 8, None, 0, 8, _A, 2, 8, 1e-5), "fp32 stream not aligned"),
]


@pytest.mark.parametrize("case", MISALIGNED, ids=capi.case_ids(MISALIGNED))
def test_misaligned_pointer_is_refused_before_any_launch(case):
    capi.assert_refused(*case)
