"""CPU tests of the channel layer norm: the C ABI is exported and bound, and ``DistributedLayerNorm`` on the CPU is still the
reference's formulation (transpose -> nn.LayerNorm -> transpose), bit for bit; the constants of chnorm_checks.py against its
emulation of the kernels' arithmetic.  No kernel launches here."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import capi_checks as capi
import chnorm_checks as cc

from makani_amd import _lib, ops
from makani_amd.layer_norm import DistributedLayerNorm

SYMBOLS = ("mk_chan_layernorm_fwd", "mk_chan_layernorm_bwd", "mk_chan_layernorm_workspace")


def test_symbols_exported_and_bound():
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    # one workspace slot of [2][C] floats per backward workgroup, never empty for a valid shape, zero for a bad one
    assert lib.mk_chan_layernorm_workspace(1, 384, 721 * 1440) >= 2 * 384
    assert lib.mk_chan_layernorm_workspace(2, 5, 15) >= 2 * 5
    assert lib.mk_chan_layernorm_workspace(1, 0, 15) == 0


def test_entry_points_validate_before_launching():
    lib = _lib.load()
    p = 4096      # non-null, aligned, never dereferenced: validation returns before any launch
    assert lib.mk_chan_layernorm_fwd(None, 0, p, p, p, 0, p, 1, 8, 16, 1e-5, 0, None) == 1
    assert lib.mk_chan_layernorm_fwd(p, 2, p, p, p, 0, p, 1, 8, 16, 1e-5, 0, None) == 1
    assert lib.mk_chan_layernorm_fwd(p, 0, p, p, p, 0, p, 1, 0, 16, 1e-5, 0, None) == 1
    assert lib.mk_chan_layernorm_bwd(p, 0, p, 0, None, p, p, p, p, p, 1, 8, 16, 0, None) == 1
    assert lib.mk_chan_layernorm_bwd(p, 0, p, 0, p, p, p, p, None, p, 1, 8, 16, 0, None) == 1      # gwb without workspace
    assert b"mk_chan_layernorm_bwd" in lib.mk_last_error()


def test_not_supported_on_cpu():
    assert not ops.channel_layer_norm_supported(torch.zeros(1, 8, 4, 6))
    assert not ops.channel_layer_norm_supported(torch.zeros(1, 8, 4, 6, dtype=torch.bfloat16))


def _reference(m, x):
    return torch.transpose(m.norm(torch.transpose(x, 1, 3)), 1, 3).contiguous()


def test_cpu_forward_is_the_reference_formulation():
    torch.manual_seed(0)
    m = DistributedLayerNorm(8, eps=1e-6)
    with torch.no_grad():
        m.norm.weight.copy_(torch.randn(8))
        m.norm.bias.copy_(torch.randn(8))
    x = torch.randn(2, 8, 5, 7) * 3 + 5
    ref = _reference(m, x)
    assert torch.equal(m(x), ref)
    assert torch.equal(m._forward_torch(x), ref)
    assert torch.equal(m(x, fuse_gelu=True), F.gelu(ref))
    assert m(x).dtype == torch.float32 and m(x).is_contiguous()
    # gradients flow through the torch path as before
    xg = x.clone().requires_grad_(True)
    m(xg, fuse_gelu=True).sum().backward()
    assert xg.grad is not None and m.norm.weight.grad is not None and m.norm.bias.grad is not None


def test_state_dict_and_sharing_annotations():
    m = DistributedLayerNorm(8, eps=1e-6)
    assert list(m.state_dict().keys()) == ["norm.weight", "norm.bias"]
    assert isinstance(m.norm, nn.LayerNorm) and m.norm.eps == 1e-6
    for p in (m.norm.weight, m.norm.bias):
        assert p.is_shared_mp == ["model"] and p.sharded_dims_mp == [None]


def test_optional_parameters_construct_and_run():
    x = torch.randn(1, 8, 3, 4)
    m = DistributedLayerNorm(8, elementwise_affine=False)
    assert list(m.state_dict().keys()) == []
    assert torch.equal(m(x), _reference(m, x))
    m = DistributedLayerNorm(8, bias=False)
    assert list(m.state_dict().keys()) == ["norm.weight"]
    assert m.norm.weight.is_shared_mp == ["model"] and m.norm.bias is None
    assert torch.equal(m(x, fuse_gelu=True), F.gelu(_reference(m, x)))


def test_emulation_stays_within_half_of_each_constant():
    worst = cc.emulation_worst()
    print("[chnorm] emulation worst ratios: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    recorded = dict(y=cc.EMU_WORST_Y, gx=cc.EMU_WORST_GX, gw=cc.EMU_WORST_GW, gb=cc.EMU_WORST_GB, stat=cc.EMU_WORST_STAT)
    limits = dict(y=cc.C_Y, gx=cc.C_GX, gw=cc.C_GW, gb=cc.C_GB, stat=cc.C_STAT)
    for k, v in worst.items():
        assert v <= limits[k] / 2, (k, v, limits[k])
        assert v <= recorded[k] * 1.02 + 0.01, f"{k}: the emulation reaches {v:.3f}, the module records {recorded[k]}"
    assert any(-(-P // 32) * B >= 3 * grid for B, _, P, grid in cc.EMU_SHAPES), "no shape with 3 tiles per workgroup"
    for act in (cc.F32, cc.BF16):
        d = cc.dgelu_abs_error(act)
        assert d <= cc.EMU_DGELU[act] * 1.02 and cc.DGELU[act] >= 2 * cc.EMU_DGELU[act], (act, d)


def test_a_defect_is_far_outside_the_bounds():
    """What the constants are there to catch, each at least 20 times its limit: a workgroup that drops the channel sums of its
    second tile, a pixel whose (mean, rstd) are its neighbour's, a one-pass variance at N(50, 0.1^2)."""
    B, C, P, grid = 3, 4, 2250, 64                                        # 213 tiles of 32 pixels on 64 workgroups
    for fuse in (False, True):
        t = cc.make_inputs(B, C, P, "n53", 0)
        ref = cc.reference(t["x"], t["w"], t["b"], 1e-6, t["gy"], fuse)
        good = cc.ratios(cc.emulate(t["x"], t["w"], t["b"], 1e-6, t["gy"], fuse, grid=grid), ref)
        assert good["gw"] <= cc.C_GW / 2 and good["gb"] <= cc.C_GB / 2 and good["y"] <= cc.C_Y / 2
        bad = cc.ratios(cc.emulate(t["x"], t["w"], t["b"], 1e-6, t["gy"], fuse, grid=grid, defect="drop_tile"), ref)
        assert bad["gw"] > 20 * cc.C_GW and bad["gb"] > 20 * cc.C_GB, bad
        bad = cc.ratios(cc.emulate(t["x"], t["w"], t["b"], 1e-6, t["gy"], fuse, grid=grid, defect="neighbour_stats"), ref)
        assert bad["y"] > 20 * cc.C_Y and bad["gx"] > 20 * cc.C_GX and bad["stat"] > 20 * cc.C_STAT, bad
        t = cc.make_inputs(1, 73, 36, "n50", 0)
        ref = cc.reference(t["x"], t["w"], t["b"], 1e-6, t["gy"], fuse)
        bad = cc.ratios(cc.emulate(t["x"], t["w"], t["b"], 1e-6, t["gy"], fuse, defect="one_pass"), ref)
        assert bad["y"] > 20 * cc.C_Y and bad["gx"] > 20 * cc.C_GX and bad["stat"] > 20 * cc.C_STAT, bad


def test_rows_and_field_are_inverse():
    x = torch.arange(2 * 3 * 5.0).view(2, 3, 5)
    r = cc.rows(x)
    assert r.shape == (10, 3) and torch.equal(r[7], x[1, :, 2]) and torch.equal(cc.field(r, 2), x)


# ---------------------------------------------------------------------------------------------------------------------
# misaligned pointers: refused by the host checks, with the message of the check (tests/capi_checks.py)
# ---------------------------------------------------------------------------------------------------------------------
_A = capi.A
MISALIGNED = [      # entry point, its arguments in front of the stream with one pointer moved off its alignment, the refusal
    ("mk_chan_layernorm_fwd", (_A + 2, 0, _A, _A, _A, 0, _A, 1, 8, 16, 1e-5, 0), "field not aligned to its element"),
    ("mk_chan_layernorm_fwd", (_A, 0, _A, _A, _A, 1, _A + 4, 1, 8, 16, 1e-5, 0), "fp32 stream not aligned"),
    ("mk_chan_layernorm_bwd", (_A, 0, _A + 1, 1, _A, _A, _A, _A, _A, _A, 1, 8, 16, 0), "field not aligned to its element"),
    ("mk_chan_layernorm_bwd", (_A, 0, _A, 0, _A, _A, _A, _A, _A, _A + 2, 1, 8, 16, 0), "fp32 stream not aligned"),
]


@pytest.mark.parametrize("case", MISALIGNED, ids=capi.case_ids(MISALIGNED))
def test_misaligned_pointer_is_refused_before_any_launch(case):
    capi.assert_refused(*case)
