"""CPU tests of the channel layer norm: the C ABI is exported and bound, and ``DistributedLayerNorm`` on the CPU is still the
reference's formulation (transpose -> nn.LayerNorm -> transpose), bit for bit.  No kernel launches here."""
import torch
import torch.nn as nn
import torch.nn.functional as F

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
