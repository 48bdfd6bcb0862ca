"""The ViT modules on the MI355X with the attention product on the ``mk_attn_*`` kernels (``MK_ATTN=hip``).

The tolerance is not a stored number: the same module runs with ``MK_ATTN=torch`` under the same bf16 autocast, and the HIP
path's relative L2 error against the fp32 / float64 value must be at most twice the torch path's, tensor by tensor."""
import pytest
import torch

from test_vit_cpu import build, ref, rel, run, wanted      # noqa: F401  (``ref`` is the module-scoped fixture)

pytestmark = pytest.mark.gpu


class Calls:
    """Counts the launches of the forward kernel and records whether lse was asked for."""

    def __init__(self, monkeypatch):
        from makani_amd import ops
        self.packed, self.plain, self.lse = 0, 0, []
        orig_fwd, orig_p, orig_u = ops.attn_fwd_raw, ops._AttentionPacked.apply, ops._Attention.apply

        def fwd(q, k, v, o, lse, scale):
            self.lse.append(lse is not None)
            return orig_fwd(q, k, v, o, lse, scale)

        def packed(*a):
            self.packed += 1
            return orig_p(*a)

        def plain(*a):
            self.plain += 1
            return orig_u(*a)

        monkeypatch.setattr(ops, "attn_fwd_raw", fwd)
        monkeypatch.setattr(ops._AttentionPacked, "apply", packed)
        monkeypatch.setattr(ops._Attention, "apply", plain)


def test_recorded_net_under_bf16_autocast(dev, ref, monkeypatch):
    net = build(ref).to(dev)
    errs = {}
    calls = Calls(monkeypatch)
    for mode in ("hip", "torch"):
        monkeypatch.setenv("MK_ATTN", mode)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y, grads = run(ref, net, dev)
        errs[mode] = {"y": rel(y.float().cpu(), ref["y"])}
        errs[mode].update({n: rel(g.float().cpu(), wanted(ref, n)) for n, g in grads.items()})
        if mode == "hip":
            assert calls.packed == len(net.blocks) and calls.lse == [True] * len(net.blocks), "the HIP path did not run"
    assert calls.packed == len(net.blocks)
    for n in errs["hip"]:
        print(f"[vit] {n}: hip {errs['hip'][n]:.3e} torch {errs['torch'][n]:.3e}")
    for n in errs["hip"]:
        assert errs["hip"][n] <= 2 * errs["torch"][n], (n, errs["hip"][n], errs["torch"][n])


def _attention_case(dev, qk_norm, tokens=200, dim=128, heads=2):
    from makani_amd.vit import Attention
    torch.manual_seed(5)
    a = Attention(dim, num_heads=heads, qkv_bias=True, qk_norm=qk_norm)
    with torch.no_grad():
        a.qkv.weight.mul_(4.0)                       # scores with a standard deviation of order 1, not a mean
        for p in (a.qkv.bias, a.proj.bias):
            p.add_(0.1 * torch.randn_like(p))
    x = torch.randn(2, tokens, dim)
    g = torch.randn(2, tokens, dim)
    return a, x, g


def _fwd_bwd(a, x, g, autocast):
    a.zero_grad(set_to_none=True)
    x = x.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        y = a(x)
    y.backward(g.to(y.dtype))
    out = {"y": y.detach(), "x": x.grad}
    out.update({n: p.grad for n, p in a.named_parameters()})
    return out


def test_qk_norm_takes_the_unpacked_path(dev, monkeypatch):
    a, x, g = _attention_case(dev, qk_norm=True)
    # float64 on the CPU; copies, because moving the module moves its gradient tensors in place
    want = {n: t.clone() for n, t in _fwd_bwd(a.double(), x.double(), g.double(), False).items()}
    a = a.float().to(dev)
    calls = Calls(monkeypatch)
    errs = {}
    for mode in ("hip", "torch"):
        monkeypatch.setenv("MK_ATTN", mode)
        got = _fwd_bwd(a, x.to(dev), g.to(dev), True)
        errs[mode] = {n: rel(t.float().cpu(), want[n]) for n, t in got.items() if n != "k_norm.bias"}
        # a constant added to every key shifts all scores of a row alike and leaves the softmax unchanged: this gradient is
        # exactly zero (the float64 value is its own rounding noise), so the error is measured against the weight's next to it
        assert torch.linalg.norm(want["k_norm.bias"]) < 1e-10 * torch.linalg.norm(want["k_norm.weight"])
        errs[mode]["k_norm.bias"] = float(torch.linalg.norm(got["k_norm.bias"].double().cpu()) / torch.linalg.norm(want["k_norm.weight"]))
    assert (calls.plain, calls.packed) == (1, 0)
    for n in errs["hip"]:
        print(f"[vit] qk_norm {n}: hip {errs['hip'][n]:.3e} torch {errs['torch'][n]:.3e}")
        assert errs["hip"][n] <= 2 * errs["torch"][n], (n, errs["hip"][n], errs["torch"][n])


def test_grad_mode_off_stores_no_lse(dev, monkeypatch):
    monkeypatch.setenv("MK_ATTN", "hip")
    a, x, g = _attention_case(dev, qk_norm=False)
    a, x = a.to(dev).bfloat16(), x.to(dev).bfloat16()
    calls = Calls(monkeypatch)
    y1 = a(x)
    with torch.no_grad():
        y0 = a(x)
    a.requires_grad_(False)
    y2 = a(x)                                        # grad mode on, nothing requires a gradient
    assert calls.lse == [True, False, False] and calls.packed == 3
    assert torch.equal(y0, y1.detach()) and torch.equal(y2, y0)


def test_attention_module_in_a_graph(dev, monkeypatch):
    """Forward and backward of one ``Attention`` captured with ``torch.cuda.graph`` after warm-up on a side stream; the replay
    on new data is bit-equal to the eager run on the same data."""
    monkeypatch.setenv("MK_ATTN", "hip")
    a, x, g = _attention_case(dev, qk_norm=False)
    a = a.to(dev).bfloat16()
    xs = torch.zeros_like(x, device=dev, dtype=torch.bfloat16).requires_grad_(True)
    gs = g.to(dev).bfloat16()
    warm = torch.randn_like(xs)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.no_grad():
            xs.copy_(warm)
        for _ in range(3):
            a.zero_grad(set_to_none=True)
            xs.grad = None
            a(xs).backward(gs)
    torch.cuda.current_stream().wait_stream(side)
    a.zero_grad(set_to_none=True)
    xs.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ys = a(xs)
        ys.backward(gs)
    data = x.to(dev).bfloat16()
    with torch.no_grad():
        xs.copy_(data)
    graph.replay()
    torch.cuda.synchronize()
    got = {"y": ys.detach().clone(), "x": xs.grad.clone()}
    got.update({n: p.grad.clone() for n, p in a.named_parameters()})
    want = _fwd_bwd(a, data, gs, False)
    torch.cuda.synchronize()
    for n in want:
        assert torch.equal(got[n], want[n]), f"{n}: the replay differs from the eager run"
    assert float(got["y"].float().abs().max()) > 0
