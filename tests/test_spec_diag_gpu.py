"""GPU tests of the diagonal filter on the private spectrum (``mk_spec_diag_fwd`` / ``_dgrad`` / ``_wgrad``, csrc/spec_diag.hip),
called through the C ABI: outputs between guard bands (``kernel_checks.guarded``), inputs between NaN bands
(``kernel_checks.poisoned``).

Truth is the reference's own formulation, ``einsum("bixy,ioxy->boxy")`` and its two adjoints, in complex128 on the unpacked
operands.  EVERY element is held to ``|y - ref| <= c * 2^-23 * mag`` (``kernel_checks.x3_elementwise``), ``mag`` the sum of the
absolute values of the real products that form the component (``absdot``) and ``c = n + 1`` with ``n`` the contraction length
(``cin`` forward, ``cout`` data gradient, ``batch`` weight gradient): a component is a chain of 2n fused multiply-adds, whose
worst-case error is ``2n u / (1 - 2n u) * mag`` with ``u = 2^-24``, i.e. ``n * 2^-23 * mag`` to first order; the 1 covers the
higher-order term.  Derived from the arithmetic, not fitted to the kernels.  Every test prints its worst ratio before it asserts.
Measured on an MI355X over the shapes below (records, not limits): forward 2.54, data gradient 2.66, weight gradient 2.18.

With ``dense = 0`` the entries of ``x`` / ``gy`` / ``w`` with global ``l < m`` are NaN: every checked output must be finite, the
guard sentinel must survive in those entries of ``y`` / ``gx`` and ``gw`` there must be bit-zero.
"""
import os

import numpy as np
import pytest
import torch

import kernel_checks as kc

pytestmark = pytest.mark.gpu

# (lloc, mloc, batch, cin, cout, l_off, m_off, dense)
SHAPES = {
    "odd_channels": (5, 5, 1, 3, 2, 0, 0, 0),          # rows 8-byte aligned only
    "shard_edge": (9, 7, 2, 5, 9, 3, 2, 0),            # a shard whose triangle edge crosses position runs; mloc no tile multiple
    "dense": (4, 9, 3, 8, 8, 0, 0, 1),
    "odd_batch": (6, 10, 5, 16, 24, 0, 0, 1),          # batch beyond the batch blocking (4): a second pass
    "many_outputs": (3, 130, 1, 2, 130, 0, 0, 1),      # more output channels than one pass of lanes holds, five runs per row
    "production": (33, 33, 1, 64, 64, 0, 0, 0),        # the production channel count over many runs; 36 MB of weight
    # the branches of the tile choice (sd_setup) the six above do not reach:
    "run_halved_for_lds": (2, 40, 2, 64, 48, 0, 0, 1),     # 32 positions do not fit the LDS budget: runs of 16
    "batch_stage_shrunk": (3, 6, 5, 300, 300, 1, 0, 0),    # runs of 8 still do not fit: the batch stage falls from 4 to 1
    "run_below_8": (2, 6, 1, 700, 600, 0, 0, 1),           # nor does one batch item: runs of 2
}
IDS = list(SHAPES)


def _valid(shape):
    lloc, mloc, _, _, _, l_off, m_off, dense = shape
    l = torch.arange(lloc).view(-1, 1) + l_off
    m = torch.arange(mloc).view(1, -1) + m_off
    return torch.ones(lloc, mloc, dtype=torch.bool) if dense else (l >= m)


def _crandn(g, *shape):
    return torch.complex(torch.randn(*shape, generator=g), torch.randn(*shape, generator=g))


_truth = {}


def truth(name):
    """Operands (public layout, CPU), complex128 results and magnitudes of one shape: computed once, shared, never modified."""
    if name not in _truth:
        lloc, mloc, B, I, O, l_off, m_off, dense = SHAPES[name]
        g = torch.Generator().manual_seed(17 + 1000 * lloc + mloc)
        x, w, gy = _crandn(g, B, I, lloc, mloc), _crandn(g, I, O, lloc, mloc), _crandn(g, B, O, lloc, mloc)
        valid = _valid(SHAPES[name])
        x64, w64, gy64 = (t.to(torch.complex128) * valid for t in (x, w, gy))
        _truth[name] = dict(
            x=x, w=w, gy=gy, valid=valid,
            y=torch.einsum("bixy,ioxy->boxy", x64, w64), y_mag=kc.absdot("bixy,ioxy->boxy", x64, w64),
            gx=torch.einsum("boxy,ioxy->bixy", gy64, w64.conj()), gx_mag=kc.absdot("boxy,ioxy->bixy", gy64, w64),
            gw=torch.einsum("bixy,boxy->ioxy", x64.conj(), gy64), gw_mag=kc.absdot("bixy,boxy->ioxy", x64, gy64))
    return _truth[name]


def _nan_triangle(t, valid):
    """``t [..., L, M]`` with NaN where the position holds no data."""
    return torch.where(valid, t, torch.full_like(t, complex(float("nan"), float("nan"))))


def _private(t):
    """public ``[B, C, L, M]`` -> private ``[L, M, B * C]``."""
    B, C, L, M = t.shape
    return t.permute(2, 3, 0, 1).reshape(L, M, B * C).contiguous()


def _public(t, B):
    """private ``[L, M, B * C]`` -> public ``[B, C, L, M]`` (a view)."""
    L, M, BC = t.shape
    return t.view(L, M, B, BC // B).permute(2, 3, 0, 1)


def _launch(name, a, b, out, shape):
    from makani_amd import _lib
    lloc, mloc, B, I, O, l_off, m_off, dense = shape
    rc = getattr(_lib.load(), name)(a.data_ptr(), b.data_ptr(), out.data_ptr(), lloc, mloc, B, I, O, l_off, m_off, dense,
                                    torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, name)


def run_kernels(t, shape, dev):
    """The three kernels on one shape's operands (NaN in the triangle, NaN bands around): guarded outputs and their checks."""
    lloc, mloc, B, I, O = shape[:5]
    v = t["valid"]
    x = kc.poisoned(_private(_nan_triangle(t["x"], v)), dev)
    gy = kc.poisoned(_private(_nan_triangle(t["gy"], v)), dev)
    w = kc.poisoned(_nan_triangle(t["w"], v), dev)
    y, y_chk = kc.guarded((lloc, mloc, B * O), torch.complex64, dev)
    gx, gx_chk = kc.guarded((lloc, mloc, B * I), torch.complex64, dev)
    gw, gw_chk = kc.guarded((I, O, lloc, mloc), torch.complex64, dev)
    _launch("mk_spec_diag_fwd", x, w, y, shape)
    _launch("mk_spec_diag_dgrad", gy, w, gx, shape)
    _launch("mk_spec_diag_wgrad", x, gy, gw, shape)
    torch.cuda.synchronize()
    y_chk("y"), gx_chk("gx"), gw_chk("gw")
    return y, gx, gw


_runs = {}


def run(name, dev):
    if name not in _runs:
        _runs[name] = tuple(o.cpu() for o in run_kernels(truth(name), SHAPES[name], dev))
    return _runs[name]


def _sentinel(t):
    return torch.full_like(t, kc.SENTINEL_C)


@pytest.mark.parametrize("name", IDS)
def test_every_element_within_the_fma_chain_bound(dev, name):
    """Forward, data gradient and weight gradient of every shape, every element; the triangle untouched (y, gx) or bit-zero (gw).
    Shapes beyond the issue's six, one per branch of the tile choice they do not reach: ``run_halved_for_lds`` (the run is
    halved from 32 because the LDS budget does not hold it), ``batch_stage_shrunk`` (the batch stage shrinks below the batch
    blocking), ``run_below_8`` (the run shrinks further after the batch stage reached 1).  The 8-byte weight path taken for a
    weight that is not 16-byte aligned has its own test below."""
    shape = SHAPES[name]
    B, I, O = shape[2:5]
    t = truth(name)
    v = t["valid"]
    y, gx, gw = run(name, dev)
    yp, gxp = _public(y, B), _public(gx, B)
    worst = {}
    worst["fwd"] = kc.x3_elementwise(yp[..., v], t["y"][..., v], t["y_mag"][..., v], c=I + 1, what=f"{name} forward")
    worst["dgrad"] = kc.x3_elementwise(gxp[..., v], t["gx"][..., v], t["gx_mag"][..., v], c=O + 1, what=f"{name} dgrad")
    worst["wgrad"] = kc.x3_elementwise(gw[..., v], t["gw"][..., v], t["gw_mag"][..., v], c=B + 1, what=f"{name} wgrad")
    print(f"[spec_diag] {name} {shape}: worst |err| / (2^-23 mag): " + "  ".join(f"{k}={r:.2f}" for k, r in worst.items()))
    if not bool(v.all()):
        assert torch.equal(yp[..., ~v], _sentinel(yp[..., ~v])), "y was written where global l < m"
        assert torch.equal(gxp[..., ~v], _sentinel(gxp[..., ~v])), "gx was written where global l < m"
        assert not bool(torch.view_as_real(gw[..., ~v]).contiguous().view(torch.int32).any()), "gw is not bit-zero where global l < m"


def test_reference_golden(dev, golden_dir):
    """Forward on the operands and the result recorded from the reference's ``_contract_diagonal`` (dense), the same bound."""
    z = np.load(os.path.join(golden_dir, "ref_contractions.npz"))
    x, w, want = (torch.from_numpy(z[k]) for k in ("x", "w_diagonal", "y_diagonal"))
    B, I, L, M = x.shape
    O = w.shape[1]
    shape = (L, M, B, I, O, 0, 0, 1)
    y, chk = kc.guarded((L, M, B * O), torch.complex64, dev)
    _launch("mk_spec_diag_fwd", kc.poisoned(_private(x), dev), kc.poisoned(w.contiguous(), dev), y, shape)
    torch.cuda.synchronize()
    chk("y")
    x64, w64 = x.to(torch.complex128), w.to(torch.complex128)
    mag = kc.absdot("bixy,ioxy->boxy", x64, w64)
    worst = kc.x3_elementwise(_public(y.cpu(), B), torch.einsum("bixy,ioxy->boxy", x64, w64), mag, c=I + 1, what="golden, complex128")
    to_recorded = kc.x3_elementwise(_public(y.cpu(), B), want.to(torch.complex128), mag, c=I + 1, what="golden, recorded")
    print(f"[spec_diag] golden: against complex128 {worst:.2f}, against the recorded complex64 result {to_recorded:.2f}")


def _shard(t, shape, l0, l1, m0, m1):
    """The operands and shape of the block [l0:l1, m0:m1] of a problem."""
    lloc, mloc, B, I, O, l_off, m_off, dense = shape
    sub = {k: t[k][..., l0:l1, m0:m1].contiguous() for k in ("x", "w", "gy", "valid")}
    return sub, (l1 - l0, m1 - m0, B, I, O, l_off + l0, m_off + m0, dense)


def _assert_shards_equal(full, shape, t, cuts, dev):
    for l0, l1, m0, m1 in cuts:
        sub, sshape = _shard(t, shape, l0, l1, m0, m1)
        y, gx, gw = (o.cpu() for o in run_kernels(sub, sshape, dev))
        # untouched entries hold the sentinel on both sides, so whole blocks compare
        assert torch.equal(y, full[0][l0:l1, m0:m1]), f"forward of shard {(l0, l1, m0, m1)} differs from the unsharded bits"
        assert torch.equal(gx, full[1][l0:l1, m0:m1]), f"dgrad of shard {(l0, l1, m0, m1)} differs from the unsharded bits"
        assert torch.equal(gw, full[2][..., l0:l1, m0:m1]), f"wgrad of shard {(l0, l1, m0, m1)} differs from the unsharded bits"


def test_shard_edge_is_bit_equal_to_its_slice_of_the_whole(dev):
    """``shard_edge`` is the block [3:12, 2:9] of a 12 x 9 problem without offsets: its results are the slices of that problem's, bit
    for bit (the operation is elementwise in (l, m))."""
    lloc, mloc, B, I, O, l_off, m_off, dense = SHAPES["shard_edge"]
    whole = (l_off + lloc, m_off + mloc, B, I, O, 0, 0, dense)
    g = torch.Generator().manual_seed(99)
    L, M = whole[:2]
    t = dict(x=_crandn(g, B, I, L, M), w=_crandn(g, I, O, L, M), gy=_crandn(g, B, O, L, M), valid=_valid(whole))
    full = tuple(o.cpu() for o in run_kernels(t, whole, dev))
    _assert_shards_equal(full, whole, t, [(l_off, L, m_off, M)], dev)


def test_two_by_two_cut_of_production_is_bit_equal(dev):
    t, shape = truth("production"), SHAPES["production"]
    cuts = [(l0, l1, m0, m1) for l0, l1 in ((0, 17), (17, 33)) for m0, m1 in ((0, 17), (17, 33))]
    _assert_shards_equal(run("production", dev), shape, t, cuts, dev)


def test_weight_aligned_to_8_bytes_only(dev):
    """An even ``mloc`` with ``w`` / ``gw`` on an 8-byte boundary takes the 8-byte weight path (the dispatch's other reason for it next
    to an odd ``mloc``): the bits of the 16-byte path, and nothing stored in front of ``gw``."""
    name = "odd_batch"
    shape = SHAPES[name]
    lloc, mloc, B, I, O = shape[:5]
    t = truth(name)
    x, gy = kc.poisoned(_private(t["x"]), dev), kc.poisoned(_private(t["gy"]), dev)
    w = kc.poisoned(torch.cat([torch.zeros(1, dtype=torch.complex64), t["w"].flatten()]), dev)[1:].view(I, O, lloc, mloc)
    assert w.data_ptr() % 16 == 8
    y, y_chk = kc.guarded((lloc, mloc, B * O), torch.complex64, dev)
    gx, gx_chk = kc.guarded((lloc, mloc, B * I), torch.complex64, dev)
    gw1, gw_chk = kc.guarded((I * O * lloc * mloc + 1,), torch.complex64, dev)
    gw = gw1[1:].view(I, O, lloc, mloc)
    _launch("mk_spec_diag_fwd", x, w, y, shape)
    _launch("mk_spec_diag_dgrad", gy, w, gx, shape)
    _launch("mk_spec_diag_wgrad", x, gy, gw, shape)
    torch.cuda.synchronize()
    y_chk("y"), gx_chk("gx"), gw_chk("gw")
    assert torch.equal(gw1[:1].cpu(), _sentinel(gw1[:1].cpu()))
    for got, want in zip((y, gx, gw), run(name, dev)):
        assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("name", ["shard_edge", "odd_batch"])
def test_two_runs_are_bit_equal(dev, name):
    a = run(name, dev)
    b = tuple(o.cpu() for o in run_kernels(truth(name), SHAPES[name], dev))
    for p, q in zip(a, b):
        assert torch.equal(p, q)


@pytest.mark.parametrize("name", ["shard_edge", "odd_batch"])
def test_graph_replay_gives_the_eager_bits(dev, name):
    """Forward + backward of ``ops.spec_diag`` captured with ``torch.cuda.graph`` and replayed on new operands equal the eager bits
    (where the spectrum holds data: the triangle of y / gx is unwritten memory)."""
    from makani_amd import ops
    shape = SHAPES[name]
    lloc, mloc, B, I, O, l_off, m_off, dense = shape
    t = truth(name)
    v = t["valid"].to(dev)
    x = _private(_nan_triangle(t["x"], t["valid"])).to(dev).requires_grad_(True)
    w = _nan_triangle(t["w"], t["valid"]).to(dev).requires_grad_(True)
    gy = _private(_nan_triangle(t["gy"], t["valid"])).to(dev)

    def step():
        y = ops.spec_diag(x, w, B, l_off, m_off, bool(dense))
        gx, gw = torch.autograd.grad(y, (x, w), gy)
        return y, gx, gw

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    with torch.no_grad():                   # new operands (scaled by powers of two: exact): the replay must compute anew
        x.mul_(0.5), w.mul_(-2.0), gy.mul_(4.0)
    graph.replay()
    torch.cuda.synchronize()
    eager = step()
    torch.cuda.synchronize()
    assert torch.equal(out[0][v], eager[0][v]) and torch.equal(out[1][v], eager[1][v]) and torch.equal(out[2], eager[2])
    # and the autograd function returns what the raw launches return: y = (x / 2)(-2 w), gx = (4 gy) conj(-2 w), gw = conj(x / 2)(4 gy)
    ref, vc = run(name, dev), t["valid"]
    assert torch.equal(-out[0].cpu()[vc], ref[0][vc]) and torch.equal(out[1].cpu()[vc] / -8, ref[1][vc])
    assert torch.equal(out[2].cpu() / 2, ref[2])
