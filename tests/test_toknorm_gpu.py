"""The trailing-axis layer norm kernels (csrc/toknorm.hip) on the MI355X: the C ABI between guard bands against the float64
reference and the bounds of toknorm_checks.py, the properties the header states (row subsets, determinism, gap columns, capture),
``ops.token_layer_norm`` under autograd, and the wiring of ViT and AFNO."""
import pytest
import torch

import kernel_checks as kc
import toknorm_checks as tc

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
NAN = float("nan")


def _code(dtype):
    return {F32: 0, BF16: 1}[dtype]


def _in(t, dev, pad=0, off=0):
    """``t [rows, L]`` on the device as rows of stride ``L + pad`` that start ``off`` elements into a buffer: everything around
    the elements -- the gap columns, the element in front, the bands -- is NaN."""
    if t is None:
        return None, 0
    rows, L = t.shape
    ld = L + pad
    flat = kc.poisoned(torch.full((rows * ld + off,), NAN, dtype=t.dtype), dev)
    v = flat[off:].view(rows, ld)[:, :L]
    v.copy_(t)
    return v, ld


def _vec(t, dev, off=0):
    if t is None:
        return None
    flat = kc.poisoned(torch.full((t.numel() + off,), NAN, dtype=t.dtype), dev)
    flat[off:].copy_(t)
    return flat[off:]


def _out(rows, L, dtype, dev, pad=0, off=0):
    """A sentinel-filled output with the same layout: (view of the elements, ld, check)."""
    ld = L + pad
    flat, bands = kc.guarded((rows * ld + off,), dtype, dev)
    v = flat[off:].view(rows, ld)

    def check(what):
        bands(what)
        assert bool((flat[:off] == kc.SENTINEL).all()), f"{what}: the element in front of the tensor was written"
        assert bool((v[:, L:] == kc.SENTINEL).all()), f"{what}: a gap column (L ... ld - 1) was written"

    return v[:, :L], ld, check


def _p(t):
    return None if t is None else t.data_ptr()


def _a3(t, ld):
    return (None, 0, 0) if t is None else (t.data_ptr(), _code(t.dtype), ld)


DEFAULTS = dict(x_dtype=F32, r_dtype=BF16, y_dtype=F32, y2=True, s_dtype=F32, gy_dtype=F32, gs_dtype=F32, w=True, b=True, pad=0, off=0,
                dist="n01", eps=1e-5, seed=0)


def run_case(dev, rows, L, inputs=None, sub=None, **opts):
    """Forward and backward through the C ABI.  Options: the dtypes (``r_dtype`` / ``y_dtype`` / ``s_dtype`` / ``gy_dtype`` /
    ``gs_dtype`` None: that tensor is absent; ``y2`` False: no bf16 copy), ``w`` / ``b`` False: NULL, ``pad``: ld = L + pad for
    every tensor, ``off``: every base pointer that many elements behind an aligned address.  Returns the inputs (CPU) and the
    results (device views).  ``sub = (a, b)``: the launch runs on rows a ... b - 1 of the same inputs."""
    from makani_amd import _lib
    o = dict(DEFAULTS, **opts)
    lib = _lib.load()
    t = tc.make_inputs(rows, L, o["dist"], o["seed"], o["x_dtype"], o["r_dtype"] or BF16) if inputs is None else inputs
    cut = (lambda v: v) if sub is None else (lambda v: v[sub[0]:sub[1]])
    n = rows if sub is None else sub[1] - sub[0]
    pad, off = o["pad"], o["off"]
    cpu = dict(x=cut(t["x"]), r=cut(t["r"]) if o["r_dtype"] else None, w=t["w"] if o["w"] else None, b=t["b"] if o["b"] else None,
               gy=cut(t["gy"]).to(o["gy_dtype"]) if o["gy_dtype"] else None, gy2=cut(t["gy2"]) if o["y2"] else None,
               gs=cut(t["gs"]).to(o["gs_dtype"]) if (o["gs_dtype"] and o["s_dtype"]) else None)
    x, x_ld = _in(cpu["x"], dev, pad, off)
    r, r_ld = _in(cpu["r"], dev, pad, off)
    w, b = _vec(cpu["w"], dev, off), _vec(cpu["b"], dev, off)
    y, y_ld, y_chk = _out(n, L, o["y_dtype"], dev, pad, off) if o["y_dtype"] else (None, 0, None)
    y2, y2_ld, y2_chk = _out(n, L, BF16, dev, pad, off) if o["y2"] else (None, 0, None)
    s, s_ld, s_chk = _out(n, L, o["s_dtype"], dev, pad, off) if o["s_dtype"] else (None, 0, None)
    stats, _, st_chk = _out(n, 2, F32, dev)
    what = f"({rows}, {L}) {opts}"
    _lib.check(lib.mk_token_layernorm_fwd(*_a3(x, x_ld), *_a3(r, r_ld), _p(w), _p(b), *_a3(y, y_ld), _p(y2), y2_ld, *_a3(s, s_ld),
                                          stats.data_ptr(), n, L, o["eps"], None), "mk_token_layernorm_fwd")
    torch.cuda.synchronize()
    for chk in (y_chk, y2_chk, s_chk, st_chk):
        if chk is not None:
            chk(f"fwd {what}")
    gy, gy_ld = _in(cpu["gy"], dev, pad, off)
    gy2, gy2_ld = _in(cpu["gy2"], dev, pad, off)
    gs, gs_ld = _in(cpu["gs"], dev, pad, off)
    gx, _, gx_chk = _out(n, L, o["x_dtype"], dev, pad, off)
    gr, _, gr_chk = _out(n, L, o["r_dtype"], dev, pad, off) if o["r_dtype"] else (None, 0, None)
    gwb, _, gwb_chk = _out(2, L, F32, dev)
    ws, ws_chk = kc.guarded((lib.mk_token_layernorm_workspace(n, L),), F32, dev, fill=NAN)      # need not be cleared: full of NaN
    _lib.check(lib.mk_token_layernorm_bwd(*_a3(x, x_ld), *_a3(r, r_ld), *_a3(gy, gy_ld), _p(gy2), gy2_ld, *_a3(gs, gs_ld), stats.data_ptr(),
                                          _p(w), gx.data_ptr(), _p(gr), ws.data_ptr(), gwb.data_ptr(), n, L, None),
               "mk_token_layernorm_bwd")
    torch.cuda.synchronize()
    for chk in (gx_chk, gr_chk, gwb_chk):
        if chk is not None:
            chk(f"bwd {what}")
    # the workspace is compared by its bytes only (NaN never equals NaN)
    ws_chk(f"bwd workspace {what}")
    return dict(cpu=cpu, opts=o, what=what, y=y, y2=y2, s=s, stats=stats, gx=gx, gr=gr, gw=gwb[0], gb=gwb[1])


def check_case(res):
    """Every result of ``run_case`` against the float64 reference; returns the worst ratios."""
    c, o, what = res["cpu"], res["opts"], res["what"]
    ref = tc.reference(c["x"], c["r"], c["w"], c["b"], o["eps"], c["gy"], c["gy2"], c["gs"] if c["gs"] is not None else torch.zeros(c["x"].shape))
    worst = tc.check_forward(ref, res["y"], res["y2"], res["stats"], what)
    if res["s"] is not None:
        want = (c["x"].float() if c["r"] is None else c["x"].float() + c["r"].float()).to(res["s"].dtype)
        assert torch.equal(res["s"].cpu(), want), f"{what}: s_out is not the fp32 sum rounded once"
    worst.update(tc.check_backward(ref, res["gx"], res["gr"], res["gw"], res["gb"], what))
    if res["gr"] is not None and res["gr"].dtype == res["gx"].dtype:
        assert torch.equal(res["gr"], res["gx"])
    return worst


# What a workgroup stages of a long row, as csrc/toknorm.hip sizes it: 160 KB of LDS less 64 bytes for the wave sums, the row
# padded to whole vectors of 8, 4 bytes per element forward (s) and 8 backward (s and g).  Longer rows are read again.
LDS_BYTES, LDS_FIXED = 160 * 1024, 64
FWD_LDS_MAX = (LDS_BYTES - LDS_FIXED) // 4 // 8 * 8          # 40 944
BWD_LDS_MAX = (LDS_BYTES - LDS_FIXED) // 8 // 8 * 8          # 20 472

# (rows, L, options): 1, 2 and 4 vectors per lane of a wavefront (L <= 512, <= 1024, <= 2048), a workgroup per row with the row in
# LDS and read again beyond, at the last staged and the first re-read length of either direction; vectors and single elements;
# more rows than persistent workgroups in the backward (4096 rows per pass of wavefronts, 256 of workgroups)
SHAPES = [
    (5, 1, {}), (3, 7, {}), (37, 48, {}), (130, 384, {}), (10, 768, {}), (9, 1030, {}), (5, 2048, {}), (3, 16200, {}),
    (6, 2056, {}),                                   # just beyond a wavefront's registers
    (2, BWD_LDS_MAX, {}),                            # the longest row staged both ways
    (2, BWD_LDS_MAX + 8, {}),                        # forward staged, backward re-read
    (2, 40904, {}),                                  # the same, well inside
    (2, FWD_LDS_MAX, {}),                            # the longest row the forward stages
    (2, FWD_LDS_MAX + 8, {}),                        # re-read both ways
    (2, FWD_LDS_MAX + 5, {"dist": "n53"}),           # the same by single elements
    (37, 48, {"pad": 3}), (130, 384, {"pad": 3}), (4, 2056, {"pad": 3}),
    (130, 384, {"pad": 8}),                          # gap columns on the vector path
    (37, 48, {"off": 1}), (130, 384, {"off": 1}), (4, 2056, {"off": 1}), (3, 16200, {"off": 1, "pad": 3}),
    (4200, 7, {}), (300, 2056, {}),                  # more rows than workspace slots
    (130, 384, {"dist": "n53"}), (130, 384, {"dist": "n50"}), (3, 16200, {"dist": "n50"}),
]
COMBOS = [
    dict(x_dtype=BF16, r_dtype=BF16, y_dtype=BF16, y2=False, s_dtype=BF16, gy_dtype=BF16, gs_dtype=BF16),
    dict(x_dtype=BF16, r_dtype=F32, y_dtype=F32, s_dtype=F32, gy_dtype=BF16),
    dict(x_dtype=F32, r_dtype=F32, y_dtype=BF16, s_dtype=None, gy_dtype=F32),
    dict(r_dtype=None, y2=False, s_dtype=None),                      # the plain norm
    dict(r_dtype=None, x_dtype=BF16, y_dtype=BF16, y2=False, s_dtype=None, gy_dtype=BF16),
    dict(y_dtype=None, gy_dtype=None, s_dtype=None),                 # only the bf16 copy, only its gradient
    dict(y2=False, gy_dtype=None),                                   # only the gradient of the sum
    dict(w=False), dict(b=False), dict(w=False, b=False, s_dtype=BF16, gs_dtype=BF16),
]


@pytest.mark.parametrize("rows,L,opts", SHAPES, ids=[f"{r}x{l}-{'-'.join(f'{k}{v}' for k, v in o.items()) or 'plain'}" for r, l, o in SHAPES])
def test_shapes_against_float64(dev, rows, L, opts):
    worst = check_case(run_case(dev, rows, L, **opts))
    print(f"[toknorm] ({rows}, {L}) {opts}: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))


@pytest.mark.parametrize("combo", range(len(COMBOS)))
@pytest.mark.parametrize("rows,L", [(37, 48), (130, 384), (3, 2056)])
def test_dtypes_and_outputs_against_float64(dev, rows, L, combo):
    worst = check_case(run_case(dev, rows, L, seed=1 + combo, **COMBOS[combo]))
    print(f"[toknorm] ({rows}, {L}) combo {combo}: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))


@pytest.mark.parametrize("L", [384, 2056])
def test_constant_rows(dev, L):
    """var = 0: y = bias exactly (2.5 k L is an fp32 number for every partial sum, so the mean is exact), everything finite."""
    t = tc.make_inputs(6, L)
    t["x"] = (2.5 * torch.arange(1, 7, dtype=F32))[:, None].expand(6, L).contiguous()
    res = run_case(dev, 6, L, inputs=t, r_dtype=None, s_dtype=None)
    assert torch.equal(res["y"].cpu(), t["b"].expand(6, L)), "y is not the bias on constant rows"
    assert torch.equal(res["stats"][:, 0].cpu(), t["x"][:, 0])
    for k in ("y2", "stats", "gx", "gw", "gb"):
        assert bool(torch.isfinite(res[k].float()).all()), k
    check_case(res)


def test_one_element_rows(dev):
    """L = 1: the norm's own gradient vanishes, gx = gs exactly."""
    res = run_case(dev, 5, 1)
    assert torch.equal(res["gx"].cpu(), res["cpu"]["gs"]) and torch.equal(res["y"].cpu(), res["cpu"]["b"].expand(5, 1))


@pytest.mark.parametrize("rows,L,a,b", [(37, 48, 5, 22), (130, 384, 3, 70), (9, 1030, 1, 8), (6, 2056, 1, 4), (3, 16200, 1, 3),
                                            (3, FWD_LDS_MAX + 8, 1, 3)])
def test_row_subsets_carry_the_bits_of_the_full_launch(dev, rows, L, a, b):
    """A launch on rows a ... b - 1 alone, and the full launch through the single-element path (every pointer one element off,
    ld = L + 5), against the full launch through 16-byte vectors."""
    t = tc.make_inputs(rows, L, "n53", 3)
    full = run_case(dev, rows, L, inputs=t)
    part = run_case(dev, rows, L, inputs=t, sub=(a, b))
    for k in ("y", "y2", "s", "gx", "gr", "stats"):
        assert torch.equal(part[k], full[k][a:b]), f"{k}: rows {a}:{b} differ from the slice of the full launch"
    shifted = run_case(dev, rows, L, inputs=t, off=1, pad=5)
    for k in ("y", "y2", "s", "gx", "gr", "stats", "gw", "gb"):
        assert torch.equal(shifted[k], full[k]), f"{k}: the single-element path differs from the vector path"


@pytest.mark.parametrize("rows,L", [(4200, 48), (130, 384), (300, 2056)])
def test_two_runs_give_the_same_bits(dev, rows, L):
    t = tc.make_inputs(rows, L, "n01", 4)
    one, two = run_case(dev, rows, L, inputs=t), run_case(dev, rows, L, inputs=t)
    for k in ("y", "y2", "s", "stats", "gx", "gr", "gw", "gb"):
        assert torch.equal(one[k], two[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# ops.token_layer_norm
# ---------------------------------------------------------------------------------------------------------------------
def _op_case(dev, lead, shape, seed=0, x_dtype=F32, r_dtype=BF16):
    L = 1
    for s in shape:
        L *= s
    rows = 1
    for s in lead:
        rows *= s
    t = tc.make_inputs(rows, L, "n53", seed, x_dtype, r_dtype)
    full = lambda v: v.view(*lead, *shape).to(dev)
    return t, dict(x=full(t["x"]).requires_grad_(True), r=full(t["r"]).requires_grad_(True), w=t["w"].view(shape).to(dev).requires_grad_(True),
                   b=t["b"].view(shape).to(dev).requires_grad_(True), gy=full(t["gy"]), gy2=full(t["gy2"]), gs=full(t["gs"]))


@pytest.mark.parametrize("lead,shape", [((2, 50), (384,)), ((2, 3), (6, 10)), ((4,), (90, 180))])
def test_autograd_against_float64(dev, lead, shape):
    from makani_amd import ops
    t, d = _op_case(dev, lead, shape)
    assert ops.token_layer_norm_supported(d["x"], shape, d["w"], d["b"])
    y, y2, s = ops.token_layer_norm(d["x"], d["w"], d["b"], 1e-5, d["r"], None, True, True)
    assert (y.dtype, y2.dtype, s.dtype) == (F32, BF16, F32) and y.shape == d["x"].shape
    torch.autograd.backward([y, y2, s], [d["gy"], d["gy2"], d["gs"]])
    ref = tc.reference(t["x"], t["r"], t["w"], t["b"], 1e-5, t["gy"], t["gy2"], t["gs"])
    flat = lambda v: v.detach().reshape(t["x"].shape)
    worst = tc.check_forward(ref, flat(y), flat(y2), what="op")
    assert d["x"].grad.dtype == F32 and d["r"].grad.dtype == BF16
    worst.update(tc.check_backward(ref, flat(d["x"].grad), flat(d["r"].grad), d["w"].grad.reshape(-1), d["b"].grad.reshape(-1), "op"))
    print(f"[toknorm] op {lead} {shape}: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    # one output, no residual, x's dtype; a strided batch of rows is taken as it is
    big = torch.randn(7, 400, device=dev).bfloat16()
    xs = big[:, 8:392].detach().requires_grad_(True)
    w1 = torch.randn(384, device=dev)
    y = ops.token_layer_norm(xs, w1, None, 1e-5)
    assert torch.is_tensor(y) and y.dtype == BF16
    y.backward(torch.ones_like(y))
    ref = tc.reference(xs.detach().cpu(), None, w1.cpu(), None, 1e-5, torch.ones(7, 384))
    tc.check_forward(ref, y.detach(), what="strided op")
    tc.check_backward(ref, xs.grad, what="strided op")
    with torch.autocast("cuda", dtype=BF16):
        assert ops.token_layer_norm(xs, w1, None, 1e-5).dtype == F32      # what torch's autocast gives layer_norm
    assert not ops.token_layer_norm_supported(xs.half(), (384,)) and not ops.token_layer_norm_supported(xs, (384,), w1.double())
    assert not ops.token_layer_norm_supported(big.t(), (7,))


@pytest.mark.parametrize("shape", [(384,), (6, 10)])
def test_module_without_parameters_normalises_over_all_its_axes(dev, monkeypatch, shape):
    """``elementwise_affine=False``: nothing but ``normalized_shape`` says how many trailing axes the norm spans."""
    from makani_amd.layers import LayerNorm
    mod = LayerNorm(shape, eps=1e-6, elementwise_affine=False).to(dev)
    twin = torch.nn.LayerNorm(shape, eps=1e-6, elementwise_affine=False).to(dev)
    L = 1
    for n in shape:
        L *= n
    t = tc.make_inputs(8, L, "n53", 5)
    x = t["x"].view(2, 4, *shape).to(dev).requires_grad_(True)
    g = t["gy"].view(2, 4, *shape).to(dev)
    calls = Calls(monkeypatch)
    monkeypatch.setenv("MK_TOKEN_NORM", "hip")
    y = mod(x)
    y.backward(g)
    assert (calls.fwd, calls.bwd, calls.torch) == (1, 1, 0)
    ref = tc.reference(t["x"], None, None, None, 1e-6, t["gy"])
    tc.check_forward(ref, y.detach().reshape(8, L), what=f"module {shape}")
    tc.check_backward(ref, x.grad.reshape(8, L), what=f"module {shape}")
    want = twin(x.detach())
    tc.check_forward(ref, want.reshape(8, L), what=f"nn.LayerNorm {shape}")      # the torch module means the same thing
    (ya,) = mod.forward_add(x.detach())
    assert torch.equal(ya, y.detach())


def test_captured_forward_and_backward_replay_to_the_eager_bits(dev):
    from makani_amd import ops
    t, d = _op_case(dev, (40,), (384,), seed=2)
    xs, rs = torch.zeros_like(d["x"]).requires_grad_(True), torch.zeros_like(d["r"]).requires_grad_(True)
    w, b = d["w"], d["b"]

    def step():
        for p in (xs, rs, w, b):
            p.grad = None
        y, y2 = ops.token_layer_norm(xs, w, b, 1e-5, rs, None, True, False)
        torch.autograd.backward([y, y2], [d["gy"], d["gy2"]])
        return y, y2

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    for p in (xs, rs, w, b):
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ys = step()
    with torch.no_grad():
        xs.copy_(d["x"])
        rs.copy_(d["r"])
    graph.replay()
    torch.cuda.synchronize()
    got = [v.detach().clone() for v in ys] + [p.grad.clone() for p in (xs, rs, w, b)]
    want = [v.detach().clone() for v in step()] + [p.grad.clone() for p in (xs, rs, w, b)]
    torch.cuda.synchronize()
    for i, (g, v) in enumerate(zip(got, want)):
        assert torch.equal(g, v), f"tensor {i}: the replay differs from the eager run"
    assert float(got[0].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# wiring
# ---------------------------------------------------------------------------------------------------------------------
class Calls:
    """Counts the launches of the forward and the backward kernel and the calls of torch's layer norm."""

    def __init__(self, monkeypatch):
        from makani_amd import ops
        self.fwd = self.bwd = self.torch = 0
        orig_f, orig_b, orig_t = ops.token_layernorm_fwd_raw, ops.token_layernorm_bwd_raw, torch.nn.functional.layer_norm

        def fwd(*a, **k):
            self.fwd += 1
            return orig_f(*a, **k)

        def bwd(*a, **k):
            self.bwd += 1
            return orig_b(*a, **k)

        def tln(*a, **k):
            self.torch += 1
            return orig_t(*a, **k)

        monkeypatch.setattr(ops, "token_layernorm_fwd_raw", fwd)
        monkeypatch.setattr(ops, "token_layernorm_bwd_raw", bwd)
        monkeypatch.setattr(torch.nn.functional, "layer_norm", tln)


def _rel(a, b):
    """Relative L2 error; a reference that is exactly zero (a filter whose soft-shrink passes nothing has no weight gradient)
    asks for exactly zero."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    num, den = float(torch.linalg.norm(a - b)), float(torch.linalg.norm(b))
    assert num == num, "NaN in a result"
    return num / den if den > 0 else (0.0 if num == 0 else float("inf"))


def _fwd_bwd(mod, x, g, autocast):
    mod.zero_grad(set_to_none=True)
    x = x.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=BF16, enabled=autocast):
        y = mod(x)
    y.backward(g.to(y.dtype))
    out = {"y": y.detach(), "x": x.grad}
    out.update({n: p.grad for n, p in mod.named_parameters()})
    return out


def _hip_against_torch(mod, x, g, dev, monkeypatch, autocast, tag, ref_dtype=torch.float64):
    """The module under ``MK_TOKEN_NORM=hip`` and ``=torch`` against its run on the CPU in ``ref_dtype`` without autocast: the HIP
    path's relative L2 error may be at most twice the torch path's, tensor by tensor (the method of tests/test_vit_gpu.py, whose
    reference is an fp32 recording: under bf16 autocast both paths are four orders of magnitude further from either reference
    than fp32 is from float64).  Returns the launch counts of the HIP run."""
    want = {n: v.clone() for n, v in _fwd_bwd(mod.to(ref_dtype), x.to(ref_dtype), g.to(ref_dtype), False).items()}
    mod = mod.float().to(dev)
    calls = Calls(monkeypatch)
    errs, counts = {}, None
    for mode in ("hip", "torch"):
        monkeypatch.setenv("MK_TOKEN_NORM", mode)
        before = (calls.fwd, calls.bwd, calls.torch)
        got = _fwd_bwd(mod, x.to(dev), g.to(dev), autocast)
        errs[mode] = {n: _rel(v.float(), want[n]) for n, v in got.items()}
        if mode == "hip":
            counts = (calls.fwd - before[0], calls.bwd - before[1], calls.torch - before[2])
    for n in errs["hip"]:
        print(f"[toknorm] {tag} {n}: hip {errs['hip'][n]:.3e} torch {errs['torch'][n]:.3e}")
    for n in errs["hip"]:
        assert errs["hip"][n] <= 2 * errs["torch"][n], (n, errs["hip"][n], errs["torch"][n])
    return counts


def _block():
    from makani_amd.vit import Block
    torch.manual_seed(7)
    blk = Block(128, 2, qkv_bias=True)
    with torch.no_grad():
        blk.attn.qkv.weight.mul_(4.0)
        for n in (blk.norm1, blk.norm2):
            n.weight.add_(0.2 * torch.randn_like(n.weight))
            n.bias.add_(0.2 * torch.randn_like(n.bias))
    return blk, torch.randn(1, 200, 128), torch.randn(1, 200, 128)


def test_vit_block_takes_the_fused_path_under_autocast(dev, monkeypatch):
    blk, x, g = _block()
    counts = _hip_against_torch(blk, x, g, dev, monkeypatch, True, "block")
    assert counts == (2, 2, 0), f"(forward launches, backward launches, torch layer_norm calls) = {counts}"


def test_vit_block_without_autocast(dev, monkeypatch):
    """fp32 tokens: one output per norm in the tokens' dtype, two launches each way.  Both paths are fp32 throughout, so their
    errors against float64 are rounding noise of the same order and are not ranked against each other: each stays under 1e-5, two
    orders above fp32 rounding through a dozen operations and five below what a wrong operand gives."""
    blk, x, g = _block()
    want = {n: v.clone() for n, v in _fwd_bwd(blk.double(), x.double(), g.double(), False).items()}
    blk = blk.float().to(dev)
    calls = Calls(monkeypatch)
    monkeypatch.setenv("MK_TOKEN_NORM", "hip")
    got = _fwd_bwd(blk, x.to(dev), g.to(dev), False)
    assert (calls.fwd, calls.bwd, calls.torch) == (2, 2, 0)
    assert got["y"].dtype == F32
    for n, v in got.items():
        assert _rel(v, want[n]) <= 1e-5, (n, _rel(v, want[n]))


def test_afno_layer_norm_runs_on_the_kernels(dev, monkeypatch):
    from makani_amd.afnonet import AdaptiveFourierNeuralOperatorNet
    torch.manual_seed(8)
    net = AdaptiveFourierNeuralOperatorNet(inp_shape=(64, 128), patch_size=(4, 4), inp_chans=3, out_chans=2, embed_dim=16, num_layers=2,
                                           num_blocks=4, normalization_layer="layer_norm", verbose=False)
    assert (net.h, net.w) == (16, 32)
    with torch.no_grad():
        for blk in net.blocks:
            for n in (blk.norm1, blk.norm2):
                n.weight.add_(0.2 * torch.randn_like(n.weight))
                n.bias.add_(0.2 * torch.randn_like(n.bias))
    x, g = torch.randn(2, 3, 64, 128), torch.randn(2, 2, 64, 128)
    # the reference in fp32: the filter's complex einsum does not take float64 weights next to the transforms' complex64
    counts = _hip_against_torch(net, x, g, dev, monkeypatch, True, "afno", ref_dtype=F32)
    assert counts == (4, 4, 0), f"(forward launches, backward launches, torch layer_norm calls) = {counts}"
