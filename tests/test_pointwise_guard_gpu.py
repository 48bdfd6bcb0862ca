"""The instance norm and the streaming helpers of csrc/pointwise.hip on the MI355X through the C ABI: outputs between sentinel
bands, inputs between NaN bands, EVERY element of y, gx, the saved (mean, rstd), the row sums and the parameter gradients bounded
against float64 with the units and constants of pointwise_checks.py -- the kernels' documented one-pass arithmetic, whose rstd
unit grows as (mean / std)^2.  rows = B C = 2 x 3 (so ``row % C`` matters), P around one and two workgroups of 8192 elements.
The fp64 sums are atomics in arrival order: nothing here asserts bit equality between runs."""
import pytest
import torch

import kernel_checks as kc
import pointwise_checks as pc

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
F64 = torch.float64
ROWS, NCH = 6, 3
LENGTHS = [8, 8184, 8192, 8200, 16392]
NAME = {F32: "f32", BF16: "bf16"}

lengths = pytest.mark.parametrize("P", LENGTHS)
dtypes = pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
fused = pytest.mark.parametrize("fuse", [False, True], ids=["plain", "gelu"])
dists = pytest.mark.parametrize("dist", ["n53", "n501"])


def _in(t, dev):
    return None if t is None else kc.poisoned(t, dev)


def _p(t):
    return None if t is None else t.data_ptr()


def _code(dtype):
    return {F32: 0, BF16: 1}[dtype]


def _lib_and_stream():
    from makani_amd import _lib, ops
    return _lib, _lib.load(), ops._stream()


def _report(what, worst, limits):
    print(f"[pointwise-guard] {what}: " + " ".join(f"{k} {v / limits[k]:.2f}" for k, v in worst.items()) + " of their limits")


def _check_stats(ref, stats, what):
    return dict(mean=pc.check(stats[:, 0], ref["mean"], ref["unit_mean"], pc.C["mean"], f"{what} mean"),
                rstd=pc.check(stats[:, 1], ref["rstd"], ref["unit_rstd"], pc.C["rstd"], f"{what} rstd"))


def _close(got, want, what):
    """fp64 sums of exactly known fp32 partials: 1e-12 relative, whatever order the atomics arrived in."""
    got, want = got.double().cpu(), want.double().cpu()
    assert bool(((got - want).abs() <= 1e-12 * want.abs()).all()), f"{what}: {got.tolist()} against {want.tolist()}"


def _forward(dev, t, fuse, rows=ROWS, nch=NCH, phase=0, ws=None, count=None):
    """``mk_instnorm_fwd`` (phase 0) or ``_fwd_ex`` on ``t["x"][:rows]``; returns the device tensors."""
    _lib, lib, st = _lib_and_stream()
    x, w, b = _in(t["x"][:rows].contiguous(), dev), _in(t["w"], dev), _in(t["b"], dev)
    P = x.shape[1]
    y, y_chk = kc.guarded((rows, P), x.dtype, dev)
    stats, st_chk = kc.guarded((rows, 2), F32, dev)
    if ws is None:
        ws, ws_chk = kc.guarded((rows, 2), F64, dev)
    else:
        ws, ws_chk = _in(ws, dev), None
    if phase == 0:
        rc = lib.mk_instnorm_fwd(x.data_ptr(), _p(w), _p(b), y.data_ptr(), stats.data_ptr(), ws.data_ptr(), _code(x.dtype), rows, nch, P,
                                 pc.EPS, int(fuse), st)
    else:
        rc = lib.mk_instnorm_fwd_ex(x.data_ptr(), _p(w), _p(b), y.data_ptr(), stats.data_ptr(), ws.data_ptr(), _code(x.dtype), rows, nch, P,
                                    count, pc.EPS, int(fuse), phase, st)
    _lib.check(rc, "mk_instnorm_fwd")
    torch.cuda.synchronize()
    for chk, name in ((y_chk, "y"), (st_chk, "stats"), (ws_chk, "workspace")):
        if chk is not None:
            chk(f"fwd {name}")
    if phase == 1:
        assert bool((y == kc.SENTINEL).all()) and bool((stats == kc.SENTINEL).all()), "phase 1 wrote more than the sums"
    return dict(x=x, w=w, b=b, y=y, stats=stats, ws=ws)


def _backward(dev, t, f, fuse, rows=ROWS, nch=NCH, phase=0, ws=None, count=None, wb=False):
    _lib, lib, st = _lib_and_stream()
    x = f["x"]
    P = x.shape[1]
    gy = _in(t["gy"][:rows].contiguous(), dev)
    stats = _in(f["stats"].cpu(), dev)
    gx, gx_chk = kc.guarded((rows, P), x.dtype, dev)
    gwb, gwb_chk = kc.guarded((2, nch), F32, dev) if wb else (None, None)
    if ws is None:
        ws, ws_chk = kc.guarded((rows, 2), F64, dev)
    else:
        ws, ws_chk = _in(ws, dev), None
    common = (x.data_ptr(), gy.data_ptr(), stats.data_ptr(), _p(f["w"]), _p(f["b"]), gx.data_ptr(), ws.data_ptr())
    if wb:
        rc = lib.mk_instnorm_bwd_wb(*common, gwb.data_ptr(), _code(x.dtype), nch, P, int(fuse), st)
    elif phase == 0:
        rc = lib.mk_instnorm_bwd(*common, _code(x.dtype), rows, nch, P, int(fuse), st)
    else:
        rc = lib.mk_instnorm_bwd_ex(*common, _code(x.dtype), rows, nch, P, count, int(fuse), phase, st)
    _lib.check(rc, "mk_instnorm_bwd")
    torch.cuda.synchronize()
    for chk, name in ((gx_chk, "gx"), (gwb_chk, "gwb"), (ws_chk, "workspace")):
        if chk is not None:
            chk(f"bwd {name}")
    if phase == 1:
        assert bool((gx == kc.SENTINEL).all()), "phase 1 wrote more than the sums"
    return dict(gx=gx, ws=ws, gwb=gwb)


def _check_bsums(ref, ws, what):
    return dict(gb=pc.check(ws[:, 0], ref["bsums"][:, 0], ref["unit_bsums"][:, 0], pc.C["gb"], f"{what} sum g"),
                gw=pc.check(ws[:, 1], ref["bsums"][:, 1], ref["unit_bsums"][:, 1], pc.C["gw"], f"{what} sum g xh"))


@lengths
@dtypes
@fused
@dists
def test_instnorm_forward_and_backward(dev, P, dtype, fuse, dist):
    t = pc.make_inputs(ROWS, P, NCH, dist, 0, dtype)
    what = f"instnorm ({ROWS}, {P}) {NAME[dtype]} {'gelu ' if fuse else ''}{dist}"
    ref = pc.instnorm_reference(t["x"], t["w"], t["b"], NCH, pc.EPS, t["gy"], fuse)
    f = _forward(dev, t, fuse)
    worst = _check_stats(ref, f["stats"], what)
    worst["y"] = pc.check(f["y"], ref["y"], ref["unit_y"], pc.C["y"], f"{what} y")
    xf = t["x"].float()
    _close(f["ws"][:, 0], pc.row_sums(xf), f"{what} sum x")
    _close(f["ws"][:, 1], pc.row_sums(xf, xf), f"{what} sum x^2")
    g = _backward(dev, t, f, fuse)
    worst["gx"] = pc.check(g["gx"], ref["gx"], ref["unit_gx"], pc.C["gx"], f"{what} gx")
    worst.update(_check_bsums(ref, g["ws"], what))
    if not fuse:      # the plain sums are exactly known on the saved stats
        s = f["stats"].cpu()
        xh = (xf - s[:, :1]) * s[:, 1:]
        _close(g["ws"][:, 0], pc.row_sums(t["gy"].float()), f"{what} sum g")
        _close(g["ws"][:, 1], pc.row_sums(t["gy"].float(), xh), f"{what} sum g xh")
    _report(what, worst, pc.C)


@lengths
@dtypes
@fused
def test_instnorm_backward_with_parameter_gradients(dev, P, dtype, fuse):
    """``mk_instnorm_bwd_wb``: one sample, rows = C; the ``[2][C]`` parameter gradients are the row sums."""
    t = pc.make_inputs(ROWS, P, NCH, "n53", 1, dtype)
    what = f"instnorm_bwd_wb ({NCH}, {P}) {NAME[dtype]} {'gelu' if fuse else ''}"
    ref = pc.instnorm_reference(t["x"][:NCH], t["w"], t["b"], NCH, pc.EPS, t["gy"][:NCH], fuse)
    f = _forward(dev, t, fuse, rows=NCH)
    g = _backward(dev, t, f, fuse, rows=NCH, wb=True)
    worst = dict(gx=pc.check(g["gx"], ref["gx"], ref["unit_gx"], pc.C["gx"], f"{what} gx"),
                 gw=pc.check(g["gwb"][0], ref["gw"], ref["unit_gw"], pc.C["gw"], f"{what} gw"),
                 gb=pc.check(g["gwb"][1], ref["gb"], ref["unit_gb"], pc.C["gb"], f"{what} gb"))
    _report(what, worst, pc.C)


@pytest.mark.parametrize("P", [p for p in LENGTHS if p >= 16])
@dtypes
@fused
@dists
def test_instnorm_phases_on_a_row_sharded_field(dev, P, dtype, fuse, dist):
    """Phase 1 on either part of every row, the workspaces added in torch, phase 2 with ``count`` = the full P: the bounds of the
    unsharded reference."""
    t = pc.make_inputs(ROWS, P, NCH, dist, 2, dtype)
    what = f"sharded instnorm ({ROWS}, {P}) {NAME[dtype]} {'gelu ' if fuse else ''}{dist}"
    ref = pc.instnorm_reference(t["x"], t["w"], t["b"], NCH, pc.EPS, t["gy"], fuse)
    h = P // 2 // 8 * 8
    parts = [dict(t, x=t["x"][:, :h], gy=t["gy"][:, :h]), dict(t, x=t["x"][:, h:], gy=t["gy"][:, h:])]
    sums = sum(_forward(dev, q, fuse, phase=1, count=P)["ws"].cpu() for q in parts)
    fs = [_forward(dev, q, fuse, phase=2, ws=sums, count=P) for q in parts]
    assert torch.equal(fs[0]["stats"], fs[1]["stats"])
    worst = _check_stats(ref, fs[0]["stats"], what)
    worst["y"] = pc.check(torch.cat([f["y"] for f in fs], 1), ref["y"], ref["unit_y"], pc.C["y"], f"{what} y")
    bsums = sum(_backward(dev, q, f, fuse, phase=1, count=P)["ws"].cpu() for q, f in zip(parts, fs))
    worst.update(_check_bsums(ref, bsums, what))
    gs = [_backward(dev, q, f, fuse, phase=2, ws=bsums, count=P) for q, f in zip(parts, fs)]
    worst["gx"] = pc.check(torch.cat([g["gx"] for g in gs], 1), ref["gx"], ref["unit_gx"], pc.C["gx"], f"{what} gx")
    _report(what, worst, pc.C)


@lengths
@dtypes
@dists
def test_instnorm_coeffs(dev, P, dtype, dist):
    """The norm as a per-row affine map from the device's own row sums: stats and (sc, sh) against float64."""
    _lib, lib, st = _lib_and_stream()
    t = pc.make_inputs(ROWS, P, NCH, dist, 3, dtype)
    what = f"instnorm_coeffs ({ROWS}, {P}) {NAME[dtype]} {dist}"
    ref, _ = pc.reference(t["x"], t["w"], t["b"], NCH)
    f = _forward(dev, t, False, phase=1, count=P)
    sums, w, b = _in(f["ws"].cpu(), dev), f["w"], f["b"]
    stats, st_chk = kc.guarded((ROWS, 2), F32, dev)
    affine, af_chk = kc.guarded((ROWS, 2), F32, dev)
    _lib.check(lib.mk_instnorm_coeffs(sums.data_ptr(), _p(w), _p(b), stats.data_ptr(), affine.data_ptr(), ROWS, NCH, P, pc.EPS, st),
               "mk_instnorm_coeffs")
    torch.cuda.synchronize()
    st_chk(f"{what} stats")
    af_chk(f"{what} affine")
    worst = _check_stats(ref, stats, what)
    worst["sc"] = pc.check(affine[:, 0], ref["sc"], ref["unit_sc"], pc.C["sc"], f"{what} sc")
    worst["sh"] = pc.check(affine[:, 1], ref["sh"], ref["unit_sh"], pc.C["sh"], f"{what} sh")
    _report(what, worst, pc.C)


@lengths
@dtypes
def test_affine_add(dev, P, dtype):
    _lib, lib, st = _lib_and_stream()
    t = pc.make_inputs(ROWS, P, NCH, "n53", 4, dtype)
    aff = torch.stack([t["w"][torch.arange(ROWS) % NCH], t["b"][torch.arange(ROWS) % NCH]], 1).contiguous()
    want, unit = pc.affine_add_reference(t["r"], t["gy"], aff)
    r, z, a = _in(t["r"], dev), _in(t["gy"], dev), _in(aff, dev)
    y, y_chk = kc.guarded((ROWS, P), dtype, dev)
    _lib.check(lib.mk_affine_add(r.data_ptr(), z.data_ptr(), a.data_ptr(), y.data_ptr(), _code(dtype), ROWS, P, st), "mk_affine_add")
    torch.cuda.synchronize()
    y_chk("affine_add y")
    what = f"affine_add ({ROWS}, {P}) {NAME[dtype]}"
    _report(what, dict(affine=pc.check(y, want, unit, pc.C["affine"], what)), pc.C)


@lengths
@dtypes
def test_bias_gelu(dev, P, dtype):
    _lib, lib, st = _lib_and_stream()
    t = pc.make_inputs(ROWS, P, NCH, "n53", 5, dtype)
    pre = t["r"]                                                           # pre-activations N(0, 1)
    what = f"bias_gelu ({ROWS}, {P}) {NAME[dtype]}"
    x, bias, gy = _in(pre, dev), _in(t["b"], dev), _in(t["gy"], dev)
    y, y_chk = kc.guarded((ROWS, P), dtype, dev)
    _lib.check(lib.mk_bias_gelu_fwd(x.data_ptr(), bias.data_ptr(), y.data_ptr(), _code(dtype), ROWS, NCH, P, st), "mk_bias_gelu_fwd")
    torch.cuda.synchronize()
    y_chk(f"{what} y")
    want, unit = pc.bias_gelu_reference(pre, t["b"], NCH)
    worst = dict(bg_y=pc.check(y, want, unit, pc.C["bg_y"], f"{what} y"))
    gx, gx_chk = kc.guarded((ROWS, P), dtype, dev)
    gbias, gb_chk = kc.guarded((NCH,), F32, dev)
    gbias.zero_()                                                          # the kernel adds into it
    _lib.check(lib.mk_bias_gelu_bwd(x.data_ptr(), bias.data_ptr(), gy.data_ptr(), gx.data_ptr(), gbias.data_ptr(), _code(dtype), ROWS, NCH, P,
                                    st), "mk_bias_gelu_bwd")
    torch.cuda.synchronize()
    gx_chk(f"{what} gx")
    gb_chk(f"{what} gbias")
    want, unit, gb64, unit_gb = pc.bias_gelu_reference(pre, t["b"], NCH, t["gy"])
    worst["bg_gx"] = pc.check(gx, want, unit, pc.C["bg_gx"], f"{what} gx")
    # the fp32 atomics: the slack in units of u, so that ``check`` takes it
    worst["bg_gb"] = pc.check(gbias, gb64, unit_gb + pc.gbias_slack(want, NCH, P) / (pc.U * pc.C["bg_gb"]), pc.C["bg_gb"], f"{what} gbias")
    _report(what, worst, pc.C)
