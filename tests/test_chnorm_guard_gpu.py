"""The channel layer norm kernels (csrc/chnorm.hip) on the MI355X through the C ABI: every output between sentinel bands, every
input between NaN bands, the workspace at exactly ``mk_chan_layernorm_workspace`` floats, and EVERY element of y, gx, gw, gb and
of the saved (mean, rstd) bounded against float64 with the units and constants of chnorm_checks.py.  The shapes are the ones at
which the kernels take another path: below one tile, a one-vector tail, one channel per row group and one more, the element path
chosen by a pointer, the on-chip limits of either direction and the first width beyond them, the persistent loop of the backward
(workgroups with 2 and 3 tiles, sums in LDS and in the workspace slot), the forward's stride beyond 2^20 tiles, no parameters.
Each test prints its worst ratios as fractions of their limits; DESIGN.md section 17 records them."""
import pytest
import torch

import chnorm_checks as cc
import kernel_checks as kc

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
NAN = float("nan")
EPS = 1e-6
PAIRS = [(F32, F32), (BF16, BF16), (BF16, F32), (F32, BF16)]      # (x dtype, y / gy dtype): backward tiles of 32, 64, 32, 32 pixels
NAME = {F32: "f32", BF16: "bf16"}

# the launcher's own numbers (csrc/chnorm.hip)
LDS_MAX, K_RG, K_LANES, FWD_GRID, BWD_GRID, MIN_TP = 160 * 1024, 64, 8, 1 << 20, 1024, 32


def _size(dtype):
    return torch.empty((), dtype=dtype).element_size()


def _acc_floats(C):
    return (2 * C + 3) & ~3


def fwd_plan(B, C, P, xd):
    """(tiles, workgroups, tile staged in LDS) of the forward launch."""
    tp = K_LANES * 16 // _size(xd)
    ntiles = -(-P // tp) * B
    fixed = (K_RG * tp + 2 * tp) * 4
    return ntiles, min(ntiles, FWD_GRID), fixed + C * tp * _size(xd) <= LDS_MAX


def bwd_plan(B, C, P, xd, gd):
    """(tiles, workgroups, tiles and channel sums in LDS) of the backward launch."""
    tp = cc.bwd_tile_px(xd, gd)
    ntiles = -(-P // tp) * B
    fixed = (2 * K_RG * tp + 4 * tp) * 4
    return ntiles, min(ntiles, BWD_GRID), fixed + 4 * _acc_floats(C) + C * tp * (_size(xd) + _size(gd)) <= LDS_MAX


def fwd_limit(xd):
    """The largest C whose forward tile is staged."""
    return max(C for C in range(1, 4096) if fwd_plan(1, C, 40, xd)[2])


def bwd_limit(xd, gd):
    return max(C for C in range(1, 4096) if bwd_plan(1, C, 40, xd, gd)[2])


def _in(t, dev, off=0):
    """``t`` on the device between NaN bands, ``off`` elements behind a 16-byte boundary (the elements in front are NaN too)."""
    if t is None:
        return None
    flat = kc.poisoned(torch.full((t.numel() + off,), NAN, dtype=t.dtype), dev)
    v = flat[off:].view(t.shape)
    v.copy_(t)
    return v


def _out(shape, dtype, dev, off=0, fill=None):
    """A sentinel-filled output between bands, ``off`` elements behind a 16-byte boundary: (view, check)."""
    n = 1
    for s in shape:
        n *= s
    flat, bands = kc.guarded((n + off,), dtype, dev, fill=fill)

    def check(what):
        bands(what)
        assert bool((flat[:off] == kc.SENTINEL).all()), f"{what}: the element in front of the tensor was written"

    return flat[off:].view(shape), check


def _p(t):
    return None if t is None else t.data_ptr()


def _code(dtype):
    return {F32: 0, BF16: 1}[dtype]


def forward(dev, t, gd, fuse, off_x=0, off_out=0):
    from makani_amd import _lib, ops
    lib = _lib.load()
    B, C, P = t["x"].shape
    x, w, b = _in(t["x"], dev, off_x), _in(t["w"], dev), _in(t["b"], dev)
    y, y_chk = _out((B, C, P), gd, dev, off_out)
    stats, st_chk = _out((B * P, 2), F32, dev)
    _lib.check(lib.mk_chan_layernorm_fwd(x.data_ptr(), _code(x.dtype), _p(w), _p(b), y.data_ptr(), _code(gd), stats.data_ptr(), B, C, P,
                                         EPS, int(fuse), ops._stream()), "mk_chan_layernorm_fwd")
    torch.cuda.synchronize()
    y_chk("fwd y")
    st_chk("fwd stats")
    return dict(x=x, w=w, b=b, y=y, stats=stats)


def backward(dev, t, f, fuse, off_out=0):
    """One backward launch into fresh buffers, on the device inputs of ``forward`` and a poisoned copy of its stats."""
    from makani_amd import _lib, ops
    lib = _lib.load()
    B, C, P = t["x"].shape
    x = f["x"]
    gy = _in(t["gy"], dev)
    stats = _in(f["stats"].cpu(), dev)
    gx, gx_chk = _out((B, C, P), x.dtype, dev, off_out)
    params = t["w"] is not None
    gwb = ws = gwb_chk = ws_chk = None
    if params:
        n = lib.mk_chan_layernorm_workspace(B, C, P)
        assert n == min(-(-P // MIN_TP) * B, BWD_GRID) * 2 * C
        gwb, gwb_chk = _out((2, C), F32, dev)
        ws, ws_chk = _out((n,), F32, dev, fill=NAN)            # exactly that many floats; need not be cleared: full of NaN
    _lib.check(lib.mk_chan_layernorm_bwd(x.data_ptr(), _code(x.dtype), gy.data_ptr(), _code(gy.dtype), stats.data_ptr(), _p(f["w"]),
                                         _p(f["b"]), gx.data_ptr(), _p(ws), _p(gwb), B, C, P, int(fuse), ops._stream()),
               "mk_chan_layernorm_bwd")
    torch.cuda.synchronize()
    gx_chk("bwd gx")
    if params:
        gwb_chk("bwd gwb")
        ws_chk("bwd workspace")                                 # by its bytes (NaN never equals NaN)
    return dict(gx=gx, gwb=gwb)


def run_case(dev, B, C, P, xd, gd, fuse, dist="n53", off_x=0, off_out=0, params=True, repeat=False, seed=0):
    """Both passes against float64; returns the worst ratios as fractions of their limits and prints them."""
    t = cc.make_inputs(B, C, P, dist, seed, xd, gd)
    if not params:
        t["w"] = t["b"] = None
    what = f"({B}, {C}, {P}) x {NAME[xd]} gy {NAME[gd]} {'gelu ' if fuse else ''}{dist}" + (f" x+{off_x}" if off_x else "") + \
           (f" out+{off_out}" if off_out else "") + ("" if params else " no parameters")
    ref = cc.reference(t["x"], t["w"], t["b"], EPS, t["gy"], fuse, gd, xd)
    f = forward(dev, t, gd, fuse, off_x, off_out)
    worst = cc.check_forward(ref, cc.rows(f["y"].cpu()), f["stats"].cpu(), what)
    g = backward(dev, t, f, fuse, off_out)
    gw, gb = (g["gwb"][0].cpu(), g["gwb"][1].cpu()) if params else (None, None)
    worst.update(cc.check_backward(ref, cc.rows(g["gx"].cpu()), gw, gb, what))
    if repeat:
        again = backward(dev, t, f, fuse, off_out)
        assert torch.equal(again["gx"], g["gx"]), f"{what}: gx of a second run differs"
        assert torch.equal(again["gwb"], g["gwb"]), f"{what}: the parameter gradients of a second run differ"
    limits = dict(y=cc.C_Y, mean=cc.C_STAT, rstd=cc.C_STAT, gx=cc.C_GX, gw=cc.C_GW, gb=cc.C_GB)
    print(f"[chnorm-guard] {what}: " + " ".join(f"{k} {v / limits[k]:.2f}" for k, v in worst.items()) + " of their limits")
    return worst


def _ids(pair):
    return f"{NAME[pair[0]]}-{NAME[pair[1]]}"


pairs = pytest.mark.parametrize("pair", PAIRS, ids=_ids)
fused = pytest.mark.parametrize("fuse", [False, True], ids=["plain", "gelu"])


@pairs
@fused
def test_below_one_tile(dev, pair, fuse):
    assert fwd_plan(2, 5, 15, pair[0])[0] == 2
    run_case(dev, 2, 5, 15, *pair, fuse)


@pairs
@fused
@pytest.mark.parametrize("dist", ["n53", "n50"])
def test_vector_path_with_a_one_vector_tail(dev, pair, fuse, dist):
    """C over 64 and no multiple of it; the forward's last tile holds one 16-byte vector."""
    P = 36 if pair[0] == F32 else 72
    tp, v = (32, 4) if pair[0] == F32 else (64, 8)
    assert P % tp == v
    run_case(dev, 1, 73, P, *pair, fuse, dist)


@pairs
@fused
@pytest.mark.parametrize("C", [64, 65])
def test_whole_tiles_one_channel_per_row_group_and_one_more(dev, pair, fuse, C):
    run_case(dev, 1, C, 96, *pair, fuse)


@pairs
@fused
@pytest.mark.parametrize("which", ["x", "out"])
def test_element_path_chosen_by_the_pointer(dev, pair, fuse, which):
    """P a multiple of the vector, but x, or only y / gx, one element past a 16-byte boundary."""
    assert 40 % 8 == 0
    run_case(dev, 2, 9, 40, *pair, fuse, off_x=int(which == "x"), off_out=int(which == "out"))


def test_limits_are_the_documented_ones():
    assert (fwd_limit(F32), fwd_limit(BF16)) == (1214, 1148)
    assert (bwd_limit(F32, F32), bwd_limit(BF16, BF16), bwd_limit(BF16, F32), bwd_limit(F32, BF16)) == (556, 492, 734, 734)


@pairs
@pytest.mark.parametrize("beyond", [0, 2], ids=["last-staged", "first-beyond"])
def test_forward_on_chip_limit(dev, pair, beyond):
    C = fwd_limit(pair[0]) + beyond
    assert C in ((1214, 1216) if pair[0] == F32 else (1148, 1150))
    assert fwd_plan(1, C, 40, pair[0])[2] == (beyond == 0)
    run_case(dev, 1, C, 40, *pair, False)


@pairs
@fused
@pytest.mark.parametrize("beyond", [0, 1], ids=["last-staged", "first-beyond"])
def test_backward_on_chip_limit_with_several_tiles_per_workgroup(dev, pair, fuse, beyond):
    """1100 one-sample tiles of 3 pixels on 1024 workgroups: 76 of them run two tiles, with the channel sums in LDS at the limit
    and in the workspace slot one channel beyond it.  Two runs give the same bits."""
    C = bwd_limit(*pair) + beyond
    assert C in {(F32, F32): (556, 557), (BF16, BF16): (492, 493)}.get(pair, (734, 735))
    ntiles, grid, use_lds = bwd_plan(1100, C, 3, *pair)
    assert (ntiles, grid, use_lds) == (1100, 1024, beyond == 0)
    run_case(dev, 1100, C, 3, *pair, fuse, repeat=True)


PERSISTENT = [(3, 4, 22500, p, "n53") for p in PAIRS if p != (BF16, BF16)] + [(3, 4, 22500, p, "n50") for p in PAIRS if p != (BF16, BF16)] + \
             [(3, 4, 22501, p, "n53") for p in PAIRS if p != (BF16, BF16)] + [(5, 4, 22504, (BF16, BF16), "n53")]


@fused
@pytest.mark.parametrize("B,C,P,pair,dist", PERSISTENT, ids=[f"{b}x{c}x{p}-{_ids(q)}-{d}" for b, c, p, q, d in PERSISTENT])
def test_backward_persistent_loop(dev, B, C, P, pair, dist, fuse):
    """More tiles than workgroups with the sums in LDS: 2112 tiles of 32 pixels (workgroups with 3 and with 2), 1760 of 64 (2 and 1);
    the last tile of a sample is ragged and sits in the middle of a workgroup's sequence.  Two runs give the same bits."""
    ntiles, grid, use_lds = bwd_plan(B, C, P, *pair)
    tp = cc.bwd_tile_px(*pair)
    assert ntiles == -(-P // tp) * B == (1760 if pair == (BF16, BF16) else 2112) and grid == 1024 and use_lds
    assert ntiles > grid and P % tp != 0 and ntiles % grid != 0
    run_case(dev, B, C, P, *pair, fuse, dist, repeat=True)


def test_forward_stride_beyond_its_grid(dev):
    B = (1 << 20) + 7
    ntiles, grid, _ = fwd_plan(B, 3, 1, F32)
    assert ntiles == B and grid == FWD_GRID < ntiles
    run_case(dev, B, 3, 1, F32, F32, False)


@fused
def test_no_parameters_and_no_parameter_gradients(dev, fuse):
    run_case(dev, 3, 4, 22500, F32, F32, fuse, params=False)
