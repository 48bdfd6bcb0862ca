"""GPU tests of the zenith kernel (csrc/zenith.hip, ops.cos_zenith, zenith.CosZenith, cache_unpredicted_times).

The bound is the one of test_zenith_cpu.py: 2 * ``pixel_rounding`` read from the fixture (about 1.5e-6 absolute), the
reference's own distance from the exact value of its per-pixel expression; the factor 2 covers a device cosf of <= 2 ulp
and one contraction on top of it.  Everything that compares the kernel with itself -- two launches, shards against
slices, one launch against many, replay against eager, times against fields -- is bit for bit.
"""
import numpy as np
import pytest
import torch

from makani_amd import _lib, ops, zenith
from test_stepper_cpu import make_params
from test_zenith_cpu import bound, cut, fixture_cases, gold

pytestmark = pytest.mark.gpu


def _tables(dev, lat, lon):
    return tuple(torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in zenith.grid_tables(lat, lon))


def _eph(dev, g, idx=None, exact=False):
    e = zenith.solar_ephemeris(g["times_us"].astype("datetime64[us]"), exact=exact)
    return torch.from_numpy(e if idx is None else e[idx]).to(dev)


def test_kernel_against_every_fixture_field(dev):
    g = gold()
    for name, lat, lon, idx, rows, cols, want in fixture_cases(g):
        got = ops.cos_zenith(_eph(dev, g, idx), *_tables(dev, lat, lon))
        assert got.dtype == torch.float32 and got.shape == (len(idx), len(lat), len(lon)), name
        err = np.abs(cut(got.cpu().numpy(), rows, cols).astype(np.float64) - want).max()
        print(f"mk_cos_zenith vs reference, {name}: {err:.3e} (bound {bound(g):.3e})")
        assert err <= bound(g), name


def test_two_launches_agree_bitwise(dev):
    g = gold()
    eph, tabs = _eph(dev, g), _tables(dev, g["f721_lat"], g["f721_lon"])
    a = ops.cos_zenith(eph, *tabs)
    b = ops.cos_zenith(eph, *tabs)
    assert torch.equal(a, b) and torch.isfinite(a).all() and a.abs().max() <= 1 + 1e-6


def test_shards_equal_slices_bitwise(dev):
    g = gold()
    eph = _eph(dev, g, [0, 3, 4])
    sin_lat, cos_lat, lon_rad = _tables(dev, g["f721_lat"], g["f721_lon"])
    full = ops.cos_zenith(eph, sin_lat, cos_lat, lon_rad)
    # rows [91 k, 91 k + 91) and the 84-row tail of 721
    for r0 in range(0, 721, 91):
        r1 = min(r0 + 91, 721)
        assert torch.equal(ops.cos_zenith(eph, sin_lat[r0:r1], cos_lat[r0:r1], lon_rad), full[:, r0:r1]), r0
    assert 721 - 7 * 91 == 84
    # a column shard at offset 3 with width 179: odd row pitch, every row starts at another alignment
    assert torch.equal(ops.cos_zenith(eph, sin_lat, cos_lat, lon_rad[3:182]), full[:, :, 3:182])
    # both at once, through the module (offset and shape of a rank of a 8 x 8 split)
    mod = zenith.CosZenith(g["f721_lat"], g["f721_lon"], offset=(91, 3), local_shape=(84, 179)).to(dev)
    assert torch.equal(mod(eph[None])[0, :, 0], full[:, 91:175, 3:182])
    # a 1439-wide output at a base that is 4 bytes off a 16-byte boundary
    buf = torch.full((3 * 721 * 1439 + 2,), 7.0, device=dev)
    assert buf.data_ptr() % 16 == 0
    out = buf[1:-1].view(3, 721, 1439)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    res = ops.cos_zenith(eph, sin_lat, cos_lat, lon_rad[:1439], out=out)
    assert res.data_ptr() == out.data_ptr() and torch.equal(out, full[:, :, :1439])
    assert buf[0] == 7.0 and buf[-1] == 7.0                       # nothing written outside


@pytest.mark.parametrize("H,W", [(1, 1), (5, 3), (9, 255), (7, 256), (6, 259), (40, 515), (3, 4099)])
def test_any_width_and_more_than_one_table(dev, H, W):
    """Widths below a vector, at and beyond the 256-column table: against the torch formulation on the CPU within the
    bound, column halves against the slices bit for bit."""
    g = gold()
    lat, lon = np.linspace(90.0, -90.0, H), np.arange(W) * (360.0 / W)
    eph = _eph(dev, g, [2, 5])
    sin_lat, cos_lat, lon_rad = _tables(dev, lat, lon)
    got = ops.cos_zenith(eph, sin_lat, cos_lat, lon_rad)
    want = zenith.CosZenith(lat, lon)(eph.cpu()[None])[0, :, 0]
    assert (got.cpu().double() - want.double()).abs().max() <= bound(g)
    c = W // 2 + 1
    assert torch.equal(ops.cos_zenith(eph, sin_lat, cos_lat, lon_rad[:c]), got[:, :, :c])
    if c < W:
        assert torch.equal(ops.cos_zenith(eph, sin_lat, cos_lat, lon_rad[c:]), got[:, :, c:])


def test_batch_of_times_in_one_launch_equals_single_launches(dev):
    g = gold()
    eph = _eph(dev, g, [0, 1, 2, 3, 4, 5]).reshape(2, 3, 4)
    tabs = _tables(dev, g["f91_lat"], g["f91_lon"])
    mod = zenith.CosZenith(g["f91_lat"], g["f91_lon"]).to(dev)
    got = mod(eph)
    assert got.shape == (2, 3, 1, 91, 180)
    for b in range(2):
        for t in range(3):
            assert torch.equal(got[b, t, 0], ops.cos_zenith(eph[b, t], *tabs)), (b, t)
    assert not torch.equal(got[0, 0], got[0, 1])
    # the module's torch formulation on the device is the comparison of the bench tool: within the bound of the kernel
    assert (mod(eph, use_hip=False) - got).abs().max() <= bound(g)


def test_more_items_than_the_grid(dev):
    """200 times x 23 row chunks x 2 column tiles = 9200 items on a grid capped at 8192: the strided items equal single
    launches."""
    g = gold()
    n = 200
    us = g["times_us"][3] + np.arange(n, dtype=np.int64) * 3600 * 1000000
    eph = torch.from_numpy(zenith.solar_ephemeris(us.astype("datetime64[us]"))).to(dev)
    tabs = _tables(dev, g["f721_lat"], g["f721_lon"][:300])
    got = ops.cos_zenith(eph, *tabs)
    for k in (0, 1, 177, 178, 199):
        assert torch.equal(got[k], ops.cos_zenith(eph[k], *tabs)), k
    want = zenith.CosZenith(g["f721_lat"], g["f721_lon"][:300])(eph.cpu()[None])[0, :, 0]
    assert (got.cpu().double() - want.double()).abs().max() <= bound(g)


# ---------------------------------------------------------------------------- the preprocessor hook
def _sfno(cin, cout, H, W, seed=11):
    from makani_amd.sfnonet import SphericalFourierNeuralOperatorNet
    torch.manual_seed(seed)
    kw = dict(inp_shape=(H, W), out_shape=(H, W), scale_factor=2, inp_chans=cin, out_chans=cout, embed_dim=16, num_layers=2,
              big_skip=True)
    return lambda: SphericalFourierNeuralOperatorNet(**kw)


def _grid(H, W):
    return np.linspace(90.0, -90.0, H), np.arange(W) * (360.0 / W)


def test_captured_times_replay_equals_eager_bitwise(dev):
    from makani_amd.preprocessor import Preprocessor2D
    g = gold()
    H, W, B, T, C = 30, 61, 2, 2, 5
    lat, lon = _grid(H, W)
    pp = Preprocessor2D(make_params(H, W, n_history=T - 1, add_grid=True, lat=lat, lon=lon)).to(dev)
    pp.eval()
    ephs = [_eph(dev, g, idx).reshape(B, T, 4) for idx in ([0, 1, 2, 3], [3, 4, 5, 6], [6, 2, 0, 5])]
    x = torch.randn(B, T * C, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(4))
    eph_static = ephs[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        eager = []
        for e in ephs:                                           # the first call builds the module and the cached tensor
            pp.cache_unpredicted_times(e)
            eager.append(pp.assemble(x).clone())
        held = pp.unpredicted_inp_eval
        pp.cache_unpredicted_times(eph_static)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            pp.cache_unpredicted_times(eph_static)
            out = pp.assemble(x)
        assert pp.unpredicted_inp_eval is held
        for e, want in list(zip(ephs, eager))[1:] + [(ephs[0], eager[0])]:
            eph_static.copy_(e)
            graph.replay()
            side.synchronize()
            assert torch.equal(out, want)
    torch.cuda.current_stream().wait_stream(side)
    assert not torch.equal(eager[0], eager[1]) and not torch.equal(eager[1], eager[2])
    cn = C + 1
    assert torch.equal(eager[2][:, cn - 1], zenith.CosZenith(lat, lon).to(dev)(ephs[2])[:, 0, 0])


@pytest.mark.parametrize("single", [True, False])
def test_wrappers_fed_times_equal_wrappers_fed_the_fields_bitwise(dev, single):
    from makani_amd import stepper
    H, W, B, T, C = 64, 128, 2, 2, 3
    steps = 1 if single else 3
    lat, lon = _grid(H, W)
    p = make_params(H, W, n_history=T - 1, add_grid=True, n_future=steps - 1, lat=lat, lon=lon, masked_channels=[1])
    cls = stepper.SingleStepWrapper if single else stepper.MultiStepWrapper
    wrap = cls(p, _sfno(T * (C + 1) + 4, C, H, W)).to(dev)
    wrap.eval()
    keys = sorted(wrap.state_dict())
    pp = wrap.preprocessor
    samples = [zenith.sample_times(2019, 200 + 31 * b, 6, 1, T - 1, steps - 1) for b in range(B)]
    inp_times, tar_times = np.stack([s[0] for s in samples]), np.stack([s[1] for s in samples])
    tabs = _tables(dev, lat, lon)
    xz = ops.cos_zenith(torch.from_numpy(zenith.solar_ephemeris(inp_times)).to(dev), *tabs).unsqueeze(2)
    yz = ops.cos_zenith(torch.from_numpy(zenith.solar_ephemeris(tar_times)).to(dev), *tabs).unsqueeze(2)
    inp = torch.randn(B, T * C, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(3))

    def rollout(cache):
        pp.unpredicted_inp_eval = pp.unpredicted_tar_eval = None
        cache()
        outs, x = [], inp
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            for step in range(steps):
                y = wrap(x)
                outs.append(y)
                x = pp.append_history(x, y, step)
        return outs, pp.unpredicted_inp_eval.clone()

    o_f, u_f = rollout(lambda: pp.cache_unpredicted_features(None, None, xz.clone(), yz.clone()))
    o_t, u_t = rollout(lambda: pp.cache_unpredicted_times(inp_times, tar_times, device=dev))
    assert pp.unpredicted_inp_eval.is_cuda and pp.unpredicted_inp_eval.shape == (B, T, 1, H, W)
    for a, b in zip(o_t, o_f):
        assert torch.equal(a, b) and torch.isfinite(a).all()
    assert torch.equal(u_t, u_f) and torch.equal(u_t[:, -1], yz[:, steps - 1])
    if not single:
        assert not torch.equal(o_t[0], o_t[1]) and not torch.equal(o_t[1], o_t[2])
    assert sorted(wrap.state_dict()) == keys


def test_one_module_per_device_however_it_is_named(dev):
    from makani_amd.preprocessor import Preprocessor2D
    lat, lon = _grid(12, 20)
    pp = Preprocessor2D(make_params(12, 20, lat=lat, lon=lon))
    assert "_cos_zenith" not in pp.__dict__                               # nothing is built before the first call
    times = zenith.sample_times(2020, 5, 6, 1, 0, 0)[0]
    pp.eval()
    pp.cache_unpredicted_times(times, device="cuda")
    held = pp.unpredicted_inp_eval
    assert held.device == dev
    pp.cache_unpredicted_times(times)                                     # device taken from the cached tensor: cuda:0
    pp.cache_unpredicted_times(times, device=dev)
    assert list(pp._cos_zenith) == [dev] and pp.unpredicted_inp_eval is held


# ---------------------------------------------------------------------------- C ABI
def test_c_abi_rejects_bad_arguments(dev):
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    eph, s, c, lon = torch.zeros(2, 4, device=dev), torch.zeros(3, device=dev), torch.ones(3, device=dev), torch.zeros(5, device=dev)
    out = torch.full((2 * 3 * 5 + 1,), 7.0, device=dev)
    args = [eph.data_ptr(), s.data_ptr(), c.data_ptr(), lon.data_ptr(), out.data_ptr()]
    assert lib.mk_cos_zenith(*args, 2, 3, 5, st) == 0
    assert lib.mk_cos_zenith(*args, 0, 3, 5, st) == 0                       # nothing to do
    for bad, why in (((-1, 3, 5), b"bad sizes"), ((2, 0, 5), b"bad sizes"), ((2, 3, 0), b"bad sizes"),
                     ((1 << 30, 1 << 20, 5), b"too large")):
        assert lib.mk_cos_zenith(*args, *bad, st) != 0
        assert why in lib.mk_last_error()
    for k in range(5):
        a = list(args)
        a[k] = None
        assert lib.mk_cos_zenith(*a, 2, 3, 5, st) != 0 and b"null pointer" in lib.mk_last_error()
        a[k] = args[k] + 2
        assert lib.mk_cos_zenith(*a, 2, 3, 5, st) != 0 and b"aligned" in lib.mk_last_error()
    torch.cuda.synchronize()
    assert out[-1] == 7.0 and out[:-1].abs().max() <= 1.0
    with pytest.raises(ValueError):
        ops.cos_zenith(eph, s, c, lon, out=torch.zeros(2, 3, 6, device=dev))
    with pytest.raises(ValueError):
        ops.cos_zenith(eph[:, :3], s, c, lon)
