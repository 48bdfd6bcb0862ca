"""CPU tests of the solar zenith channel (makani_amd/zenith.py, Preprocessor2D.cache_unpredicted_times).

The fixture tests/golden/ref_zenith.npz holds scalars and fields of the reference's own zenith_angle.py
(tests/golden/make_zenith_golden.py).  The host functions must reproduce it bit for bit.  Whatever evaluates the per-pixel
expression with another cosine (torch on the CPU here, cosf on the device in test_zenith_gpu.py) is held to

    BOUND = 2 * pixel_rounding        (about 1.5e-6 absolute)

where ``pixel_rounding`` is read from the fixture: the reference's own distance from the exact (float64) value of its
per-pixel expression.  The factor 2 covers a cosine of <= 2 ulp (1.2e-7) and one contraction on top of it.  The bound is
never taken from the code under test.
"""
import datetime
import os

import numpy as np
import pytest
import torch

import capi_checks as capi

from makani_amd import ops, zenith
from test_stepper_cpu import make_params

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_zenith.npz")
UTC = datetime.timezone.utc


def gold():
    return dict(np.load(GOLD).items())


def bound(g):
    return 2.0 * float(g["pixel_rounding"])


def as_datetimes(times_us):
    return np.asarray([datetime.datetime(1970, 1, 1, tzinfo=UTC) + datetime.timedelta(microseconds=int(u)) for u in times_us], dtype=object)


def fixture_cases(g):
    """(name, lat [H], lon [W], time indices, rows or None, columns or None, expected) for every field and slice."""
    n = len(g["times_us"])
    return [("33x64", g["f33_lat"], g["f33_lon"], np.arange(n), None, None, g["f33_field"]),
            ("91x180", g["f91_lat"], g["f91_lon"], g["f91_times"], None, None, g["f91_field"]),
            ("721 rows", g["f721_lat"], g["f721_lon"], g["f721_times"], g["f721_rows"], None, g["f721_row_fields"]),
            ("721 cols", g["f721_lat"], g["f721_lon"], g["f721_times"], None, g["f721_cols"], g["f721_col_fields"])]


def cut(field, rows, cols):
    if rows is not None:
        field = field[..., rows, :]
    if cols is not None:
        field = field[..., cols]
    return field


def test_fixture_holds_what_the_issue_asks_for():
    g = gold()
    have = set(g["times_us"].astype("datetime64[us]").astype("datetime64[h]").astype(str))
    assert {"1979-01-01T00", "2000-01-01T12", "2002-06-01T12", "2018-03-21T06", "2024-12-31T18"} <= have
    assert g["f33_field"].shape == (len(g["times_us"]), 33, 64) and g["f91_field"].shape == (2, 91, 180)
    assert g["f721_row_fields"].shape == (3, 8, 1440) and g["f721_col_fields"].shape == (3, 721, 8)
    assert {0, 360, 720} <= set(g["f721_rows"].tolist()) and {0, 1439} <= set(g["f721_cols"].tolist())
    assert 1e-7 < float(g["pixel_rounding"]) < 2e-6          # a few fp32 roundings of numbers of size one
    assert os.path.getsize(GOLD) < 1 << 20


def test_ephemeris_reproduces_the_reference_bit_for_bit():
    g = gold()
    want = np.stack([np.sin(g["dec"]), np.cos(g["dec"]), g["gmst"], g["ra"]], axis=-1)
    assert want.dtype == np.float32
    from_dt64 = zenith.solar_ephemeris(g["times_us"].astype("datetime64[us]"))
    from_dt = zenith.solar_ephemeris(as_datetimes(g["times_us"]))
    assert from_dt64.dtype == np.float32 and from_dt64.shape == (len(g["times_us"]), 4)
    for k, name in enumerate(("sin dec", "cos dec", "gmst", "ra")):
        assert np.array_equal(from_dt64[:, k], want[:, k]), name
    assert np.array_equal(from_dt, from_dt64)
    # coarser datetime64 units, another time zone for the same instants, a list, one time, a [B, T] array
    assert np.array_equal(zenith.solar_ephemeris(g["times_us"].astype("datetime64[us]").astype("datetime64[h]")), want)
    east = datetime.timezone(datetime.timedelta(hours=5, minutes=30))
    assert np.array_equal(zenith.solar_ephemeris([t.astimezone(east) for t in as_datetimes(g["times_us"])]), want)
    assert np.array_equal(zenith.solar_ephemeris(as_datetimes(g["times_us"])[3]), want[3])
    assert np.array_equal(zenith.solar_ephemeris(g["times_us"][:6].astype("datetime64[us]").reshape(2, 3)), want[:6].reshape(2, 3, 4))


def test_naive_datetime_raises():
    with pytest.raises(ValueError, match="naive"):
        zenith.solar_ephemeris(datetime.datetime(2018, 3, 21, 6))
    with pytest.raises(ValueError, match="naive"):
        zenith.solar_ephemeris([datetime.datetime(2018, 3, 21, 6, tzinfo=UTC), datetime.datetime(2018, 3, 21, 12)])
    with pytest.raises(TypeError):
        zenith.solar_ephemeris([1.0, 2.0])


def test_cos_zenith_angle_equals_every_fixture_field_bit_for_bit():
    g = gold()
    times = as_datetimes(g["times_us"])
    for name, lat, lon, idx, rows, cols, want in fixture_cases(g):
        lon2, lat2 = np.meshgrid(lon, lat)
        got = zenith.cos_zenith_angle(times[idx], lon2, lat2)
        assert got.dtype == np.float32 and got.shape == (len(idx), len(lat), len(lon)), name
        assert np.array_equal(cut(got, rows, cols), want), name
    # arrays that are no lat / lon grid take the pointwise route: the same numbers
    lon2, lat2 = np.meshgrid(g["f33_lon"], g["f33_lat"])
    perm = np.random.default_rng(0).permutation(lon2.size)
    got = zenith.cos_zenith_angle(times, lon2.reshape(-1)[perm].reshape(lon2.shape), lat2.reshape(-1)[perm].reshape(lon2.shape))
    assert np.array_equal(got.reshape(len(times), -1), g["f33_field"].reshape(len(times), -1)[:, perm])


def test_module_on_cpu_tensors_within_the_bound():
    g = gold()
    eph = torch.from_numpy(zenith.solar_ephemeris(g["times_us"].astype("datetime64[us]")))
    for name, lat, lon, idx, rows, cols, want in fixture_cases(g):
        mod = zenith.CosZenith(lat, lon)
        assert set(dict(mod.named_buffers())) == {"sin_lat", "cos_lat", "lon_rad"} and not mod.state_dict()
        got = mod(eph[idx][None])
        assert got.dtype == torch.float32 and got.shape == (1, len(idx), 1, len(lat), len(lon)), name
        err = np.abs(cut(got[0, :, 0].numpy(), rows, cols).astype(np.float64) - want).max()
        print(f"CosZenith (CPU) vs reference, {name}: {err:.3e} (bound {bound(g):.3e})")
        assert err <= bound(g), name


def test_shard_equals_the_slice_of_the_full_field():
    g = gold()
    eph = torch.from_numpy(zenith.solar_ephemeris(g["times_us"][:4].astype("datetime64[us]").reshape(2, 2)))
    lat, lon = g["f721_lat"], g["f721_lon"]
    full = zenith.CosZenith(lat, lon)(eph)
    shard = zenith.CosZenith(lat, lon, offset=(91, 3), local_shape=(84, 179))(eph)
    assert shard.shape == (2, 2, 1, 84, 179)
    assert torch.equal(shard, full[..., 91:175, 3:182])
    # the last shard of an uneven split is clipped to the grid
    p = make_params(721, 1440, lat=lat, lon=lon, img_local_offset_x=637, img_local_offset_y=1261, img_local_shape_x=91,
                    img_local_shape_y=180)
    tail = zenith.CosZenith.from_params(p)(eph)
    assert tail.shape == (2, 2, 1, 84, 179) and torch.equal(tail, full[..., 637:, 1261:])
    # without lat / lon the grid is the loaders' default one
    assert torch.equal(zenith.CosZenith.from_params(make_params(721, 1440))(eph), full)


@pytest.mark.parametrize("n_history", [0, 2])
@pytest.mark.parametrize("n_future", [0, 3])
@pytest.mark.parametrize("dt", [1, 4])
def test_sample_times_are_the_loaders(n_history, n_future, dt):
    year, local_idx, dhours = 2018, 317, 6
    jan_01 = datetime.datetime(year, 1, 1, 0, 0, 0, tzinfo=UTC)
    want_inp = [jan_01 + datetime.timedelta(hours=idx * dhours) for idx in range(local_idx - dt * n_history, local_idx + 1, dt)]
    want_tar = [jan_01 + datetime.timedelta(hours=idx * dhours)
                for idx in range(local_idx + dt, local_idx + dt * (n_future + 1) + 1, dt)]
    inp, tar = zenith.sample_times(year, local_idx, dhours, dt, n_history, n_future)
    assert list(inp) == want_inp and list(tar) == want_tar
    assert len(inp) == n_history + 1 and len(tar) == n_future + 1 and inp[-1] == want_inp[-1]
    assert all(t.tzinfo is not None for t in list(inp) + list(tar))
    assert zenith.solar_ephemeris(inp).shape == (n_history + 1, 4)


# ---------------------------------------------------------------------------- independent of the reference
def _ephemeris_f64(times_us):
    """The published formulas in float64, stated once more: Meeus' low-precision sun (mean anomaly M, mean longitude L,
    equation of centre C), the IAU obliquity polynomial and the GMST of AIAA 2006-6753, T in Julian centuries from J2000."""
    jd = np.asarray(times_us, dtype=np.float64) / 86400e6 + 2440587.5
    T = (jd - 2451545.0) / 36525.0
    rad = np.pi / 180.0
    M = (357.52910 + T * (35999.05030 + T * (-0.0001559 - T * 0.00000048))) * rad
    L = (280.46645 + T * (36000.76983 + T * 0.0003032)) * rad
    C = ((1.914600 + T * (-0.004817 - T * 0.000014)) * np.sin(M) + (0.019993 - 0.000101 * T) * np.sin(2 * M)
         + 0.000290 * np.sin(3 * M)) * rad
    lam = L + C
    arcsec = T * (46.836769 + T * (-0.0001831 + T * (0.00200340 + T * (-0.576e-6 - T * 4.34e-8))))
    eps = (23.0 + 26.0 / 60.0 + (21.406 - arcsec) / 3600.0) * rad
    dec = np.arcsin(np.sin(eps) * np.sin(lam))
    ra = np.arctan2(np.cos(eps) * np.sin(lam), np.cos(lam))
    gmst_s = 67310.54841 + T * (876600.0 * 3600.0 + 8640184.812866 + T * (0.093104 - T * 6.2e-6))
    gmst = np.mod(gmst_s / 240.0 * rad, 2 * np.pi)
    return dec, ra, gmst


def test_exact_ephemeris_against_the_published_formulas_in_float64():
    """The field from ``exact=True`` scalars against float64 throughout.  The grid is the module's: coordinates in fp32
    radians.  What remains is the rounding of the four scalars (GMST below 2 pi: 2.4e-7, the rest less) and of the
    per-pixel expression, which is what the bound is made for."""
    g = gold()
    dec, ra, gmst = _ephemeris_f64(g["times_us"])
    eph = zenith.solar_ephemeris(g["times_us"].astype("datetime64[us]"), exact=True)
    assert eph.dtype == np.float32
    # the scalars themselves: one fp32 rounding each (angles compared on the circle)
    assert np.abs(eph[:, 0] - np.sin(dec)).max() <= 6e-8 and np.abs(eph[:, 1] - np.cos(dec)).max() <= 6e-8
    assert np.abs(np.angle(np.exp(1j * (eph[:, 2].astype(np.float64) - gmst)))).max() <= 2.4e-7
    assert np.abs(np.angle(np.exp(1j * (eph[:, 3].astype(np.float64) - ra)))).max() <= 2.4e-7
    lat, lon = g["f91_lat"], g["f91_lon"]
    latr = np.deg2rad(lat, dtype=np.float32).astype(np.float64)[None, :, None]
    lonr = np.deg2rad(lon, dtype=np.float32).astype(np.float64)[None, None, :]
    d, a, s = (v[:, None, None] for v in (dec, ra, gmst))
    want = np.sin(latr) * np.sin(d) + np.cos(latr) * np.cos(d) * np.cos(s + lonr - a)
    got = zenith.CosZenith(lat, lon)(torch.from_numpy(eph)[None])[0, :, 0].numpy()
    err = np.abs(got - want).max()
    print(f"exact=True field vs float64 formulas: {err:.3e} (bound {bound(g):.3e})")
    assert err <= bound(g)
    # the reference's fp32 chain is 1e-3 to 2e-3 off the same formulas for dates far from 2000; exact=True is not
    ref = zenith.CosZenith(lat, lon)(torch.from_numpy(zenith.solar_ephemeris(g["times_us"].astype("datetime64[us]")))[None])
    assert np.abs(ref[0, :, 0].numpy() - want).max() > 5e-4


def test_physics_of_the_field():
    g = gold()
    lat, lon = g["f91_lat"], g["f91_lon"]
    eph = zenith.solar_ephemeris(g["times_us"].astype("datetime64[us]"), exact=True)
    f = zenith.CosZenith(lat, lon)(torch.from_numpy(eph)[None])[0, :, 0].numpy().astype(np.float64)
    assert np.abs(f).max() <= 1 + 1e-6
    # the subsolar point lies within half a cell (1 degree) of a grid point: cos(1.5 deg) = 0.99966
    assert (f.max(axis=(1, 2)) >= 0.999).all()
    # the integral over the sphere of the cosine of the angle to a fixed direction is zero
    theta, w = ops.quadrature("equiangular", len(lat))
    assert np.allclose(np.rad2deg(theta), 90.0 - lat, atol=1e-9) and abs(w.sum() - 2.0) < 1e-12
    mean = (f.mean(axis=2) * w[None]).sum(axis=1) / 2.0
    print("sphere means:", mean)
    assert np.abs(mean).max() <= 1e-5
    # and its square integrates to 1/3
    assert np.abs(((f ** 2).mean(axis=2) * w[None]).sum(axis=1) / 2.0 - 1.0 / 3.0).max() <= 1e-3


# ---------------------------------------------------------------------------- the preprocessor hook
class _Mix(torch.nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv = torch.nn.Conv2d(cin, cout, 1)

    def forward(self, x):
        return self.conv(x)


def _wrapper(H, W, T, C, cls_name="MultiStepWrapper", **kw):
    from makani_amd import stepper
    torch.manual_seed(5)
    p = make_params(H, W, n_history=T - 1, add_grid=True, **kw)
    wrap = getattr(stepper, cls_name)(p, lambda: _Mix(T * (C + 1) + 4, C))
    wrap.eval()
    return wrap


def test_cache_unpredicted_times_equals_caching_the_fields():
    g = gold()
    H, W, B, T, C, steps = 33, 64, 2, 2, 3, 3
    lat, lon = g["f33_lat"], g["f33_lon"]
    wrap = _wrapper(H, W, T, C, n_future=steps - 1, lat=lat, lon=lon)
    pp = wrap.preprocessor
    keys = sorted(wrap.state_dict())
    assert keys == ["model.conv.bias", "model.conv.weight"]
    samples = [zenith.sample_times(2018, 317 + 40 * b, 6, 2, T - 1, steps - 1) for b in range(B)]
    inp_times, tar_times = np.stack([s[0] for s in samples]), np.stack([s[1] for s in samples])
    assert inp_times.shape == (B, T) and tar_times.shape == (B, steps)
    # the fields themselves: the module's, within the bound of the reference's numpy function on the same times
    cosz = zenith.CosZenith(lat, lon)
    xz = cosz(torch.from_numpy(zenith.solar_ephemeris(inp_times)))
    yz = cosz(torch.from_numpy(zenith.solar_ephemeris(tar_times)))
    lon2, lat2 = np.meshgrid(lon, lat)
    ref = np.stack([zenith.cos_zenith_angle(tar_times[b], lon2, lat2) for b in range(B)])
    assert np.abs(yz[:, :, 0].numpy() - ref).max() <= bound(g)
    inp = torch.randn(B, T * C, H, W, generator=torch.Generator().manual_seed(1))

    def rollout(cache):
        pp.unpredicted_inp_eval = pp.unpredicted_tar_eval = None
        cache()
        state = (pp.unpredicted_inp_eval.clone(), pp.unpredicted_tar_eval.clone())
        outs, x = [], inp
        with torch.no_grad():
            for step in range(steps):
                y = wrap(x)
                outs.append(y)
                x = pp.append_history(x, y, step)
        return state, outs, pp.unpredicted_inp_eval.clone()

    s_f, o_f, u_f = rollout(lambda: pp.cache_unpredicted_features(None, None, xz.clone(), yz.clone()))
    s_t, o_t, u_t = rollout(lambda: pp.cache_unpredicted_times(inp_times, tar_times))
    assert s_t[0].shape == (B, T, 1, H, W) and s_t[1].shape == (B, steps, 1, H, W)
    assert torch.equal(s_t[0], s_f[0]) and torch.equal(s_t[1], s_f[1])
    for a, b in zip(o_t, o_f):
        assert torch.equal(a, b)
    assert torch.equal(u_t, u_f) and torch.equal(u_t[:, -1], yz[:, steps - 1])
    assert not torch.equal(o_t[0], o_t[1])
    # a second call copies into the cached tensors (the behaviour of cache_unpredicted_features), from times or from
    # ready [B, T, 4] scalars alike
    held = pp.unpredicted_inp_eval
    pp.cache_unpredicted_times(torch.from_numpy(zenith.solar_ephemeris(inp_times)))
    assert pp.unpredicted_inp_eval is held and torch.equal(held, xz)
    # exact=True reaches the ephemeris
    pp.cache_unpredicted_times(inp_times, exact=True)
    assert pp.unpredicted_inp_eval is held and not torch.equal(held, xz) and (held - xz).abs().max() < 5e-3
    assert sorted(wrap.state_dict()) == keys


def test_wrappers_are_unchanged_unless_the_method_is_called():
    for name in ("SingleStepWrapper", "MultiStepWrapper"):
        wrap = _wrapper(33, 64, 1, 3, cls_name=name)
        assert sorted(wrap.state_dict()) == ["model.conv.bias", "model.conv.weight"]
        assert [n for n, _ in wrap.preprocessor.named_buffers()] == ["history_normalization_weights", "static_features"]
        assert [n for n, _ in wrap.preprocessor.named_children()] == []
        # one sample given as [T] times; the default grid of the loaders
        wrap.preprocessor.cache_unpredicted_times(zenith.sample_times(2020, 5, 6, 1, 0, 0)[0])
        assert wrap.preprocessor.unpredicted_inp_eval.shape == (1, 1, 1, 33, 64) and wrap.preprocessor.unpredicted_tar_eval is None
        assert sorted(wrap.state_dict()) == ["model.conv.bias", "model.conv.weight"]
        assert [n for n, _ in wrap.preprocessor.named_buffers()] == ["history_normalization_weights", "static_features"]
        with torch.no_grad():
            assert wrap(torch.zeros(1, 3, 33, 64)).shape == (1, 3, 33, 64)


def test_the_op_has_no_cpu_fallback():
    z = torch.zeros(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cos_zenith(z, torch.zeros(3), torch.ones(3), torch.zeros(5))


# ---------------------------------------------------------------------------------------------------------------------
# misaligned pointers: refused by the host checks, with the message of the check (tests/capi_checks.py)
# ---------------------------------------------------------------------------------------------------------------------
_A = capi.A
MISALIGNED = [      # entry point, its arguments in front of the stream with one pointer moved off its alignment, the refusal
    ("mk_cos_zenith", (_A, _A, _A, _A, _A + 2, 1, 4, 8), "fp32 stream not 4-byte aligned"),
    ("mk_cos_zenith", (_A + 2, _A, _A, _A, _A, 1, 4, 8), "fp32 stream not 4-byte aligned"),
]


@pytest.mark.parametrize("case", MISALIGNED, ids=capi.case_ids(MISALIGNED))
def test_misaligned_pointer_is_refused_before_any_launch(case):
    capi.assert_refused(*case)
