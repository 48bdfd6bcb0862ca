"""Generate tests/golden/ref_zenith.npz: scalars and fields of the reference's own
``makani/third_party/climt/zenith_angle.py``.

Run in the build container (the reference tree is mounted read-only there):

    python tests/golden/make_zenith_golden.py

The file is imported by path with a stub ``numba`` module whose ``jit`` / ``njit`` hand the function back, so it runs as
the plain numpy it is written in.  ``pytz`` is needed.

The fixture is data only (times, expected scalars and fields); no reference source text is stored.

* ``times_us``: int64 microseconds since the Unix epoch (UTC);
* ``days``, ``gmst``, ``ra``, ``dec``: the reference's fp32 scalars per time;
* ``f33_*``: lat / lon in degrees and full fields on 33 x 64 for all times;
* ``f91_*``: full fields on 91 x 180 for two times;
* ``f721_*``: on 721 x 1440 and three times, 8 rows x all columns and all rows x 8 columns;
* ``pixel_rounding``: the largest |reference - float64 evaluation of the per-pixel expression from the reference's own
  fp32 scalars and fp32 radians| over everything above -- the reference's distance from the exact value of its
  expression, from which the tests take their bound.
"""
import datetime
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

TIMES = [(1979, 1, 1, 0), (2000, 1, 1, 12), (2002, 6, 1, 12), (2018, 3, 21, 6), (2024, 12, 31, 18), (2016, 2, 29, 9), (1990, 9, 23, 21)]
ROWS_721 = [0, 1, 180, 360, 361, 540, 719, 720]
COLS_721 = [0, 1, 359, 720, 721, 1080, 1438, 1439]


def _load_reference():
    import pytz

    def identity_decorator(*args, **kwargs):
        if len(args) == 1 and callable(args[0]) and not kwargs:
            return args[0]
        return lambda f: f

    nb = types.ModuleType("numba")
    nb.jit = nb.njit = identity_decorator
    sys.modules["numba"] = nb
    spec = importlib.util.spec_from_file_location("ref_zenith_angle", os.path.join(REF, "makani/third_party/climt/zenith_angle.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, pytz


def grid(H, W):
    """The loaders' default grid, as 1-D degrees and as the 2-D arrays the reference takes."""
    res = 180.0 / (H - 1)
    lat = np.arange(-90, 90 + res, res)[::-1]
    lon = np.arange(0, 360, 360.0 / W)
    assert lat.shape == (H,) and lon.shape == (W,)
    lon2, lat2 = np.meshgrid(lon, lat)
    return lat, lon, lat2, lon2


def main():
    ref, pytz = _load_reference()
    times = np.asarray([datetime.datetime(y, m, d, h, 0, 0, tzinfo=pytz.utc) for (y, m, d, h) in TIMES])
    epoch = datetime.datetime(1970, 1, 1, tzinfo=pytz.utc)
    out = {"times_us": np.asarray([(t - epoch) // datetime.timedelta(microseconds=1) for t in times], dtype=np.int64)}
    ra, dec = ref._right_ascension_declination(times)
    out.update(days=ref._days_from_2000(times), gmst=ref._greenwich_mean_sidereal_time(times), ra=np.asarray(ra), dec=np.asarray(dec))
    for k in ("days", "gmst", "ra", "dec"):
        assert out[k].dtype == np.float32 and out[k].shape == (len(TIMES),), (k, out[k].dtype, out[k].shape)

    worst = 0.0

    def rounding(field, idx, lat2, lon2):
        """|reference - float64 expression| from the reference's fp32 scalars and fp32 radians."""
        nonlocal worst
        lonr = np.deg2rad(lon2, dtype=np.float32).astype(np.float64)[None]
        latr = np.deg2rad(lat2, dtype=np.float32).astype(np.float64)[None]
        g, a, d = (out[k][idx].astype(np.float64).reshape(-1, 1, 1) for k in ("gmst", "ra", "dec"))
        exact = np.sin(latr) * np.sin(d) + np.cos(latr) * np.cos(d) * np.cos((g + lonr) - a)
        worst = max(worst, float(np.abs(field.astype(np.float64) - exact).max()))

    lat, lon, lat2, lon2 = grid(33, 64)
    f = ref.cos_zenith_angle(times, lon2, lat2)
    assert f.dtype == np.float32 and f.shape == (len(TIMES), 33, 64)
    rounding(f, np.arange(len(TIMES)), lat2, lon2)
    out.update(f33_lat=lat, f33_lon=lon, f33_field=f)

    lat, lon, lat2, lon2 = grid(91, 180)
    idx = np.asarray([2, 3])
    f = ref.cos_zenith_angle(times[idx], lon2, lat2)
    rounding(f, idx, lat2, lon2)
    out.update(f91_lat=lat, f91_lon=lon, f91_times=idx, f91_field=f)

    lat, lon, lat2, lon2 = grid(721, 1440)
    idx = np.asarray([0, 3, 4])
    f = ref.cos_zenith_angle(times[idx], lon2, lat2)
    assert f.dtype == np.float32 and f.shape == (3, 721, 1440)
    rounding(f, idx, lat2, lon2)
    out.update(f721_lat=lat, f721_lon=lon, f721_times=idx, f721_rows=np.asarray(ROWS_721), f721_cols=np.asarray(COLS_721),
               f721_row_fields=f[:, ROWS_721, :].copy(), f721_col_fields=f[:, :, COLS_721].copy())

    out["pixel_rounding"] = np.float64(worst)
    path = os.path.join(HERE, "ref_zenith.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays, pixel_rounding {worst:.3e}")


if __name__ == "__main__":
    main()
