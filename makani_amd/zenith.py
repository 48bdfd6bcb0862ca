"""Cosine of the solar zenith angle: the unpredicted input channel of the production configurations.

The reference's loaders compute it on the host (``makani/third_party/climt/zenith_angle.py::cos_zenith_angle``, which
needs ``numba``) and upload one ``[H, W]`` field per time level.  On a lat / lon grid the function is separable,

    cosz[n, i, j] = sin(lat_i) sin(dec_n) + cos(lat_i) cos(dec_n) cos((GMST_n + lon_j) - ra_n)

so a time level is four scalars and the grid is two latitude tables and one longitude table:

* ``solar_ephemeris(times, exact=False)`` -- the four scalars ``(sin dec, cos dec, GMST, ra)`` per time, on the host;
* ``cos_zenith_angle(time, lon, lat)`` -- the reference's function in plain numpy, bit-equal to it;
* ``sample_times(...)`` -- the times of a sample's input and target steps, as the multifiles loader forms them;
* ``CosZenith`` -- an ``nn.Module`` holding the tables of a (local) grid; ``forward(eph[B, T, 4])`` gives
  ``[B, T, 1, H, W]``, on CUDA tensors through one store-only HIP kernel (``ops.cos_zenith`` / ``mk_cos_zenith``);
* ``Preprocessor2D.cache_unpredicted_times`` (``preprocessor.py``) feeds the step wrappers from times.

The astronomy is written from the published formulas: the sun's mean anomaly, mean longitude and equation of centre of
Meeus, *Astronomical Algorithms* (as tabulated at geoastro.de/elevaz/basics/meeus.htm), Greenwich mean sidereal time of
Vallado et al., AIAA 2006-6753, and the fifth-order IAU obliquity polynomial.

``exact=False`` (the default) gives the reference's numbers bit for bit, which means rounding where it rounds: the days
since J2000 are formed in float64 and rounded to fp32, and everything after that is fp32 with the constants entering as
Python scalars.  The GMST polynomial is then evaluated on an fp32 argument of ~7e8 seconds, whose ulp is 64 s, and its
cubic coefficient is the reference's ``6.2 * 10e-6`` (ten times the published 6.2e-6; invisible next to the ulp).  Any other
order of operations moves the field by up to 5e-3, so the order below is the reference's and must stay.  For dates far from
2000 these numbers are 1e-3 to 2e-3 away from the same formulas in float64; ``exact=True`` evaluates them in float64 with
the published coefficient and rounds only the four results.
"""
import datetime

import numpy as np
import torch
from torch import nn

from . import ops

_F32 = np.float32
_J2000 = np.datetime64("2000-01-01T12:00:00", "us")
_EPOCH = datetime.datetime(1970, 1, 1, tzinfo=datetime.timezone.utc)
_DAY_US = 86400 * 1000000
_TWO_PI = 2 * np.pi


# ------------------------------------------------------------------------------------------------ times
def _utc_microseconds(times):
    """``(int64 microseconds since the Unix epoch, shape)`` of tz-aware datetimes, arrays of them, or datetime64 (UTC)."""
    arr = np.asarray(times)
    if np.issubdtype(arr.dtype, np.datetime64):
        return arr.astype("datetime64[us]").astype(np.int64).reshape(-1), arr.shape
    if arr.dtype != object:
        raise TypeError(f"times must be tz-aware datetimes or numpy.datetime64, got dtype {arr.dtype}")
    us = np.empty(arr.size, dtype=np.int64)
    for k, t in enumerate(arr.reshape(-1)):
        if not isinstance(t, datetime.datetime):
            raise TypeError(f"times must be tz-aware datetimes or numpy.datetime64, got {type(t).__name__}")
        if t.tzinfo is None or t.utcoffset() is None:
            raise ValueError(f"naive datetime {t!r}: the zenith angle needs a time zone (UTC is not assumed)")
        d = t - _EPOCH
        us[k] = (d.days * 86400 + d.seconds) * 1000000 + d.microseconds
    return us, arr.shape


def _days_since_j2000(us):
    """float64 days since 2000-01-01T12:00Z: the quotient of two integer microsecond counts, as numpy divides timedeltas."""
    return (us - _J2000.astype(np.int64)).astype(np.float64) / np.float64(_DAY_US)


def sample_times(year, local_idx, dhours, dt, n_history, n_future):
    """``(inp_times, tar_times)`` of the sample at index ``local_idx`` of ``year``: object arrays of UTC datetimes at
    ``dhours`` per index, ``n_history + 1`` input steps ending at ``local_idx`` and ``n_future + 1`` target steps after it,
    ``dt`` indices apart (the ranges of ``data_loader_multifiles.py::_compute_zenith_angle``)."""
    jan_01 = datetime.datetime(year, 1, 1, 0, 0, 0, tzinfo=datetime.timezone.utc)

    def at(indices):
        out = np.empty(len(indices), dtype=object)
        out[:] = [jan_01 + datetime.timedelta(hours=idx * dhours) for idx in indices]
        return out

    return (at(range(local_idx - dt * n_history, local_idx + 1, dt)),
            at(range(local_idx + dt, local_idx + dt * (n_future + 1) + 1, dt)))


# ------------------------------------------------------------------------------------------------ ephemeris
def _ephemeris_fp32(days64):
    """The reference's rounding points: fp32 days, then fp32 throughout on 1-D arrays (never 0-d, so that Python scalars
    stay weak under NumPy 1.x and 2.x alike).  Returns ``(sin dec, cos dec, gmst, ra, dec, days)``, each fp32 ``[n]``."""
    days = days64.astype(_F32)
    t = days / 36525.0                                                # Julian centuries since J2000

    # Greenwich mean sidereal time, seconds -> degrees (240 s per degree) -> radians in [0, 2 pi)
    rate = 876600 * 3600 + 8640184.812866                             # one Python double before it meets the array
    theta = _F32(67310.54841 + t * (rate + t * (0.093104 - t * 6.2 * 10e-6)))
    gmst = (np.deg2rad(theta / 240.0) % _TWO_PI).astype(_F32)

    # ecliptic longitude of the sun: mean longitude plus the equation of centre
    anomaly = np.deg2rad(357.52910 + 35999.05030 * t - 0.0001559 * t * t - 0.00000048 * t * t * t, dtype=_F32)
    mean_lon = np.deg2rad(280.46645 + 36000.76983 * t + 0.0003032 * (t ** 2), dtype=_F32)
    centre = np.deg2rad((1.914600 - 0.004817 * t - 0.000014 * (t ** 2)) * np.sin(anomaly)
                        + (0.019993 - 0.000101 * t) * np.sin(2 * anomaly) + 0.000290 * np.sin(3 * anomaly), dtype=_F32)
    ecl_lon = mean_lon + centre

    # obliquity of the ecliptic: 23 deg 26' 21.406" minus the polynomial in arc seconds
    eps = np.deg2rad(23.0 + 26.0 / 60 + 21.406 / 3600.0
                     - (46.836769 * t - 0.0001831 * (t ** 2) + 0.00200340 * (t ** 3) - 0.576e-6 * (t ** 4)
                        - 4.34e-8 * (t ** 5)) / 3600.0, dtype=_F32)

    # equatorial unit vector of the sun -> declination and right ascension (half-angle form of atan2(y, x))
    x = np.cos(ecl_lon)
    y = np.cos(eps) * np.sin(ecl_lon)
    z = np.sin(eps) * np.sin(ecl_lon)
    r = np.sqrt(1.0 - z * z)
    dec = np.arctan2(z, r)
    ra = _F32(2.0 * np.arctan2(y, x + r))
    return np.sin(dec), np.cos(dec), gmst, ra, dec, days


def _horner(t, *coeffs):
    """``c0 + c1 t + c2 t^2 + ...``"""
    acc = np.zeros_like(t)
    for c in reversed(coeffs):
        acc = acc * t + c
    return acc


def _ephemeris_fp64(days64):
    """The same astronomy in float64, straight from the published polynomials in T (Julian centuries since J2000), each in
    Horner form, with the published cubic coefficient of the GMST polynomial."""
    t = days64 / 36525.0
    deg = np.pi / 180.0
    # Meeus: mean anomaly M, mean longitude L0, equation of centre C (degrees)
    m = deg * _horner(t, 357.52910, 35999.05030, -0.0001559, -0.00000048)
    l0 = _horner(t, 280.46645, 36000.76983, 0.0003032)
    c = (_horner(t, 1.914600, -0.004817, -0.000014) * np.sin(m) + _horner(t, 0.019993, -0.000101) * np.sin(2.0 * m)
         + 0.000290 * np.sin(3.0 * m))
    lam = deg * (l0 + c)                                              # true ecliptic longitude
    # obliquity: 23 deg 26' 21.406" minus a polynomial in arc seconds
    eps = deg * (23.0 + (26.0 + (21.406 - _horner(t, 0.0, 46.836769, -0.0001831, 0.00200340, -0.576e-6, -4.34e-8)) / 60.0) / 60.0)
    sin_dec = np.sin(eps) * np.sin(lam)
    ra = np.arctan2(np.cos(eps) * np.sin(lam), np.cos(lam))
    # AIAA 2006-6753: GMST in seconds of time, 240 s per degree
    gmst_s = _horner(t, 67310.54841, 876600.0 * 3600.0 + 8640184.812866, 0.093104, -6.2e-6)
    gmst = np.mod(deg * (gmst_s / 240.0), _TWO_PI)
    return sin_dec, np.sqrt(1.0 - sin_dec * sin_dec), gmst, ra


def solar_ephemeris(times, exact=False):
    """``np.float32 [..., 4]``: ``(sin dec, cos dec, GMST, right ascension)`` of the sun per time (angles in radians), in
    the shape of ``times`` -- tz-aware ``datetime``s, arrays of them, or ``numpy.datetime64`` taken as UTC.  A naive
    ``datetime`` raises ``ValueError``.  ``exact=False`` is the reference bit for bit, ``exact=True`` float64 astronomy
    rounded once (see the module docstring)."""
    us, shape = _utc_microseconds(times)
    days64 = _days_since_j2000(us)
    parts = _ephemeris_fp64(days64) if exact else _ephemeris_fp32(days64)[:4]
    return np.stack([np.asarray(p, dtype=_F32) for p in parts], axis=-1).reshape(tuple(shape) + (4,))


# ------------------------------------------------------------------------------------------------ numpy fields
def grid_tables(lat_deg, lon_deg):
    """``(sin_lat [H], cos_lat [H], lon_rad [W])`` fp32 from 1-D coordinates in degrees, made the reference's way:
    ``deg2rad(., dtype=float32)``, then fp32 sine and cosine."""
    lat_rad = np.deg2rad(np.asarray(lat_deg).reshape(-1), dtype=_F32)
    lon_rad = np.deg2rad(np.asarray(lon_deg).reshape(-1), dtype=_F32)
    return np.sin(lat_rad), np.cos(lat_rad), lon_rad


def _fields(eph, sin_lat, cos_lat, lon_rad):
    """``[n, ...]`` fp32 from ``eph [n, 4]`` and tables that broadcast against each other (``[H, 1]`` / ``[1, W]`` on a
    lat / lon grid, ``[H, W]`` each in general).  Every operation is a separate fp32 rounding, in the reference's order."""
    e = eph.reshape(-1, 4).reshape((-1, 4) + (1,) * sin_lat.ndim)
    sin_dec, cos_dec, gmst, ra = e[:, 0], e[:, 1], e[:, 2], e[:, 3]
    hour = (gmst + lon_rad[None]) - ra
    return sin_lat[None] * sin_dec + cos_lat[None] * cos_dec * np.cos(hour)


def cos_zenith_angle(time, lon, lat):
    """Cosine of the solar zenith angle at ``time`` (UTC) for ``lon`` / ``lat`` in degrees (2-D arrays of one shape):
    fp32 ``[t, lat, lon]``.  Signature and result of the reference's function, in plain numpy.  A lat / lon grid (every row
    of ``lon`` and every column of ``lat`` alike) is evaluated from its three tables, any other pair of arrays pointwise;
    the numbers are the same."""
    eph = solar_ephemeris(np.reshape(np.asarray(time), (-1,)))
    lon_rad = np.deg2rad(lon, dtype=_F32)
    lat_rad = np.deg2rad(lat, dtype=_F32)
    if (lon_rad.ndim == 2 and lat_rad.shape == lon_rad.shape and np.array_equal(lon_rad, np.broadcast_to(lon_rad[:1], lon_rad.shape))
            and np.array_equal(lat_rad, np.broadcast_to(lat_rad[:, :1], lat_rad.shape))):
        lat1, lon1 = lat_rad[:, :1], lon_rad[:1]
        return _fields(eph, np.sin(lat1), np.cos(lat1), lon1)
    lon_rad, lat_rad = np.broadcast_arrays(lon_rad, lat_rad)
    return _fields(eph, np.sin(lat_rad), np.cos(lat_rad), lon_rad)


# ------------------------------------------------------------------------------------------------ the module
def default_grid(img_shape_x, img_shape_y):
    """``(lat, lon)`` in degrees of the loaders' default grid: ``lat = arange(-90, 90 + res, res)[::-1]`` with
    ``res = 180 / (H - 1)``, ``lon = arange(0, 360, 360 / W)``."""
    res = 180.0 / (img_shape_x - 1)
    lat = np.arange(-90, 90 + res, res)[::-1]
    lon = np.arange(0, 360, 360.0 / img_shape_y)
    if lat.shape[0] != img_shape_x or lon.shape[0] != img_shape_y:
        raise ValueError(f"the default grid of {img_shape_x} x {img_shape_y} has {lat.shape[0]} x {lon.shape[0]} points; pass lat / lon")
    return lat, lon


class CosZenith(nn.Module):
    """The zenith channel of a (local) lat / lon grid: ``forward(eph [B, T, 4]) -> [B, T, 1, H_loc, W_loc]`` fp32.

    ``lat_deg [H]`` and ``lon_deg [W]`` are the global coordinates in degrees; ``offset`` and ``local_shape`` select this
    rank's rows and columns (clipped to the grid, as ``Preprocessor2D`` slices its static features).  The non-persistent
    buffers ``sin_lat``, ``cos_lat``, ``lon_rad`` hold the local slices of the tables.  CUDA tensors take the HIP kernel,
    CPU tensors the same expression in torch ops; ``use_hip=False`` selects the torch ops on any device (the comparison
    of ``tools/zenith_bench.py``)."""

    def __init__(self, lat_deg, lon_deg, offset=(0, 0), local_shape=None):
        super().__init__()
        sin_lat, cos_lat, lon_rad = grid_tables(lat_deg, lon_deg)
        x0, y0 = int(offset[0]), int(offset[1])
        x1 = sin_lat.shape[0] if local_shape is None else min(x0 + int(local_shape[0]), sin_lat.shape[0])
        y1 = lon_rad.shape[0] if local_shape is None else min(y0 + int(local_shape[1]), lon_rad.shape[0])
        if not (0 <= x0 < x1 and 0 <= y0 < y1):
            raise ValueError(f"empty shard: offset {tuple(offset)}, shape {local_shape} on a {sin_lat.shape[0]} x {lon_rad.shape[0]} grid")
        self.register_buffer("sin_lat", torch.from_numpy(sin_lat[x0:x1].copy()), persistent=False)
        self.register_buffer("cos_lat", torch.from_numpy(cos_lat[x0:x1].copy()), persistent=False)
        self.register_buffer("lon_rad", torch.from_numpy(lon_rad[y0:y1].copy()), persistent=False)

    @classmethod
    def from_params(cls, params):
        if hasattr(params, "lat") and hasattr(params, "lon"):
            lat, lon = np.asarray(params.lat), np.asarray(params.lon)
        else:
            lat, lon = default_grid(params.img_shape_x, params.img_shape_y)
        return cls(lat, lon, offset=(params.img_local_offset_x, params.img_local_offset_y),
                   local_shape=(params.img_local_shape_x, params.img_local_shape_y))

    def _forward_torch(self, eph):
        e = eph.float()
        sin_dec, cos_dec, gmst, ra = (e[..., k, None, None] for k in range(4))              # [B, T, 1, 1]
        hour = (gmst + self.lon_rad) - ra                                                     # [B, T, 1, W]
        return (self.sin_lat[:, None] * sin_dec + (self.cos_lat[:, None] * cos_dec) * torch.cos(hour)).unsqueeze(2)

    def forward(self, eph, use_hip=True):
        if eph.dim() != 3 or eph.shape[-1] != 4:
            raise ValueError(f"CosZenith: eph {tuple(eph.shape)} must be [B, T, 4]")
        if not (eph.is_cuda and use_hip):
            return self._forward_torch(eph)
        return ops.cos_zenith(eph, self.sin_lat, self.cos_lat, self.lon_rad).unsqueeze(2)
