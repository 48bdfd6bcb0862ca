"""Generate tests/golden/ref_grids.npz: tables and outputs of the reference's own ``makani/utils/grids.py: GridConverter`` and the
static features its ``makani/models/preprocessor.py: Preprocessor2D`` builds from the converted coordinates.

Run in the build container (the reference tree is mounted read-only there):

    python tests/golden/make_grids_golden.py

The two modules are imported by file path (package ``__init__`` files bypassed, as in make_stepper_golden.py) with stubs for
what they import and is not installed there:``torch_harmonics.quadrature`` (``legendre_gauss_weights`` hands back
``numpy.polynomial.legendre.leggauss(n)``, which is where torch-harmonics takes its nodes from), ``makani.utils.comm`` (every
size 1) and ``modulus.distributed.mappings`` (identities).

Recorded, for nlat = 2, 3, 4, 5, 8, 33, 721 and lat = deg2rad(linspace(90, -90, nlat)) in fp32 and in float64: ``lat``,
``dst_lat``, ``indices``, ``interp_weights``; for nlat = 3, 8, 33 and W = 2 nlat an fp32 ``[2, 3, nlat, W]`` input and the converter's output;
and ``static_features`` of a 5 x 8 preprocessor with a sinusoidal grid of two frequencies, equiangular data and a
Legendre-Gauss model grid.

The fixture is data only; no reference source text is stored.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
NLATS = (2, 3, 4, 5, 8, 33, 721)
FIELD_NLATS = (3, 8, 33)


class Params:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _load_reference_modules():
    def stub(name, **attrs):
        mod = types.ModuleType(name)
        mod.__path__ = []
        mod.__dict__.update(attrs)
        sys.modules[name] = mod
        return mod

    def leggauss(n, a, b):
        return np.polynomial.legendre.leggauss(n)

    for name in ("makani", "makani.models", "makani.utils", "modulus", "modulus.distributed", "torch_harmonics"):
        stub(name)
    stub("torch_harmonics.quadrature", legendre_gauss_weights=leggauss, clenshaw_curtiss_weights=None)
    stub("makani.utils.comm", get_size=lambda name: 1, get_rank=lambda name: 0)
    sys.modules["makani.utils"].comm = sys.modules["makani.utils.comm"]
    stub("modulus.distributed.mappings", reduce_from_parallel_region=lambda x, name: x, copy_to_parallel_region=lambda x, name: x)

    def load(modname, relpath):
        spec = importlib.util.spec_from_file_location(modname, os.path.join(REF, relpath))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[modname] = mod
        spec.loader.exec_module(mod)
        return mod

    grids = load("makani.utils.grids", "makani/utils/grids.py")
    pre = load("makani.models.preprocessor", "makani/models/preprocessor.py")
    return grids, pre


def latitudes(nlat, dtype):
    """North to south, in radians, as the loaders hand them over (fp32) or in float64."""
    return torch.deg2rad(torch.linspace(90.0, -90.0, nlat, dtype=dtype))


def longitudes(nlon, dtype):
    return torch.deg2rad(torch.linspace(0.0, 360.0, nlon + 1, dtype=dtype)[:-1])


def main():
    grids, pre = _load_reference_modules()
    g = torch.Generator().manual_seed(721)
    out = {}
    for nlat in NLATS:
        for name, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            lat = latitudes(nlat, dtype)
            conv = grids.GridConverter("equiangular", "legendre-gauss", lat, longitudes(2 * nlat, dtype))
            k = f"n{nlat}_{name}_"
            out[k + "lat"] = lat.numpy()
            out[k + "dst_lat"] = conv.dst_lat.numpy()
            out[k + "indices"] = conv.indices.numpy()
            out[k + "interp_weights"] = conv.interp_weights.numpy()
            if name == "f32" and nlat in FIELD_NLATS:
                x = torch.randn(2, 3, nlat, 2 * nlat, generator=g) * 3.0 + 1.0
                out[f"n{nlat}_x"] = x.numpy()
                out[f"n{nlat}_y"] = conv(x).numpy()

    H, W = 5, 8
    lat = np.linspace(90.0, -90.0, H).astype(np.float32)
    lon = np.linspace(0.0, 360.0, W, endpoint=False).astype(np.float32)
    p = Params(n_history=0, history_normalization_mode="none", history_normalization_decay=0.5, target="default",
               normalize_residual=False, img_shape_x=H, img_shape_y=W, img_local_offset_x=0, img_local_offset_y=0,
               img_local_shape_x=H, img_local_shape_y=W, add_grid=True, gridtype="sinusoidal", grid_num_frequencies=2,
               data_grid_type="equiangular", model_grid_type="legendre-gauss", add_orography=False, add_landmask=False,
               n_future=0, lat=lat, lon=lon)
    out.update(pre_lat=lat, pre_lon=lon, pre_static=pre.Preprocessor2D(p).static_features.numpy())

    path = os.path.join(HERE, "ref_grids.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
