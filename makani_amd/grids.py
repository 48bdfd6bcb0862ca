"""Grid conversion of the data loaders: ``GridConverter`` of ``makani/utils/grids.py`` (constructor, attributes, ``get_src_coords``,
``get_dst_coords``, ``forward(data)``; no parameters, no buffers, no ``state_dict`` keys) on one HIP pass.

An equiangular archive (``nlat`` rows from pole to pole) is brought onto the Legendre-Gauss latitudes of the same ``nlat``, the grid
on which the SHT's quadrature is exact: every destination row is the linear blend of the two source rows around it,

    y[..., k, :] = lerp(x[..., i_k, :], x[..., i_k + 1, :], w_k),   lat[i_k] > dst_lat[k] >= lat[i_k + 1],
    w_k = (dst_lat[k] - lat[i_k]) / (lat[i_k + 1] - lat[i_k]),

longitudes unchanged.  The tables are built on the host: the nodes from ``numpy.polynomial.legendre.leggauss(nlat)`` in float64
(where torch-harmonics, which the reference asks, takes them from), ``dst_lat = arccos(nodes) - pi / 2`` (north to south),
``indices`` int64 by a sorted search and ``interp_weights`` float64 ``[nlat, 1]`` from the latitudes in the dtype they were given
in -- what the reference computes, bit for bit (``tests/golden/ref_grids.npz``).  They are kept on ``lat_rad.device``.

The arithmetic is ``ops.lat_interp`` (``MK_GRID=hip``: ``mk_lat_lerp_fwd`` / ``mk_lat_lerp_bwd``, ``csrc/grid.hip``; CPU tensors,
float64 and ``MK_GRID=torch``: the reference's ``torch.lerp`` expression).  Additions to the reference's ``forward(data)``:

* ``bias`` / ``scale`` (``C`` elements each, the channel axis is the last one before the rows): the loader's ``(x - bias) / scale`` in
  the same pass; ``out`` (any view with contiguous rows, such as a channel slice of the model's input buffer) and ``out_dtype``
  (fp32 or the engine's bf16);
* ``dst_rows=(k0, k1)`` with ``src_row0``: a latitude shard.  ``source_rows(k0, k1)`` is the range of source rows those destination
  rows need (one halo row beyond the naive cut); on that slab the result is bit-equal to rows ``[k0, k1)`` of the full one.

Only ``dst_grid == "legendre-gauss"`` is implemented, as in the reference (the reverse needs a rule at the poles that the reference
does not give); ``src_grid == dst_grid`` hands the data back.  Grid names are spelled with a hyphen here, as in the reference's
``grids.py`` and in ``ops.GRIDS``; the loss and metric handlers keep the reference's ``"legendre_gauss"`` with an underscore.

Where the reference gives garbage, this class raises ``ValueError``: its index search relies on latitudes that descend strictly
from north to south and are symmetric about the equator; latitudes that do not descend, or for which a computed index leaves
``[0, nlat - 2]``, are refused.
"""
import numpy as np
import torch
from torch import nn

from . import ops


class GridConverter(nn.Module):
    def __init__(self, src_grid, dst_grid, lat_rad, lon_rad):
        super().__init__()
        self.src = src_grid
        self.dst = dst_grid
        self.src_lat = lat_rad
        self.src_lon = lon_rad
        self._tables = {}           # (device, k0, k1, src_row0, rows of the slab) -> ops.LatInterpTables
        if self.src == self.dst:
            self.dst_lat = self.src_lat
            self.dst_lon = self.src_lon
            return
        if self.dst != "legendre-gauss":
            raise NotImplementedError(f"GridConverter: destination grid {self.dst!r} is not implemented (only 'legendre-gauss' is)")
        nlat = lat_rad.shape[0]
        lat = lat_rad.detach().cpu()
        if lat.dim() != 1 or nlat < 2:
            raise ValueError(f"GridConverter: latitudes {tuple(lat.shape)} must be a vector of at least two")
        if not bool((lat[1:] < lat[:-1]).all()):
            raise ValueError("GridConverter: the source latitudes must descend strictly from north to south")
        nodes, _ = np.polynomial.legendre.leggauss(nlat)
        dst_lat = torch.arccos(torch.from_numpy(nodes)) - torch.pi / 2.0
        # the position of every destination latitude among the ascending (reversed) source latitudes; read backwards it is,
        # for symmetric latitudes, the row i with lat[i] > dst_lat >= lat[i + 1]
        backwards = torch.arange(nlat - 1, -1, -1)
        indices = (torch.searchsorted(lat, dst_lat, sorter=backwards) - 1)[backwards]
        if int(indices.min()) < 0 or int(indices.max()) > nlat - 2:
            raise ValueError(f"GridConverter: source rows {int(indices.min())} ... {int(indices.max()) + 1} for {nlat} latitudes: "
                             "the source grid does not enclose the Legendre-Gauss latitudes symmetrically")
        weights = ((dst_lat - lat[indices]) / torch.diff(lat)[indices]).reshape(-1, 1)
        self.dst_lat = dst_lat.to(lat_rad.device)
        self.dst_lon = lon_rad
        self.indices = indices.to(lat_rad.device)
        self.interp_weights = weights.to(lat_rad.device)
        self._host = (indices.numpy().copy(), weights.double().reshape(-1).numpy().copy())

    def get_src_coords(self):
        return self.src_lat, self.src_lon

    def get_dst_coords(self):
        return self.dst_lat, self.dst_lon

    def source_rows(self, k0, k1):
        """``(s0, s1)``: the source rows destination rows ``[k0, k1)`` are blended from."""
        idx = self._host[0][self._rows(k0, k1)]
        return int(idx.min()), int(idx.max()) + 2

    def _rows(self, k0, k1):
        n = self._host[0].shape[0]
        if not 0 <= k0 < k1 <= n:
            raise ValueError(f"GridConverter: destination rows [{k0}, {k1}) of {n}")
        return slice(int(k0), int(k1))

    def tables(self, device, dst_rows=None, src_row0=0, n_src_rows=None):
        """The device tables of ``ops.lat_interp`` for destination rows ``dst_rows`` (default: all) on a slab of ``n_src_rows`` source
        rows (default: all) starting at ``src_row0``; built once per device and shard."""
        n = self._host[0].shape[0]
        k0, k1 = (0, n) if dst_rows is None else (int(dst_rows[0]), int(dst_rows[1]))
        n_src_rows = n - int(src_row0) if n_src_rows is None else int(n_src_rows)
        key = (torch.device(device), k0, k1, int(src_row0), n_src_rows)
        if key not in self._tables:
            rows = self._rows(k0, k1)
            self._tables[key] = ops.lat_interp_tables(self._host[0][rows], self._host[1][rows], n_src_rows, src_row0=src_row0,
                                                      device=device)
        return self._tables[key]

    def forward(self, data, bias=None, scale=None, out=None, out_dtype=None, dst_rows=None, src_row0=0):
        if self.src == self.dst:
            if not (bias is None and scale is None and out is None and out_dtype is None):
                raise ValueError("GridConverter: equal grids hand the data back; bias, scale, out and out_dtype need a conversion")
            return data
        if dst_rows is None and (src_row0 != 0 or data.shape[-2] != self._host[0].shape[0]):
            raise ValueError(f"GridConverter: input {tuple(data.shape)} must have the {self._host[0].shape[0]} source rows "
                             "(a slab takes dst_rows and src_row0)")
        tables = self.tables(data.device, dst_rows, src_row0, data.shape[-2])
        return ops.lat_interp(data, tables, bias=bias, scale=scale, out=out, out_dtype=out_dtype)
