"""``mk_cos_zenith`` (csrc/zenith.hip) through ``ops.cos_zenith(..., out=)`` with a guarded output and tables between NaN bands.

The output sits 0, 1, 2 and 3 elements past a 16-byte boundary (the kernel's scalar head is 0, 3, 2 and 1 points, per row and
per 256-column tile), the ephemeris and the three tables each 0 and 1 elements past one, in every combination.  Every element is
bit-equal to the aligned launch of the same field, as the header of zenith.hip promises (the value of a point depends on
(n, i, j) only), and within the fixture's ``bound(g)`` of the torch formulation on the CPU; the guard bands and the elements in
front of an offset output hold the sentinel, and the tables come back bit for bit.  Widths below a vector, at, next to and beyond
the 256-column table and two tables plus three points; heights of one row, one chunk and more than a chunk of 32 rows."""
import itertools

import numpy as np
import pytest
import torch

from stream_checks import out_at, put, unchanged
from test_zenith_cpu import bound, gold

pytestmark = pytest.mark.gpu

_GOLD = []


def _gold():
    if not _GOLD:
        _GOLD.append(gold())
    return _GOLD[0]


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("H", [1, 9, 40])
@pytest.mark.parametrize("W", [1, 3, 255, 256, 259, 515])
def test_every_element_at_every_alignment(dev, W, H, n):
    from makani_amd import ops, zenith
    g = _gold()
    lat, lon = np.linspace(90.0, -90.0, H), np.arange(W) * (360.0 / W)
    eph = torch.from_numpy(zenith.solar_ephemeris(g["times_us"].astype("datetime64[us]"))[[2, 5, 0][:n]].copy())
    tabs = [torch.from_numpy(np.ascontiguousarray(t)) for t in zenith.grid_tables(lat, lon)]
    want = zenith.CosZenith(lat, lon)(eph[None])[0, :, 0]
    assert want.shape == (n, H, W)

    def launch(offs, oo):
        what = f"offsets eph {offs[0]} sin_lat {offs[1]} cos_lat {offs[2]} lon {offs[3]} out {oo}"
        placed = [put(t, o, dev) for t, o in zip([eph] + tabs, offs)]
        out, chk = out_at((n, H, W), torch.float32, oo, dev)
        res = ops.cos_zenith(*[p[0] for p in placed], out=out)
        torch.cuda.synchronize()
        assert res.data_ptr() == out.data_ptr()
        chk(what)
        for _, whole, flat in placed:
            unchanged(whole, flat, what)
        return out, what

    base, what = launch((0, 0, 0, 0), 0)
    worst = float((base.cpu().double() - want.double()).abs().max()) / bound(g)
    assert worst <= 1.0, f"{what}: {worst:.3f} of the bound against the torch formulation"
    combos = [((0, 0, 0, 0), oo) for oo in (1, 2, 3)] + [(offs, k % 4) for k, offs in enumerate(itertools.product((0, 1), repeat=4))]
    for offs, oo in combos:
        out, what = launch(offs, oo)
        bad = out.view(torch.int32) != base.view(torch.int32)
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements differ from the aligned launch, the first at " \
                                    f"{tuple(int(i) for i in torch.nonzero(bad)[0])}"
    print("RATIO mk_cos_zenith", f"{n}x{H}x{W}", f"launches={len(combos) + 1} differing elements=0 worst={worst:.3f}")
