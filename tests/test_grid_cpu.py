"""CPU tests of ``makani_amd.grids.GridConverter`` and ``ops.lat_interp``: the tables and the forward against a recorded run of the
reference (tests/golden/ref_grids.npz, written by tests/golden/make_grids_golden.py), the CSR transpose against the dense matrix,
autograd of the torch formulation against the float64 transpose, the opt-in of ``Preprocessor2D``, the switch and the refusals."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import capi_checks as capi
import grid_checks as gc
from makani_amd import _lib, ops
from makani_amd.grids import GridConverter
from makani_amd.preprocessor import Preprocessor2D

LG, EQ = "legendre-gauss", "equiangular"


def converter(nlat, kind="f32"):
    f = gc.fixture()
    lat = torch.from_numpy(f[f"n{nlat}_{kind}_lat"])
    lon = torch.deg2rad(torch.linspace(0.0, 360.0, 2 * nlat + 1, dtype=lat.dtype)[:-1])
    return GridConverter(EQ, LG, lat, lon)


@pytest.mark.parametrize("kind", ["f32", "f64"])
@pytest.mark.parametrize("nlat", gc.NLATS)
def test_tables_equal_the_reference(nlat, kind):
    f, conv = gc.fixture(), converter(nlat, kind)
    k = f"n{nlat}_{kind}_"
    assert conv.dst_lat.dtype == torch.float64 and torch.equal(conv.dst_lat, torch.from_numpy(f[k + "dst_lat"]))
    assert conv.indices.dtype == torch.int64 and torch.equal(conv.indices, torch.from_numpy(f[k + "indices"]))
    assert conv.interp_weights.dtype == torch.float64 and conv.interp_weights.shape == (nlat, 1)
    assert torch.equal(conv.interp_weights, torch.from_numpy(f[k + "interp_weights"]))
    idx, w = conv.indices.numpy(), conv.interp_weights.numpy().reshape(-1)
    assert (np.diff(idx) >= 0).all()
    assert len(set(idx.tolist())) == (nlat - 1 if nlat >= 3 else 1)
    assert idx.min() >= 0 and idx.max() <= nlat - 2
    if nlat % 2:
        assert w[nlat // 2] == 1.0 and idx[nlat // 2] == nlat // 2 - 1
    assert conv.get_src_coords()[0] is conv.src_lat and conv.get_dst_coords()[0] is conv.dst_lat
    assert conv.get_dst_coords()[1] is conv.src_lon and conv.src == EQ and conv.dst == LG
    assert len(conv.state_dict()) == 0


@pytest.mark.parametrize("nlat", [3, 8, 33])
def test_forward_equals_the_reference(nlat):
    f, conv = gc.fixture(), converter(nlat)
    x = torch.from_numpy(f[f"n{nlat}_x"])
    assert torch.equal(conv(x), torch.from_numpy(f[f"n{nlat}_y"]))
    # 5-D input, and shards on their slab of source rows
    x5 = torch.stack([x, x + 1.0])
    y5 = conv(x5)
    assert y5.shape == (2, 2, 3, nlat, 2 * nlat) and torch.equal(y5[0], conv(x))
    for k0, k1 in ((0, nlat // 2), (nlat // 2, nlat), (1, nlat - 1)):
        s0, s1 = conv.source_rows(k0, k1)
        assert s1 - s0 <= (k1 - k0) + 2
        assert torch.equal(conv(x5[..., s0:s1, :], dst_rows=(k0, k1), src_row0=s0), y5[..., k0:k1, :])


def test_normalisation_out_and_dtype_on_the_cpu():
    f, conv = gc.fixture(), converter(8)
    x = torch.from_numpy(f["n8_x"])
    bias, scale = torch.from_numpy(gc.BIAS).reshape(1, 3, 1, 1), torch.from_numpy(gc.SCALE).reshape(1, 3, 1, 1)
    want = conv((x - bias) / scale)
    assert torch.equal(conv(x, bias=bias, scale=scale), want)
    buf = torch.full((2, 5, 8, 16), -77.0, dtype=torch.bfloat16)
    got = conv(x, bias=bias, scale=scale, out=buf[:, 1:4])
    assert got.data_ptr() == buf[:, 1:4].data_ptr() and torch.equal(buf[:, 1:4], want.bfloat16())
    assert bool((buf[:, 0] == -77.0).all()) and bool((buf[:, 4] == -77.0).all())
    # bf16 data: widened, blended with the fp32 weights, rounded once
    xb = x.bfloat16()
    assert torch.equal(conv(xb), conv(xb.float()).bfloat16())
    assert conv(x.double()).dtype == torch.float64
    with pytest.raises(ValueError):
        conv(x, bias=bias)
    with pytest.raises(ValueError):
        conv(x[..., :7, :])


def test_identity_unsupported_and_invalid():
    lat = torch.deg2rad(torch.linspace(90.0, -90.0, 5))
    x = torch.randn(2, 5, 10)
    same = GridConverter(EQ, EQ, lat, lat)
    assert same(x) is x and same.dst_lat is lat and same.dst_lon is lat
    with pytest.raises(NotImplementedError):
        GridConverter(LG, EQ, lat, lat)
    with pytest.raises(ValueError, match="descend"):
        GridConverter(EQ, LG, torch.flip(lat, [0]), lat)
    with pytest.raises(ValueError):
        GridConverter(EQ, LG, torch.tensor([1.0, 0.5, 0.4, 0.3, 0.2]), lat)      # the southern nodes lie below the last row


def test_lat_interp_tables_rejects_rows_outside_the_slab():
    for idx, n, s0 in (([0, 3], 4, 0), ([-1, 0], 4, 0), ([2, 3], 4, 3), ([5], 3, 3)):
        with pytest.raises(ValueError, match="leave the slab"):
            ops.lat_interp_tables(np.array(idx), np.full(len(idx), 0.5), n, src_row0=s0)
    with pytest.raises(ValueError):
        ops.lat_interp_tables(np.array([0]), np.array([np.nan]), 4)
    with pytest.raises(ValueError):
        ops.lat_interp_tables(np.array([0]), np.array([0.5]), 1)
    t = ops.lat_interp_tables(np.array([3, 4]), np.array([0.25, 0.5]), 3, src_row0=3)
    assert t.idx.tolist() == [0, 1] and t.idx.dtype == torch.int32 and t.wgt.dtype == torch.float32


def test_switch_is_validated_on_every_call(monkeypatch):
    conv = converter(3)
    x = torch.from_numpy(gc.fixture()["n3_x"])
    assert "MK_GRID" in ops.KNOBS and ops.GRID_DEFAULT in ops.KNOBS["MK_GRID"]
    monkeypatch.setenv("MK_GRID", "bogus")
    with pytest.raises(ValueError, match=r"unknown MK_GRID 'bogus' \(hip \| torch\)"):
        conv(x)
    monkeypatch.setenv("MK_GRID", "hip")          # CPU tensors take the torch formulation whatever the switch says
    assert torch.equal(conv(x), torch.from_numpy(gc.fixture()["n3_y"]))


def test_signatures_are_pinned():
    ll, i, p = ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p
    assert _lib.SIGNATURES["mk_lat_lerp_fwd"] == (i, [p, i, ll, ll, p, i, ll, ll, p, p, p, p, i, ll, i, i, i, p])
    assert _lib.SIGNATURES["mk_lat_lerp_bwd"] == (i, [p, i, ll, ll, p, i, ll, ll, p, p, p, p, i, ll, i, i, i, p])
    assert _lib.SIGNATURES["mk_lat_lerp_chunk"] == (i, [])


@pytest.mark.parametrize("name", gc.TABLES + ["conv721"])
def test_csr_transpose_equals_the_transposed_matrix(name):
    idx, w, hs = gc.table(name)
    t = ops.lat_interp_tables(idx, w, hs)
    w32 = w.astype(np.float32)
    dense32 = np.zeros((len(idx), hs))
    for k, i in enumerate(idx):                               # 1 - w and w, each rounded once from float64
        dense32[k, i] += float(np.float32(1.0 - w[k]))
        dense32[k, i + 1] += float(w32[k])
    got, terms = gc.csr_to_dense(t)
    assert np.array_equal(got, dense32.T)
    assert np.array_equal(terms, np.bincount(np.concatenate([idx, idx + 1]), minlength=hs)) and int(terms.sum()) == 2 * len(idx)
    assert np.abs(got - gc.dense_matrix(idx, w, hs).T).max() <= 2.0 ** -23
    # per source row: ascending destination rows, the a-term of a row before its b-term
    rp, tr = t.rowptr.numpy(), t.term_row.numpy()
    assert rp[0] == 0 and rp[-1] == 2 * len(idx) and t.rowptr.dtype == t.term_row.dtype == torch.int32
    for j in range(hs):
        assert (np.diff(tr[rp[j]:rp[j + 1]]) >= 0).all()


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "norm"])
@pytest.mark.parametrize("name", ["conv33", "nonmono", "extrap"])
def test_autograd_of_the_torch_formulation_is_the_transpose(name, norm):
    idx, w, hs = gc.table(name)
    t = ops.lat_interp_tables(idx, w, hs)
    P, W = 6, 5
    x = torch.from_numpy(gc.field((2, 3, hs, W), 5)).requires_grad_(True)
    gy = gc.field((P, len(idx), W), 6)
    bias, scale = (torch.from_numpy(gc.BIAS), torch.from_numpy(gc.SCALE)) if norm else (None, None)
    y = ops.lat_interp(x, t, bias=bias, scale=scale)
    y.backward(torch.from_numpy(gy).reshape(y.shape))
    ref, bound, terms = gc.backward_reference(gy, idx, w, hs, norm)
    got = x.grad.reshape(P, hs, W)
    gc.assert_within(got, ref, bound, torch.float32, f"{name} norm={norm}")
    assert bool((got[:, terms == 0] == 0).all())


def _params(**kw):
    H, W = 5, 8
    f = gc.fixture()
    p = dict(n_history=0, history_normalization_mode="none", history_normalization_decay=0.5, target="default",
             normalize_residual=False, img_shape_x=H, img_shape_y=W, img_local_offset_x=0, img_local_offset_y=0,
             img_local_shape_x=H, img_local_shape_y=W, add_grid=True, gridtype="sinusoidal", grid_num_frequencies=2,
             data_grid_type=EQ, model_grid_type=LG, add_orography=False, add_landmask=False, n_future=0, lat=f["pre_lat"],
             lon=f["pre_lon"])
    p.update(kw)
    return SimpleNamespace(**p)


def test_preprocessor_grid_features_are_opt_in():
    pp = Preprocessor2D(_params(allow_grid_conversion=True))
    want = torch.from_numpy(gc.fixture()["pre_static"])
    assert pp.static_features.dtype == want.dtype and torch.equal(pp.static_features, want)
    for p in (_params(), _params(allow_grid_conversion=False)):
        with pytest.raises(NotImplementedError, match="allow_grid_conversion"):
            Preprocessor2D(p)
    same = Preprocessor2D(_params(model_grid_type=EQ, allow_grid_conversion=True))
    assert not torch.equal(same.static_features, want)


_A = capi.A


def _fwd_args(**kw):
    a = dict(x=_A, xdtype=0, xps=40, xrs=8, y=_A, ydtype=0, yps=40, yrs=8, idx=_A, wgt=_A, bias=None, scale=None, C=3, P=6, Hs=5,
             Hd=5, W=8)
    a.update(kw)
    return tuple(a.values())


def _bwd_args(**kw):
    a = dict(gy=_A, gydtype=0, gyps=40, gyrs=8, gx=_A, gxdtype=0, gxps=40, gxrs=8, rowptr=_A, trow=_A, tcoef=_A, scale=None, C=3, P=6,
             Hs=5, Hd=5, W=8)
    a.update(kw)
    return tuple(a.values())


REFUSED = [
    ("mk_lat_lerp_fwd", _fwd_args(x=None), "null pointer"),
    ("mk_lat_lerp_fwd", _fwd_args(idx=None), "null table pointer"),
    ("mk_lat_lerp_fwd", _fwd_args(wgt=_A + 2), "a table is not 4-byte aligned"),
    ("mk_lat_lerp_fwd", _fwd_args(scale=_A), "bias and scale come together"),
    ("mk_lat_lerp_fwd", _fwd_args(xdtype=2), "dtype must be 0 (fp32) or 1 (bf16)"),
    ("mk_lat_lerp_fwd", _fwd_args(ydtype=-1), "dtype must be 0 (fp32) or 1 (bf16)"),
    ("mk_lat_lerp_fwd", _fwd_args(Hs=1), "Hs below 2: a destination row blends two source rows"),
    ("mk_lat_lerp_fwd", _fwd_args(W=0), "bad sizes"),
    ("mk_lat_lerp_fwd", _fwd_args(yrs=7), "a row stride below W"),
    ("mk_lat_lerp_fwd", _fwd_args(yps=39), "planes of the output overlap"),
    ("mk_lat_lerp_fwd", _fwd_args(x=_A + 2), "a field is not aligned to its element"),
    ("mk_lat_lerp_fwd", _fwd_args(ydtype=1, y=_A + 1), "a field is not aligned to its element"),
    ("mk_lat_lerp_bwd", _bwd_args(gx=None), "null pointer"),
    ("mk_lat_lerp_bwd", _bwd_args(tcoef=None), "null table pointer"),
    ("mk_lat_lerp_bwd", _bwd_args(rowptr=_A + 1), "a table is not 4-byte aligned"),
    ("mk_lat_lerp_bwd", _bwd_args(gxdtype=2), "dtype must be 0 (fp32) or 1 (bf16)"),
    ("mk_lat_lerp_bwd", _bwd_args(Hs=1), "Hs below 2: a destination row blends two source rows"),
    ("mk_lat_lerp_bwd", _bwd_args(W=-1), "bad sizes"),
    ("mk_lat_lerp_bwd", _bwd_args(gxps=39), "planes of the output overlap"),
]


@pytest.mark.parametrize("case", REFUSED, ids=capi.case_ids(REFUSED))
def test_bad_argument_is_refused_before_any_launch(case):
    capi.assert_refused(*case)
