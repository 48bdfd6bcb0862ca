"""CPU tests of the ensemble forecast products: the checker of tests/ens_products_checks.py against numpy's own quantile and
against planted errors, the torch formulation of ``ops.ensemble_products`` against that checker, ``quantile_position``, the
``EnsembleProducts`` module, ``EnsembleRollout.run(products=...)`` against the module applied by hand, and the refusals of
``mk_ens_products``."""
import numpy as np
import pytest
import torch

import capi_checks as capi
import ens_checks as ec
import ens_products_checks as pc
from test_rollout_cpu import C, build, make_params, make_problem

ids = lambda s: "x".join(map(str, s))


def run_op(ens, table, dtype="float32", out_dtype=torch.float32, **kw):
    """``ops.ensemble_products`` on CPU tensors made of numpy inputs; returns fp32 numpy."""
    from makani_amd import ops
    t = torch.from_numpy(np.array(ens)).to(getattr(torch, dtype))
    kw = {k: (torch.from_numpy(np.asarray(v, dtype=np.float32)) if k in ("thr", "scale", "shift") and v is not None else v)
          for k, v in kw.items()}
    out = ops.ensemble_products(t, *table, out_dtype=out_dtype, **kw)
    assert out.dtype == out_dtype
    return out.float().numpy()


# ---------------------------------------------------------------------------- the checker
def test_reference_order_statistic_is_numpys_linear_quantile():
    """The float64 order statistic of the reference against ``np.quantile(..., method="linear")`` within ``2^-51 |r|``, on the
    temperature-like channel (offset 250)."""
    worst = 0.0
    for E in (2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 50, 64):
        ens, _, _ = ec.problem((1, E, 1, 5, 8))
        for q in (0.0, 0.1, 0.25, 0.5, 0.9, 0.99, 1.0):
            k, t = pc.quantile_position(q, E)
            (p,) = pc.reference(ens, ([pc.ORDER], [k], [t]))
            want = np.quantile(ens.astype(np.float64), q, axis=1, method="linear")
            rel = float((np.abs(p.want.astype(np.float64) - want) / np.abs(want)).max())
            worst = max(worst, rel)
            assert rel <= 2.0 ** -51, (E, q, rel)
    print(f"worst relative difference to np.quantile: {worst:.3e}")


def _planted_problem():
    """Integer-valued members with ties, thresholds equal to members, one NaN point, one point of equal members."""
    rng = np.random.default_rng(5)
    ens = rng.integers(-3, 4, size=(2, 5, 2, 3, 7)).astype(np.float32) + np.float32(250.0)
    ens[0, 2, 1, 1, 3] = np.nan
    ens[1, :, 0, 2, 2] = 251.0
    E = ens.shape[1]
    table = ([pc.MEAN, pc.STD, pc.ORDER, pc.ORDER, pc.ABOVE, pc.BELOW], [0, 0, 1, 1, 0, 0], [0.0, 0.0, 0.0, 0.375, 0.0, 0.0])
    thr = np.full((6, 2), 250.0, dtype=np.float32)
    return ens, table, thr, E


def test_the_checker_accepts_its_own_reference_and_rejects_planted_errors():
    ens, table, thr, E = _planted_problem()
    planes = pc.reference(ens, table, thr=thr)
    good = np.stack([p.want.astype(np.float32) for p in planes], axis=1)
    pc.assert_products(good, planes, "its own values")
    assert (ens == 250.0).any(axis=1).mean() > 0.3                  # the premise of the tie cases
    x = np.sort(ens, axis=1)
    x64 = ens.astype(np.float64)
    with np.errstate(invalid="ignore"):
        m = x64.sum(axis=1) / E
        planted = {
            "x_(k+1) for x_(k)": (2, x[:, 2]),
            "x_(k+1) for x_(k) under a fraction": (3, (x[:, 2] + 0.375 * (x[:, 3].astype(np.float64) - x[:, 2])).astype(np.float32)),
            "variance divided by E": (1, np.sqrt(((x64 - m[:, None]) ** 2).sum(axis=1) / E).astype(np.float32)),
            ">= for > at ties": (4, ((ens >= 250.0).sum(axis=1) / np.float32(E)).astype(np.float32)),
            "a member left out of the mean": (0, (x64[:, 1:].sum(axis=1) / (E - 1)).astype(np.float32)),
            "a NaN point not propagated": (0, np.nan_to_num(good[:, 0], nan=250.0)),
            "scale applied to a count plane": (5, good[:, 5] * np.float32(1.5)),
        }
    for what, (i, plane) in planted.items():
        bad = good.copy()
        bad[:, i] = np.where(np.isnan(good[:, i]) & (what != "a NaN point not propagated"), np.nan, plane)
        with pytest.raises(AssertionError):
            pc.assert_products(bad, planes, what)


def test_affine_and_bf16_helpers():
    plain = np.array([[[[[1.5, -2.0]]], [[[0.25, 0.5]]], [[[0.4, 0.6]]]]], dtype=np.float32)         # [1, 3, 1, 1, 2]
    out = pc.affine(plain, [pc.MEAN, pc.STD, pc.ABOVE], [2.0], [10.0])
    assert out[0, :, 0, 0].tolist() == [[13.0, 6.0], [0.5, 1.0], [np.float32(0.4), np.float32(0.6)]]
    assert pc.as_bf16(np.array([1.00390625, 1.01171875], dtype=np.float32)).tolist() == [1.0, 1.015625]     # ties to even


# ---------------------------------------------------------------------------- quantile_position
def test_quantile_position_edge_cases():
    from makani_amd import ops
    assert ops.quantile_position(0.0, 5) == (0, 0.0) and ops.quantile_position(1.0, 5) == (4, 0.0)
    assert ops.quantile_position(1.0, 1) == (0, 0.0) and ops.quantile_position(0.3, 1) == (0, 0.0)
    assert ops.quantile_position(0.5, 2) == (0, 0.5) and ops.quantile_position(0.0, 2) == (0, 0.0) and ops.quantile_position(1.0, 2) == (1, 0.0)
    assert ops.quantile_position(0.25, 5) == (1, 0.0) and ops.quantile_position(0.5, 9) == (4, 0.0)     # q (E - 1) an integer
    k, t = ops.quantile_position(0.1, 50)
    assert k == 4 and t == 0.1 * 49 - 4 and isinstance(k, int) and isinstance(t, float)
    for E in (2, 3, 17, 50, 64):
        for q in (0.0, 0.1, 0.25, 0.5, 0.9, 0.99, 1.0):
            k, t = ops.quantile_position(q, E)
            assert (k, t) == pc.quantile_position(q, E) and 0 <= k <= E - 1 and 0.0 <= t < 1.0 and (t == 0.0 or k <= E - 2)
    for q, E in ((-0.1, 4), (1.5, 4), (0.5, 0)):
        with pytest.raises(ValueError, match="quantile_position"):
            ops.quantile_position(q, E)


# ---------------------------------------------------------------------------- the torch formulation
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("shape", [(2, 3, 2, 3, 5), (1, 5, 3, 5, 8), (2, 8, 2, 17, 20), (1, 17, 2, 5, 33), (1, 64, 1, 3, 9)], ids=ids)
def test_torch_formulation_is_within_the_bounds_of_the_reference(shape, dtype):
    ens, _, _ = ec.problem(shape, dtype)
    E, Cn = shape[1], shape[2]
    table = pc.table7(E)
    thr = pc.thresholds(ens, 7)
    plain = run_op(ens, table, dtype, thr=thr)
    pc.assert_products(plain, pc.reference(ens, table, thr=thr), f"torch {ids(shape)} {dtype}")
    scale, shift = np.linspace(0.5, 3.0, Cn, dtype=np.float32), np.linspace(-7.0, 280.0, Cn, dtype=np.float32)
    scaled = run_op(ens, table, dtype, thr=thr, scale=scale, shift=shift)
    pc.assert_same_bits(scaled, pc.affine(plain, table[0], scale, shift), "scale and shift")
    pc.assert_same_bits(run_op(ens, table, dtype, torch.bfloat16, thr=thr), pc.as_bf16(plain), "bf16")


def test_channel_selection_repeats_and_out_argument():
    from makani_amd import ops
    ens, _, _ = ec.problem((2, 5, 3, 5, 8))
    table = pc.table7(5)
    for chans in ([2, 0], [1, 1]):
        thr = pc.thresholds(ens, 7, chans)
        got = run_op(ens, table, chans=chans, thr=thr)
        pc.assert_products(got, pc.reference(ens, table, chans, thr), f"chans {chans}")
        poisoned = np.array(ens)
        poisoned[:, :, [c for c in range(3) if c not in chans]] = np.nan
        assert np.array_equal(pc.bits(run_op(poisoned, table, chans=chans, thr=thr)), pc.bits(got))
        as_tensor = run_op(ens, table, chans=torch.tensor(chans, dtype=torch.int32), thr=thr)
        assert np.array_equal(pc.bits(as_tensor), pc.bits(got))
    # out= a slice of a larger buffer: the bytes between the blocks stay
    thr = pc.thresholds(ens, 7)
    big = torch.full((2, 9, 4, 5, 8), -5.0)
    out = big[:, 1:8, :3]
    res = ops.ensemble_products(torch.from_numpy(np.array(ens)), *table, thr=torch.from_numpy(thr), out=out)
    assert res is out and np.array_equal(pc.bits(out.numpy()), pc.bits(run_op(ens, table, thr=thr)))
    assert bool((big[:, 0] == -5).all()) and bool((big[:, 8] == -5).all()) and bool((big[:, :, 3] == -5).all())


def test_ties_thresholds_equal_to_members_equal_members_and_nan():
    ens, table, thr, E = _planted_problem()
    got = run_op(ens, table, thr=thr)
    planes = pc.reference(ens, table, thr=thr)
    pc.assert_products(got, planes, "planted")
    assert np.isnan(got[0, :, 1, 1, 3]).all() and np.isnan(got).sum() == 6            # the NaN point, in all K planes, only there
    assert got[1, 0, 0, 2, 2] == 251.0 and pc.bits(got[1, 1, 0, 2, 2]) == 0              # equal members: m = x, spread +0
    assert got[1, 4, 0, 2, 2] == 1.0 and got[1, 5, 0, 2, 2] == 0.0
    tie = (ens == 250.0).sum(axis=1)[1, 1]                                              # a tie counts for neither side
    assert np.array_equal(np.rint(got[1, 4, 1] * E) + np.rint(got[1, 5, 1] * E) + tie, np.full(tie.shape, E))
    thr[4, 1] = np.nan                                                                  # a NaN threshold: a NaN plane, only that one
    got = run_op(ens, table, thr=thr)
    assert np.isnan(got[:, 4, 1]).all() and not np.isnan(got[:, 4, 0]).all() and not np.isnan(got[1, 5, 1]).any()
    pc.assert_products(got, pc.reference(ens, table, thr=thr), "NaN threshold")


def test_device_independent_paths_one_member_seventeen_products_and_the_knob(monkeypatch):
    from makani_amd import ops
    ens, _, _ = ec.problem((2, 1, 2, 3, 5))
    one = run_op(ens, ([pc.MEAN, pc.STD, pc.ORDER, pc.ABOVE], [0, 0, 0, 0], [0.0] * 4), thr=np.zeros((4, 2), dtype=np.float32))
    assert np.array_equal(pc.bits(one[:, 0]), pc.bits(ens[:, 0])) and np.array_equal(pc.bits(one[:, 2]), pc.bits(ens[:, 0]))
    assert np.isnan(one[:, 1]).all() and np.array_equal(one[:, 3], (ens[:, 0] > 0).astype(np.float32))
    ens, _, _ = ec.problem((1, 5, 3, 5, 8))
    table = ([pc.ORDER] * 17, [i % 5 for i in range(17)], [0.0] * 17)
    many = run_op(ens, table)
    assert many.shape == (1, 17, 3, 5, 8)
    pc.assert_products(many, pc.reference(ens, table), "K = 17")
    assert "MK_ENS_PRODUCTS" in ops.KNOBS and ops.ENS_PRODUCTS_DEFAULT in ops.KNOBS["MK_ENS_PRODUCTS"]
    assert ops.ENS_PRODUCTS_MAX == 16 and ops.ENS_PRODUCT_KINDS == ("mean", "std", "order", "above", "below")
    monkeypatch.setenv("MK_ENS_PRODUCTS", "torch")
    named = run_op(ens, (["order"] * 17, table[1], table[2]))
    assert np.array_equal(pc.bits(named), pc.bits(many))
    monkeypatch.setenv("MK_ENS_PRODUCTS", "bogus")
    with pytest.raises(ValueError, match="MK_ENS_PRODUCTS"):
        run_op(ens, table)


def test_bad_arguments_are_refused():
    from makani_amd import ops
    x = torch.zeros(2, 4, 3, 5, 8)
    for table, kw, msg in [
        (([0], [0], [0.0]), dict(ens=x[0]), r"must be \[B, E, C, H, W\]"),
        (([7], [0], [0.0]), {}, "unknown kind"),
        (([0, 1], [0], [0.0, 0.0]), {}, "one of each per product"),
        (([2], [4], [0.0]), {}, "rank 4"),
        (([2], [3], [0.5]), {}, "rank 3"),
        (([2], [0], [1.0]), {}, "fraction 1.0"),
        (([3], [0], [0.0]), {}, "needs thr"),
        (([3], [0], [0.0]), dict(thr=torch.zeros(1, 2)), "needs thr"),
        (([0], [0], [0.0]), dict(chans=[3]), "out of range"),
        (([0], [0], [0.0]), dict(scale=torch.ones(3)), "come together"),
        (([0], [0], [0.0]), dict(scale=torch.ones(2), shift=torch.ones(2)), "needs Cs = 3"),
        (([0], [0], [0.0]), dict(out=torch.zeros(2, 1, 3, 5, 7)), "out"),
    ]:
        kw = dict(kw)
        with pytest.raises(ValueError, match=msg):
            ops.ensemble_products(kw.pop("ens", x), *table, **kw)
    y = torch.randn(2, 4, 3, 5, 8, requires_grad=True)
    assert not ops.ensemble_products(y, [0], [0], [0.0]).requires_grad


# ---------------------------------------------------------------------------- the module
def test_module_names_table_and_threshold_conversion():
    from makani_amd import ops
    from makani_amd.ensemble import EnsembleProducts
    E = 5
    means, stds = [250.0, 1.0, -3.0], [2.0, 0.5, 10.0]
    specs = ["mean", "std", "min", "max", "median", ("quantile", 0.1), ("above", 252.0), ("below", {0: 249.0, 2: -1.0})]
    mod = EnsembleProducts(E, specs, stats=(means, stds))
    assert mod.names == ["mean", "std", "min", "max", "median", "q0.1", "above_252", "below"]
    k10, t10 = ops.quantile_position(0.1, E)
    assert mod.table == ([0, 1, 2, 2, 2, 2, 3, 4], [0, 0, 0, E - 1, 2, k10, 0, 0], [0.0, 0.0, 0.0, 0.0, 0.0, t10, 0.0, 0.0])
    thr = mod.thresholds(3).numpy()
    want6 = ((np.float64(252.0) - np.array(means)) / np.array(stds)).astype(np.float32)
    assert thr.dtype == np.float32 and thr.shape == (8, 3) and np.array_equal(thr[6], want6)
    assert thr[7, 0] == np.float32((249.0 - 250.0) / 2.0) and np.isnan(thr[7, 1]) and thr[7, 2] == np.float32((-1.0 + 3.0) / 10.0)
    assert np.isnan(thr[:6]).all()
    # thresholds in the members' units are taken as they are; without statistics there is nothing to convert
    assert EnsembleProducts(E, [("above", 0.5)], stats=(means, stds), thresholds_in="members").thresholds(3).tolist() == [[0.5] * 3]
    assert EnsembleProducts(E, [("above", 0.5)]).thresholds(2).tolist() == [[0.5] * 2]
    ens, _, _ = ec.problem((2, E, 3, 5, 8))
    x = torch.from_numpy(np.array(ens))
    got = mod(x)
    assert got.shape == (2, 8, 3, 5, 8) and got.dtype == torch.float32
    plain = ops.ensemble_products(x, *mod.table, thr=torch.from_numpy(thr)).numpy()
    pc.assert_same_bits(got.numpy(), pc.affine(plain, mod.table[0], stds, means), "module")
    assert np.isnan(got[:, 7, 1].numpy()).all() and not np.isnan(got[:, 7, 0].numpy()).any()      # a channel without a value
    pc.assert_same_bits(mod(x.reshape(2 * E, 3, 5, 8)).numpy(), got.numpy())                                    # the model's [B * E, C, H, W]
    assert mod._device_tables(x.device, 3) is mod._device_tables(x.device, 3)                    # uploaded once
    sel = EnsembleProducts(E, ["max", ("below", {2: -1.0})], channels=[2, 0], stats=([-3.0, 250.0], [10.0, 2.0]), out_dtype=torch.bfloat16)
    got = sel(x)
    assert got.shape == (2, 2, 2, 5, 8) and got.dtype == torch.bfloat16 and np.isnan(got[:, 1, 1].float().numpy()).all()
    assert torch.equal(got[:, 0, 0], (x[:, :, 2].max(dim=1).values * 10.0 - 3.0).bfloat16())
    for bad in (dict(stats=(means, [1.0, 0.0, 1.0])), dict(stats=(means, [1.0, -2.0, 1.0])), dict(thresholds_in="physical"),
                dict(channels=[0, 1], stats=(means, stds)), dict(products=["mode"]), dict(products=[]), dict(members=0)):
        kw = dict(dict(members=E, products=["mean"]), **bad)
        with pytest.raises(ValueError, match="EnsembleProducts"):
            EnsembleProducts(**kw)
    with pytest.raises(ValueError, match="must be"):
        mod(torch.zeros(2, E + 1, 3, 5, 8))


# ---------------------------------------------------------------------------- the rollout
def test_rollout_products_are_the_module_applied_to_each_steps_members(tmp_path):
    from makani_amd.ensemble import EnsembleProducts, EnsembleScores
    from makani_amd.inference import EnsembleRollout
    H, W, B, steps, E = 12, 24, 2, 3, 4
    params = make_params(H, W, tmp_path, steps=steps, n_history=0, history_normalization_mode="none", masked_channels=[1])
    params.noise_std = 0.25
    prob = make_problem(B, 1, H, W, steps, seed=3)
    mod = EnsembleProducts(E, ["mean", "std", "median", ("quantile", 0.9), ("above", 0.1)], channels=[2, 0],
                           stats=([1.0, -2.0], [3.0, 0.5]))
    res = {}
    for with_products in (False, True):
        wrap, _, _ = build(params, prob)
        sc = EnsembleScores(params, E, "cpu")
        ro = EnsembleRollout(params, wrap, sc, E)
        assert ro.last_products is None
        out = ro.run(prob.inp, prob.tar, generator=torch.Generator().manual_seed(11), output_channels=list(range(C)),
                     products=mod if with_products else None)
        res[with_products] = (out, sc, ro.last_products)
    members, _, planes = res[True]
    assert res[False][2] is None and planes.shape == (steps, B, 5, 2, H, W) and planes.dtype == torch.float32
    for idt in range(steps):
        assert torch.equal(planes[idt], mod(members[idt])), idt          # the emitted members are pred itself (no statistics)
    assert torch.equal(res[True][0], res[False][0])                       # what run returns, and the scores, do not change
    for name in ("sums", "counter", "rank_histogram", "skipped"):
        assert torch.equal(getattr(res[True][1], name), getattr(res[False][1], name)), name
    wrap, _, _ = build(params, prob)
    with pytest.raises(ValueError, match="members"):
        EnsembleRollout(params, wrap, None, E).run(prob.inp, steps=1, products=EnsembleProducts(E + 1, ["mean"]))


# ---------------------------------------------------------------------------- the C ABI
def test_signature_row_and_source_list():
    import ctypes
    from makani_amd import _lib, build
    P, I, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert _lib.SIGNATURES["mk_ens_products"] == (I, [P, I, LL, LL, P, I, LL, LL, P, P, P, P, P, P, P, I, I, I, I, I, I, I, P])
    assert "ens_products.hip" in build.SOURCES and "ens_tile.h" in build.HEADERS
    assert hasattr(_lib.load(), "mk_ens_products")


_A = capi.A
_KINDS = np.array([0, 1, 2, 3], dtype=np.int32)
_ORDERS = np.array([0, 0, 1, 0], dtype=np.int32)
_FRACS = np.array([0.0, 0.0, 0.5, 0.0], dtype=np.float64)
_OK = dict(ens=_A, dtype=0, bstride=3 * 80, estride=80, out=_A, out_dtype=0, obstride=4 * 80, okstride=80, chans=None,
           kinds=_KINDS.ctypes.data, orders=_ORDERS.ctypes.data, fracs=_FRACS.ctypes.data, thr=_A, scale=None, shift=None,
           B=2, E=3, C=2, Cs=2, K=4, H=5, W=8)


def _args(**kw):
    return tuple(dict(_OK, **kw).values())


def _table(kinds, orders, fracs):
    """Host arrays that live as long as the module (the refusal reads them before it returns)."""
    arrays = (np.array(kinds, dtype=np.int32), np.array(orders, dtype=np.int32), np.array(fracs, dtype=np.float64))
    _table.keep.append(arrays)
    return dict(kinds=arrays[0].ctypes.data, orders=arrays[1].ctypes.data, fracs=arrays[2].ctypes.data, K=len(kinds))


_table.keep = []

REFUSED = [
    ("mk_ens_products", _args(out=None), "null pointer"),
    ("mk_ens_products", _args(kinds=None), "null pointer"),
    ("mk_ens_products", _args(out_dtype=2), "dtype and out_dtype must be 0 (fp32) or 1 (bf16)"),
    ("mk_ens_products", _args(E=1), "E outside 2 ... 64 (the members of a point are sorted in registers)"),
    ("mk_ens_products", _args(E=65, bstride=65 * 80), "E outside 2 ... 64 (the members of a point are sorted in registers)"),
    ("mk_ens_products", _args(K=0), "K outside 1 ... 16"),
    ("mk_ens_products", _args(K=17, obstride=17 * 80), "K outside 1 ... 16"),
    ("mk_ens_products", _args(Cs=1), "without a channel list Cs must equal C"),
    ("mk_ens_products", _args(W=0), "bad sizes"),
    ("mk_ens_products", _args(estride=79), "a member's [C][H][W] block must be contiguous: strides below C * H * W"),
    ("mk_ens_products", _args(okstride=79), "a product's [Cs][H][W] block must be contiguous: strides below Cs * H * W"),
    ("mk_ens_products", _args(chans=_A, Cs=3), "a product's [Cs][H][W] block must be contiguous: strides below Cs * H * W"),
    ("mk_ens_products", _args(bstride=239), "members of different samples overlap: need bstride >= E * estride or estride >= B * bstride"),
    ("mk_ens_products", _args(obstride=319), "products of different samples overlap: need obstride >= K * okstride or okstride >= B * obstride"),
    ("mk_ens_products", _args(ens=_A + 2), "ensemble or products not aligned to their element"),
    ("mk_ens_products", _args(out=_A + 1, out_dtype=1), "ensemble or products not aligned to their element"),
    ("mk_ens_products", _args(thr=_A + 2), "32-bit table not 4-byte aligned"),
    ("mk_ens_products", _args(scale=_A), "scale and shift come together or not at all"),
    ("mk_ens_products", _args(**_table([0, 5], [0, 0], [0.0, 0.0]), obstride=160), "product kind outside 0 ... 4"),
    ("mk_ens_products", _args(**_table([2], [3], [0.0]), obstride=80), "an order statistic's rank outside 0 ... E - 1 (E - 2 with a fraction)"),
    ("mk_ens_products", _args(**_table([2], [2], [0.25]), obstride=80), "an order statistic's rank outside 0 ... E - 1 (E - 2 with a fraction)"),
    ("mk_ens_products", _args(**_table([2], [0], [1.0]), obstride=80), "an order statistic's fraction must lie in [0, 1)"),
    ("mk_ens_products", _args(**_table([2], [0], [float("nan")]), obstride=80), "an order statistic's fraction must lie in [0, 1)"),
    ("mk_ens_products", _args(thr=None), "a count product needs thresholds"),
]


@pytest.mark.parametrize("case", REFUSED, ids=capi.case_ids(REFUSED))
def test_bad_argument_is_refused_before_any_launch(case):
    capi.assert_refused(*case)
