"""GPU tests of csrc/ens_products.hip through the C ABI (members between NaN bands and compared bit for bit afterwards, outputs
between sentinel bands, both sides 0 and 1 element past a 16-byte boundary), of ``ops.ensemble_products`` and
``EnsembleProducts`` on the device and of ``EnsembleRollout.run(products=...)`` on a small SFNO.  Every plane is held to the
bounds and equalities of tests/ens_products_checks.py against its numpy restatement, which the CPU tests hold to numpy's own
quantile and to planted errors first."""
import functools

import numpy as np
import pytest
import torch

import ens_checks as ec
import ens_products_checks as pc
import stream_checks as sc
from kernel_checks import SENTINEL, poisoned

pytestmark = pytest.mark.gpu

# (B, E, C, H, W), the shapes of tests/test_ens_gpu.py: one point; odd sizes; P = 8, 16, 32, 64 with and without pads; two slabs
# and several tiles (17 x 20, 33 x 64); a row longer than a tile at P = 64 (1441); samples whose alignments disagree (C H W = 27)
SHAPES = [(1, 2, 1, 1, 1), (2, 3, 2, 3, 5), (1, 5, 3, 5, 8), (2, 8, 2, 17, 20), (1, 16, 3, 33, 64), (1, 17, 2, 5, 33), (1, 33, 1, 3, 9),
          (1, 63, 1, 3, 9), (1, 64, 1, 2, 1441), (4, 4, 1, 3, 9)]
DTYPES = ["float32", "bfloat16"]
OUT_DTYPES = [torch.float32, torch.bfloat16]
ids = lambda s: "x".join(map(str, s))
oid = lambda d: str(d).split(".")[-1]


@functools.lru_cache(maxsize=None)
def case(shape, dtype):
    """The shared problem of a shape: members, the K = 7 table, its thresholds and the reference planes, computed once."""
    ens, _, _ = ec.problem(shape, dtype)
    table = pc.table7(shape[1])
    thr = pc.thresholds(ens, 7)
    thr.setflags(write=False)
    return ens, table, thr, pc.reference(ens, table, thr=thr)


def _device_members(ens, dtype, dev, offset, gap):
    """The members on the device as ``dtype`` between NaN bands; ``offset`` elements past a 16-byte boundary; ``gap`` NaN elements
    behind every member's block.  Returns (pointer, bstride, estride, unchanged) with ``unchanged()`` the bit-for-bit check."""
    B, E = ens.shape[:2]
    chw = int(np.prod(ens.shape[2:]))
    t = torch.from_numpy(np.array(ens)).to(getattr(torch, dtype)).reshape(B, E, chw)
    if gap:
        t = torch.cat([t, torch.full((B, E, gap), float("nan"), dtype=t.dtype)], dim=2)
    view, whole, flat = sc.put(t.reshape(-1), offset, dev)
    return view.data_ptr(), E * (chw + gap), chw + gap, lambda: sc.unchanged(whole, flat, "members")


def launch(dev, ens, table, dtype="float32", out_dtype=torch.float32, chans=None, thr=None, scale=None, shift=None, in_off=0,
           gap=0, out_off=0, out_gaps=(0, 0), keep=None):
    """One call of mk_ens_products on numpy inputs; returns the fp32 numpy ``[B, K, Cs, H, W]`` after checking the sentinel bands,
    the sentinels in the output's gaps (``out_gaps``: elements behind every product block, behind every sample) and that the
    members still hold their bits.  ``keep``: a dict that receives what a caller needs to launch again (a graph capture)."""
    from makani_amd import _lib
    lib = _lib.load()
    B, E, C, H, W = ens.shape
    kinds, orders, fracs = (np.asarray(a, dtype=t) for a, t in zip(table, (np.int32, np.int32, np.float64)))
    K, Cs = len(kinds), C if chans is None else len(chans)
    eptr, bstride, estride, unchanged = _device_members(ens, dtype, dev, in_off, gap)
    okstride = Cs * H * W + out_gaps[0]
    obstride = K * okstride + out_gaps[1]
    out, o_check = sc.out_at((B * obstride,), out_dtype, out_off, dev)
    dv = {name: None if a is None else poisoned(torch.from_numpy(np.array(a, dtype=np.float32)), dev)
          for name, a in (("thr", thr), ("scale", scale), ("shift", shift))}
    cd = None if chans is None else torch.tensor(list(chans), dtype=torch.int32, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()

    def call():
        _lib.check(lib.mk_ens_products(eptr, 0 if dtype == "float32" else 1, bstride, estride, out.data_ptr(), sc.code(out_dtype),
                                       obstride, okstride, ptr(cd), kinds.ctypes.data, orders.ctypes.data, fracs.ctypes.data,
                                       ptr(dv["thr"]), ptr(dv["scale"]), ptr(dv["shift"]), B, E, C, Cs, K, H, W, sc.stream()),
                   "mk_ens_products")

    def collect():
        torch.cuda.synchronize()
        o_check("products")
        unchanged()
        rows = out.cpu().view(B, obstride)
        blocks = rows[:, :K * okstride].reshape(B, K, okstride)
        gaps = torch.cat([blocks[:, :, Cs * H * W:].reshape(-1), rows[:, K * okstride:].reshape(-1)])
        assert torch.equal(sc.bits(gaps), sc.bits(torch.full_like(gaps, SENTINEL))), "a gap of the output was written"
        return blocks[:, :, :Cs * H * W].reshape(B, K, Cs, H, W).float().numpy()

    call()
    if keep is not None:
        keep.update(call=call, collect=collect, out=out, refs=(dv, cd, kinds, orders, fracs))
    return collect()


@pytest.mark.parametrize("out_dtype", OUT_DTYPES, ids=oid)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_products_within_the_bounds_at_every_alignment(dev, shape, dtype, out_dtype):
    ens, table, thr, planes = case(shape, dtype)
    plain = launch(dev, ens, table, dtype, thr=thr)
    pc.assert_products(plain, planes, f"{ids(shape)} {dtype}")
    want = plain if out_dtype == torch.float32 else pc.as_bf16(plain)
    for in_off in (0, 1):
        for out_off in (0, 1):
            got = launch(dev, ens, table, dtype, out_dtype, thr=thr, in_off=in_off, out_off=out_off)
            pc.assert_same_bits(got, want, f"{ids(shape)} {dtype} -> {oid(out_dtype)}, offsets {in_off} {out_off}")
    Cn = shape[2]
    scale, shift = np.linspace(0.5, 3.0, Cn, dtype=np.float32), np.linspace(-7.0, 280.0, Cn, dtype=np.float32)
    scaled = pc.affine(plain, table[0], scale, shift)
    got = launch(dev, ens, table, dtype, out_dtype, thr=thr, scale=scale, shift=shift, in_off=1)
    pc.assert_same_bits(got, scaled if out_dtype == torch.float32 else pc.as_bf16(scaled), f"{ids(shape)} scale and shift")


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_and_sixteen_products_of_two_members(dev, dtype):
    shape = (2, 2, 2, 17, 20)
    ens, _, _ = ec.problem(shape, dtype)
    one = ([pc.ORDER], [0], [0.625])
    pc.assert_products(launch(dev, ens, one, dtype, out_off=1), pc.reference(ens, one), f"K = 1 {dtype}")
    kinds = [pc.MEAN, pc.STD, pc.ORDER, pc.ORDER, pc.ORDER, pc.ABOVE, pc.BELOW, pc.ORDER] * 2
    table = (kinds, [0, 0, 0, 0, 1, 0, 0, 0] * 2, [0.0, 0.0, 0.0, 0.5, 0.0, 0.0, 0.0, 0.25] + [0.0, 0.0, 0.0, 0.75, 0.0, 0.0, 0.0, 0.999])
    thr = pc.thresholds(ens, 16, seed=1)
    got = launch(dev, ens, table, dtype, thr=thr, in_off=1)
    pc.assert_products(got, pc.reference(ens, table, thr=thr), f"K = 16 {dtype}")
    assert np.array_equal(pc.bits(got[:, 0]), pc.bits(got[:, 8])) and not np.array_equal(pc.bits(got[:, 5]), pc.bits(got[:, 13]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("chans", [[2, 0], [1, 1]], ids=ids)
def test_channel_list_in_any_order_with_repeats(dev, chans, dtype):
    shape = (1, 5, 3, 5, 8)
    ens, _, _ = ec.problem(shape, dtype)
    table = pc.table7(5)
    thr = pc.thresholds(ens, 7, chans)
    got = launch(dev, ens, table, dtype, chans=chans, thr=thr)
    pc.assert_products(got, pc.reference(ens, table, chans, thr), f"chans {chans} {dtype}")
    hidden = np.array(ens)
    hidden[:, :, [c for c in range(3) if c not in chans]] = np.nan      # a channel that is not selected is never read
    assert np.array_equal(pc.bits(launch(dev, hidden, table, dtype, chans=chans, thr=thr, in_off=1)), pc.bits(got))
    outside = launch(dev, ens, ([pc.MEAN, pc.ORDER], [0, 0], [0.0, 0.0]), dtype, chans=[1, 3])      # not a channel: NaN planes
    assert np.isnan(outside[:, :, 1]).all() and not np.isnan(outside[:, :, 0]).any()


@pytest.mark.parametrize("out_dtype", OUT_DTYPES, ids=oid)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 3, 2, 3, 5), (1, 16, 3, 33, 64), (1, 64, 1, 2, 1441)], ids=ids)
def test_gaps_between_members_are_not_read_and_gaps_of_the_output_not_written(dev, shape, dtype, out_dtype):
    """Five NaN elements behind every member's block (so the members' alignments disagree); three sentinel elements behind every
    product's block and seven more behind every sample (so the planes' alignments disagree)."""
    ens, table, thr, planes = case(shape, dtype)
    plain = launch(dev, ens, table, dtype, thr=thr)
    got = launch(dev, ens, table, dtype, out_dtype, thr=thr, gap=5, out_gaps=(3, 7))
    pc.assert_same_bits(got, plain if out_dtype == torch.float32 else pc.as_bf16(plain), f"gaps {ids(shape)} {dtype}")


@pytest.mark.parametrize("E", [4, 5, 33])
def test_ties_thresholds_equal_to_members_equal_members_and_nan_points(dev, E):
    rng = np.random.default_rng(E)
    ens = rng.integers(-2, 3, size=(2, E, 2, 5, 33)).astype(np.float32)
    ens[0, :, 0, 2, 5:9] = ens[0, :1, 0, 2, 5:9]                    # points of equal members
    ens[0, E - 1, 1, 4, 32] = ens[1, 0, 0, 0, 0] = np.nan           # NaN members: the last and the first element
    table = pc.table7(E)
    thr = np.array([[0.0, 1.0]] * 7, dtype=np.float32)              # thresholds that ARE members
    thr[6, 1] = np.nan                                              # and a NaN threshold: a NaN plane
    assert (ens == 0.0).any(axis=1)[:, 0].mean() >= 0.25            # the premise: at least a quarter of the points tie
    planes = pc.reference(ens, table, thr=thr)
    for dtype in DTYPES:                                            # small integers are bf16 values
        got = launch(dev, ens, table, dtype, thr=thr)
        pc.assert_products(got, planes, f"ties E = {E} {dtype}")
        assert np.isnan(got[0, :, 1, 4, 32]).all() and np.isnan(got[1, :, 0, 0, 0]).all() and np.isnan(got[:, 6, 1]).all()
        assert np.isnan(got).sum() == 2 * 7 + 2 * 5 * 33 - 1        # nowhere else
        assert not pc.bits(got[0, 1, 0, 2, 5:9]).any() and np.array_equal(got[0, 0, 0, 2, 5:9], ens[0, 0, 0, 2, 5:9])


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_slice_of_the_rows_gives_the_slice_of_the_planes(dev, dtype):
    shape = (1, 16, 3, 33, 64)
    ens, table, thr, _ = case(shape, dtype)
    full = launch(dev, ens, table, dtype, thr=thr)
    part = launch(dev, np.ascontiguousarray(ens[..., 5:20, :]), table, dtype, thr=thr)
    assert np.array_equal(pc.bits(part), pc.bits(full[..., 5:20, :]))


@pytest.mark.parametrize("shape", [(2, 8, 2, 17, 20), (1, 64, 1, 2, 1441)], ids=ids)
def test_runs_repeat_and_a_captured_launch_replays_to_the_eager_bits(dev, shape):
    ens, table, thr, _ = case(shape, "bfloat16")
    keep = {}
    eager = launch(dev, ens, table, "bfloat16", thr=thr, in_off=1, out_off=1, keep=keep)
    again = launch(dev, ens, table, "bfloat16", thr=thr, in_off=1, out_off=1)
    assert np.array_equal(pc.bits(again), pc.bits(eager))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep["call"]()
    for _ in range(2):
        keep["out"].fill_(SENTINEL)
        graph.replay()
        assert np.array_equal(pc.bits(keep["collect"]()), pc.bits(eager))


# ---------------------------------------------------------------------------- the op, the module and the rollout on the device
def _counted(monkeypatch):
    """``_lib.load`` wrapped so that every ``mk_ens_products`` call records whether the stream was capturing."""
    from makani_amd import _lib
    lib, calls = _lib.load(), []

    class Counted:
        def __getattr__(self, name):
            if name == "mk_ens_products":
                return lambda *a: calls.append(torch.cuda.is_current_stream_capturing()) or lib.mk_ens_products(*a)
            return getattr(lib, name)

    monkeypatch.setattr(_lib, "load", lambda: Counted())
    return calls


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 5, 3, 5, 8), (1, 16, 3, 33, 64), (1, 50, 2, 5, 33), (2, 64, 1, 3, 9)], ids=ids)
def test_op_on_the_device_against_the_torch_formulation(dev, monkeypatch, shape, dtype):
    """E = 50: counts over a divisor that is no power of two and no small one (torch divides by a python scalar on the device as
    a multiplication by the reciprocal, which is not the IEEE quotient; the formulation divides by a tensor)."""
    from makani_amd import ops
    calls = _counted(monkeypatch)
    ens, table, thr, planes = case(shape, dtype)
    B, E, Cn, H, W = shape
    x = torch.from_numpy(np.array(ens)).to(dev, getattr(torch, dtype))
    thr_d = torch.from_numpy(np.array(thr)).to(dev)
    scale, shift = np.linspace(0.5, 3.0, Cn, dtype=np.float32), np.linspace(-7.0, 280.0, Cn, dtype=np.float32)
    kw = dict(thr=thr_d, scale=torch.from_numpy(scale).to(dev), shift=torch.from_numpy(shift).to(dev))
    out = {}
    for mode in ("hip", "torch"):
        monkeypatch.setenv("MK_ENS_PRODUCTS", mode)
        plain = ops.ensemble_products(x, *table, thr=thr_d)
        assert plain.dtype == torch.float32 and plain.shape == (B, 7, Cn, H, W)
        pc.assert_products(plain.cpu().numpy(), planes, f"{mode} {ids(shape)} {dtype}")
        big = torch.full((B, 9, Cn + 1, H, W), SENTINEL, dtype=torch.bfloat16, device=dev)
        res = ops.ensemble_products(x, *table, out=big[:, 1:8, :Cn], **kw)           # a slice of a larger buffer
        assert res.data_ptr() == big[:, 1:8, :Cn].data_ptr()
        assert bool((big[:, 0] == SENTINEL).all()) and bool((big[:, 8] == SENTINEL).all()) and bool((big[:, :, Cn] == SENTINEL).all())
        pc.assert_same_bits(res.float().cpu().numpy(), pc.as_bf16(pc.affine(plain.cpu().numpy(), table[0], scale, shift)), mode)
        out[mode] = plain.cpu().numpy()
    assert calls == [False, False]                                    # the two hip calls, and only they, reached the kernel
    for i, p in enumerate(planes):
        if p.exact:
            pc.assert_same_bits(out["hip"][:, i], out["torch"][:, i], f"plane {i}")


def test_module_on_the_device_reads_a_strided_model_output(dev, monkeypatch):
    from makani_amd.ensemble import EnsembleProducts
    calls = _counted(monkeypatch)
    B, E, Cn, H, W = 2, 4, 3, 17, 20
    ens, _, _ = ec.problem((B, E, Cn, H, W), "bfloat16")
    wide = torch.full((B * E, Cn + 1, H, W), float("nan"), dtype=torch.bfloat16, device=dev)
    wide[:, :Cn] = torch.from_numpy(np.array(ens)).to(dev, torch.bfloat16).reshape(B * E, Cn, H, W)
    mod = EnsembleProducts(E, ["mean", "std", "min", "max", "median", ("quantile", 0.9), ("above", 251.0), ("below", {2: -1.0})],
                           channels=[2, 0], stats=([-3.0, 250.0], [10.0, 2.0]))
    res = {}
    for mode in ("hip", "torch"):
        monkeypatch.setenv("MK_ENS_PRODUCTS", mode)
        res[mode] = mod(wide[:, :Cn].view(B, E, Cn, H, W)).cpu().numpy()      # member blocks contiguous, strides with a gap
    assert calls == [False] and res["hip"].shape == (B, 8, 2, H, W)
    table, thr = mod.table, mod.thresholds(Cn).numpy()
    planes = pc.reference(ens, table, [2, 0], thr)
    plain = {}
    for mode in ("hip", "torch"):
        monkeypatch.setenv("MK_ENS_PRODUCTS", mode)
        from makani_amd import ops
        p = ops.ensemble_products(wide[:, :Cn].view(B, E, Cn, H, W), *table, chans=[2, 0], thr=torch.from_numpy(thr).to(dev))
        plain[mode] = p.cpu().numpy()
        pc.assert_products(plain[mode], planes, f"module table, {mode}")
        pc.assert_same_bits(res[mode], pc.affine(plain[mode], table[0], [10.0, 2.0], [-3.0, 250.0]), f"module, {mode}")
    assert np.isnan(res["hip"][:, 7, 1]).all() and not np.isnan(res["hip"][:, :7]).any()


def test_ensemble_rollout_products_of_the_package_sfno_captured_equals_eager(dev, tmp_path, monkeypatch):
    """Two steps of E = 4 members of a small package SFNO under bf16 autocast, with ``capture`` off and on: ``last_products`` is
    the module applied to the emitted members of the same run, bit for bit, from launches behind the step (or its replay)."""
    from makani_amd.ensemble import EnsembleProducts
    from makani_amd.inference import EnsembleRollout
    from test_rollout_cpu import C as CR, build, make_params, make_problem
    from test_stepper_gpu import _sfno
    monkeypatch.setenv("MK_ROLLOUT", "hip")
    monkeypatch.setenv("MK_ENS_PRODUCTS", "hip")
    H, W, B, steps, T, E = 64, 128, 2, 2, 2, 4
    params = make_params(H, W, tmp_path, steps=steps, n_history=T - 1, masked_channels=[1])
    params.noise_std = 0.1
    prob = make_problem(B, T, H, W, steps, seed=4)
    mod = EnsembleProducts(E, ["mean", "std", "min", "median", ("quantile", 0.9), "max", ("above", 0.5)], channels=[2, 0],
                           stats=([1.0, -2.0], [3.0, 0.5]), out_dtype=torch.bfloat16)
    calls = _counted(monkeypatch)
    res = {}
    for capture in (False, True):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            wrap, _, _ = build(params, prob, dev, model=_sfno(dev, T * (CR + 1) + 3, CR, H, W))
            ro = EnsembleRollout(params, wrap, None, E, capture=capture)
            members = ro.run(prob.inp.to(dev), steps=steps, generator=torch.Generator(device=dev).manual_seed(7),
                             output_channels=list(range(CR)), products=mod)
        planes = ro.last_products
        assert planes.shape == (steps, B, 7, 2, H, W) and planes.dtype == torch.bfloat16 and planes.is_pinned()
        n = len(calls)
        for idt in range(steps):
            want = mod(members[idt].to(dev)).float().cpu().numpy()          # the emitted members are pred, widened exactly
            pc.assert_same_bits(planes[idt].float().numpy(), want, f"capture {capture}, step {idt}")
        del calls[n:]
        assert bool((planes[:, :, 2].float() <= planes[:, :, 5].float()).all()) and bool((planes[:, :, 1] > 0).any())
        res[capture] = (members, planes)
    assert calls == [False] * (2 * steps)
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(sc.bits(res[True][1]), sc.bits(res[False][1]))
