"""The optimizer kernels (csrc/optim.hip, csrc/adam.hip) held to the three criteria of tests/kernel_checks.py through the C ABI:
``mk_mt_sumsq``, ``mk_mt_norm_finish``, ``mk_mt_step_inc``, ``mk_mt_scale``, ``mk_mt_adam``, ``mk_mt_lamb`` and ``mk_adam_step``.

EVERY element of p, m and v after ONE launch from a random non-zero state is bounded against the float64 restatement of
tests/optim_checks.py (bounds derived there, checked against an fp32 emulation in tests/test_optim_checks_cpu.py); every written
stream is a guarded buffer of its own, every read-only stream sits between NaN bands and must come back bit for bit
(``optim_checks.build_list``).  The tensors of one list get different step counts and visibly different norms, so an indexing
error changes values.  Shapes: the edges of ``walk`` (lengths around the float4 body and the 16384-real chunk, at every common
offset, with mixed offsets, with only the gradient offset), lists longer than one argument block (89 / 181 / 241 tensors), the
unfused finalize, a step table whose slots are not in list order, every LAMB switch, and one grid-stride pass per kernel.

Worst error / bound seen on an MI355X (records, not limits) are in DESIGN.md, section 42.
"""
import numpy as np
import pytest
import torch

import optim_checks as oc
from kernel_checks import SENTINEL, guarded, poisoned

pytestmark = pytest.mark.gpu

F = np.float32
H = dict(lr=oc.f32(1e-2), beta1=oc.f32(0.9), beta2=oc.f32(0.95), eps=oc.f32(1e-8), wd=oc.f32(0.1))
LAMB_EPS, BETA3 = oc.f32(1e-6), oc.f32(1.0 - oc.f32(0.9))
COEF = oc.f32(0.37)
EDGE = (1, 2, 3, 4, 5, 7, 16383, 16384, 16385, 2 * 16384 + 5)
BIG = 2 * 16384 + 5                                      # 3 chunks
OFFSETS = {"off0": (0, 0, 0, 0), "off1": (1, 1, 1, 1), "off2": (2, 2, 2, 2), "off3": (3, 3, 3, 3), "mixed": (0, 1, 2, 3),
           "rotated": (2, 3, 0, 1), "g-only": (0, 1, 0, 0)}
PGMV_READONLY = (False, True, False, False)
GRID_N = 2050 * 16384                                    # more than kGridCap = 2048 chunks in one launch


@pytest.fixture(scope="module")
def lib(dev):
    from makani_amd import _lib
    return _lib.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ok(rc, what):
    from makani_amd import _lib
    _lib.check(rc, what)
    torch.cuda.synchronize()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _record(entry, **ratios):
    print("RATIO", entry, " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(got, want, what):
    assert np.array_equal(_bits(got), _bits(want)), f"{what}: not bit for bit what it was"


def state(lengths, seed=0):
    """(p, g, m, v) per tensor: N(0, 1)-like, m and v non-zero, the scale of every stream different from tensor to tensor."""
    rng = np.random.default_rng(seed)
    out = []
    for t, n in enumerate(lengths):
        p = rng.standard_normal(n) * 0.5 * (1 + t % 5)
        g = rng.standard_normal(n) * (0.3 + 0.2 * (t % 3))
        m = rng.standard_normal(n) * (0.2 + 0.1 * (t % 4))
        v = (rng.standard_normal(n) * 0.3) ** 2 + 1e-4
        out.append(tuple(a.astype(F) for a in (p, g, m, v)))
    return out


def steps_for(T):
    return [1 + (3 * t) % 7 for t in range(T)]


def split_lengths(T, seed=5):
    """1 ... 40 reals per tensor, but a 3-chunk tensor early in the first launch and one as the last tensor (index 88 / 180 / 240,
    the first one past an argument block), so ``pbase`` and ``t0`` of the second launch are not trivial."""
    n = [int(x) for x in np.random.default_rng(seed).integers(1, 41, T)]
    n[5] = n[T - 1] = BIG
    return n


def split_offsets(T):
    return [(0, 1, 2, 3) if t % 5 == 0 else (t % 4,) * 4 for t in range(T)]


def dev_scalar(dev, x):
    return poisoned(torch.tensor([x], dtype=torch.float32), dev)


# ---------------------------------------------------------------------------------------------------------------------
# AdamW / Adam
# ---------------------------------------------------------------------------------------------------------------------
def run_adam(lib, dev, data, offsets, steps, adamw, coef, table=None, coef_dev=None):
    L = oc.build_list(dev, data, offsets, PGMV_READONLY)
    cf = coef_dev if coef_dev is not None else (dev_scalar(dev, coef) if coef is not None else None)
    _ok(lib.mk_mt_adam(L.T, L.ptrs, L.n, oc.i32(steps), _ptr(table), H["lr"], None, H["beta1"], H["beta2"], H["eps"], H["wd"],
                       adamw, _ptr(cf), _st()), "mk_mt_adam")
    L.check("mk_mt_adam")
    if cf is not None and coef is not None:
        assert float(cf[0]) == coef
    return L


def check_adam(L, data, steps, adamw, coef, what):
    worst = dict(p=0.0, m=0.0, v=0.0)
    for t in range(L.T):
        ref = oc.adam_ref(*data[t], adamw=adamw, coef=1.0 if coef is None else coef, step=steps[t], **H)
        for key, d in (("p", 0), ("m", 2), ("v", 3)):
            worst[key] = max(worst[key], oc.worst_ratio(L.host(t, d), ref[key], ref["e_" + key],
                                                        f"{what}: tensor {t} (n = {L.n[t]}, step {steps[t]}): {key}"))
    return worst


@pytest.mark.parametrize("coef", [None, COEF])
@pytest.mark.parametrize("adamw", [1, 0])
@pytest.mark.parametrize("offs", list(OFFSETS))
def test_adam_edges_of_walk(dev, lib, offs, adamw, coef):
    data, steps = state(EDGE, seed=1), steps_for(len(EDGE))
    L = run_adam(lib, dev, data, OFFSETS[offs], steps, adamw, coef)
    _record("mk_mt_adam", **check_adam(L, data, steps, adamw, coef, f"{offs} adamw={adamw} coef={coef}"))


def test_adam_l2_cancellation(dev, lib):
    """``g ~ -wd p / coef``: the moments see the rounding residue of two terms a million times larger."""
    rng = np.random.default_rng(2)
    data = state((16385, 7), seed=2)
    data = [(p, (-np.float64(H["wd"]) * p / np.float64(COEF) * (1 + rng.standard_normal(p.size) * 1e-6)).astype(F), m,
             (v * F(1e-6)).astype(F)) for p, g, m, v in data]
    L = run_adam(lib, dev, data, (1, 1, 1, 1), [3, 1], 0, COEF)
    _record("mk_mt_adam(l2-cancel)", **check_adam(L, data, [3, 1], 0, COEF, "cancellation"))


@pytest.mark.parametrize("T", [89, 181, 241])
def test_adam_list_splits(dev, lib, T):
    data, steps = state(split_lengths(T), seed=T), steps_for(T)
    L = run_adam(lib, dev, data, split_offsets(T), steps, 1, COEF)
    _record(f"mk_mt_adam(T={T})", **check_adam(L, data, steps, 1, COEF, f"T={T}"))


def test_adam_grid_stride(dev, lib):
    """2050 chunks in one tensor, one float past a 16-byte boundary: the chunk loop of every workgroup takes a second trip.
    Reference and bound in float64 torch on the device."""
    g = torch.Generator(device=dev).manual_seed(7)
    p, gr, m = (torch.randn(GRID_N, device=dev, generator=g) for _ in range(3))
    v = torch.randn(GRID_N, device=dev, generator=g).square_().add_(1e-4)
    L = run_adam(lib, dev, [(p, gr, m, v)], (1, 1, 1, 1), [3], 1, COEF)
    ref = oc.adam_ref(p, gr, m, v, adamw=1, coef=COEF, step=3, **H)
    _record("mk_mt_adam(grid)", **{key: oc.worst_ratio(L.view(0, d), ref[key], ref["e_" + key], f"grid stride: {key}")
                                   for key, d in (("p", 0), ("m", 2), ("v", 3))})


def test_adam_repeatable(dev, lib):
    data, steps = state(EDGE, seed=3), steps_for(len(EDGE))
    a = run_adam(lib, dev, data, OFFSETS["mixed"], steps, 0, COEF)
    b = run_adam(lib, dev, data, OFFSETS["mixed"], steps, 0, COEF)
    for t in range(a.T):
        for d in (0, 2, 3):
            assert torch.equal(a.view(t, d), b.view(t, d))


# ---------------------------------------------------------------------------------------------------------------------
# mk_adam_step (16-byte contract)
# ---------------------------------------------------------------------------------------------------------------------
def run_adam_step(lib, dev, data, step, offsets=(0, 0, 0, 0)):
    L = oc.build_list(dev, [data], offsets, PGMV_READONLY)
    rc = lib.mk_adam_step(L.ptrs[0], L.ptrs[1], L.ptrs[2], L.ptrs[3], L.n[0], H["lr"], H["beta1"], H["beta2"], H["eps"], H["wd"],
                          step, _st())
    torch.cuda.synchronize()
    L.check("mk_adam_step")
    return L, rc


def test_adam_step_edges(dev, lib):
    worst = dict(p=0.0, m=0.0, v=0.0)
    for (n, data), step in zip(zip(EDGE, state(EDGE, seed=4)), steps_for(len(EDGE))):
        L, rc = run_adam_step(lib, dev, data, step)
        assert rc == 0
        ref = oc.adam_ref(*data, adamw=0, coef=1.0, step=step, **H)
        for key, d in (("p", 0), ("m", 2), ("v", 3)):
            worst[key] = max(worst[key], oc.worst_ratio(L.host(0, d), ref[key], ref["e_" + key], f"n = {n}: {key}"))
    _record("mk_adam_step", **worst)


@pytest.mark.parametrize("stream", [0, 1, 2, 3])
def test_adam_step_refuses_a_misaligned_pointer(dev, lib, stream):
    data = state((37,), seed=5)[0]
    offsets = tuple(1 if d == stream else 0 for d in range(4))
    L, rc = run_adam_step(lib, dev, data, 1, offsets)
    assert rc != 0 and b"buffers must be 16-byte aligned" in lib.mk_last_error()
    for d in range(4):
        _same_bits(L.host(0, d), data[d], f"stream {d} after a refused call")


def test_adam_step_grid_stride(dev, lib):
    """More than 4096 workgroups of 256 float4 lanes, and n % 4 = 3 (the scalar tail behind a grid-stride body)."""
    n = 2 * 4096 * 1024 + 3
    g = torch.Generator(device=dev).manual_seed(8)
    p, gr, m = (torch.randn(n, device=dev, generator=g) for _ in range(3))
    v = torch.randn(n, device=dev, generator=g).square_().add_(1e-4)
    L, rc = run_adam_step(lib, dev, (p, gr, m, v), 2)
    assert rc == 0
    ref = oc.adam_ref(p, gr, m, v, adamw=0, coef=1.0, step=2, **H)
    _record("mk_adam_step(grid)", **{key: oc.worst_ratio(L.view(0, d), ref[key], ref["e_" + key], f"grid stride: {key}")
                                     for key, d in (("p", 0), ("m", 2), ("v", 3))})


# ---------------------------------------------------------------------------------------------------------------------
# LAMB
# ---------------------------------------------------------------------------------------------------------------------
def run_lamb(lib, dev, data, offsets, steps, *, adamw, bc, trust, div, wd=H["wd"], what="lamb"):
    """Both stages on one list, each checked; returns the worst ratios."""
    L = oc.build_list(dev, data, offsets, PGMV_READONLY)
    T, nch = L.T, sum(oc.chunks(n) for n in L.n)
    ws = [guarded(shape, torch.float64, dev) for shape in ((nch,), (nch,), (T,), (T,))]
    dv = dev_scalar(dev, div) if div is not None else None
    args = (T, L.ptrs, L.n, oc.i32(steps), None, H["lr"], None, H["beta1"], H["beta2"], BETA3, LAMB_EPS, wd, adamw, bc, trust,
            _ptr(dv))
    wsp = [w.data_ptr() for w, _ in ws]

    def bands(stage):
        L.check(f"{what}: stage {stage}")
        for (_, chk), name in zip(ws, ("part_p", "part_u", "tsum_p", "tsum_u")):
            chk(f"{what}: stage {stage}: {name}")

    _ok(lib.mk_mt_lamb(1, *args, *wsp, _st()), "mk_mt_lamb stage 1")
    bands(1)
    worst = dict(p=0.0, m=0.0, v=0.0, tsum_p=0.0, tsum_u=0.0)
    tp, tu = ws[2][0].cpu().numpy(), ws[3][0].cpu().numpy()
    moments = []
    for t in range(T):
        k = oc.lamb_scalars(beta1=H["beta1"], beta2=H["beta2"], beta3=BETA3, eps=LAMB_EPS, wd=wd, adamw=adamw,
                            bias_correction=bc, div=1.0 if div is None else div, step=steps[t])
        r = oc.lamb1_ref(*data[t], k)
        tag = f"{what}: stage 1: tensor {t} (n = {L.n[t]}, step {steps[t]})"
        _same_bits(L.host(t, 0), data[t][0], tag + ": p")
        m1, v1 = L.host(t, 2), L.host(t, 3)
        worst["m"] = max(worst["m"], oc.worst_ratio(m1, r["m"], r["e_m"], tag + ": m"))
        worst["v"] = max(worst["v"], oc.worst_ratio(v1, r["v"], r["e_v"], tag + ": v"))
        worst["tsum_p"] = max(worst["tsum_p"], oc.scalar_ratio(tp[t], r["sp"], r["e_sp"], tag + ": tsum_p"))
        worst["tsum_u"] = max(worst["tsum_u"], oc.scalar_ratio(tu[t], r["su"], r["e_su"], tag + ": tsum_u"))
        moments.append((k, m1, v1))
    _ok(lib.mk_mt_lamb(2, *args, *wsp, _st()), "mk_mt_lamb stage 2")
    bands(2)
    assert np.array_equal(ws[2][0].cpu().numpy(), tp) and np.array_equal(ws[3][0].cpu().numpy(), tu)
    ratios = []
    for t, (k, m1, v1) in enumerate(moments):
        tag = f"{what}: stage 2: tensor {t} (n = {L.n[t]}, step {steps[t]})"
        _same_bits(L.host(t, 2), m1, tag + ": m")
        _same_bits(L.host(t, 3), v1, tag + ": v")
        r = oc.lamb2_ref(data[t][0], m1, v1, k, lr=H["lr"], trust=trust)
        worst["p"] = max(worst["p"], oc.worst_ratio(L.host(t, 0), r["p"], r["e_p"], tag + ": p"))
        ratios.append(r["ratio"])
    return worst, ratios, L


@pytest.mark.parametrize("adamw", [1, 0])
@pytest.mark.parametrize("offs", list(OFFSETS))
def test_lamb_edges_of_walk(dev, lib, offs, adamw):
    """``g-only``: stage 1 walks scalar, stage 2 (``walk<3>``, which never looks at g) takes the vector path on the same tensors."""
    data, steps = state(EDGE, seed=11), steps_for(len(EDGE))
    worst, ratios, _ = run_lamb(lib, dev, data, OFFSETS[offs], steps, adamw=adamw, bc=1, trust=1, div=COEF, what=offs)
    assert len(set(ratios)) == len(ratios), "the trust ratios of the list must differ for the test to see a mix-up"
    _record("mk_mt_lamb", **worst)


@pytest.mark.parametrize("T", [89, 181, 241])
def test_lamb_list_splits(dev, lib, T):
    data, steps = state(split_lengths(T), seed=100 + T), steps_for(T)
    worst, _, _ = run_lamb(lib, dev, data, split_offsets(T), steps, adamw=1, bc=1, trust=1, div=COEF, what=f"T={T}")
    _record(f"mk_mt_lamb(T={T})", **worst)


def _lamb_variant_state():
    """0, 1: ordinary; 2: an all-zero parameter (the ratio falls back to lr); 3: zero gradient and first moment (the update is
    ``wd p`` alone, exactly zero without weight decay); 4: all of p, g, m zero (both norms zero, p stays zero)."""
    data = [list(x) for x in state((7, 16385, 40, 5, 33), seed=12)]
    data[2][0] = np.zeros_like(data[2][0])
    data[3][1], data[3][2] = np.zeros_like(data[3][1]), np.zeros_like(data[3][2])
    for d in (0, 1, 2):
        data[4][d] = np.zeros_like(data[4][d])
    return [tuple(x) for x in data]


@pytest.mark.parametrize("div", [None, COEF])
@pytest.mark.parametrize("adamw", [1, 0])
@pytest.mark.parametrize("bc", [1, 0])
@pytest.mark.parametrize("trust", [1, 0])
def test_lamb_variants(dev, lib, trust, bc, adamw, div):
    data = _lamb_variant_state()
    worst, ratios, L = run_lamb(lib, dev, data, OFFSETS["off1"], [1, 4, 2, 3, 5], adamw=adamw, bc=bc, trust=trust, div=div,
                                what=f"trust={trust} bc={bc} adamw={adamw} div={div}")
    assert ratios[2] == H["lr"] and ratios[4] == H["lr"] and (ratios[0] != H["lr"]) == bool(trust)
    assert not L.host(4, 0).any()
    _record("mk_mt_lamb(variants)", **worst)


@pytest.mark.parametrize("adamw", [1, 0])
def test_lamb_exactly_zero_update(dev, lib, adamw):
    """Without weight decay a tensor with zero gradient and first moment has u = 0: |u| = 0, the ratio is lr, p is untouched."""
    data = _lamb_variant_state()
    worst, ratios, L = run_lamb(lib, dev, data, OFFSETS["off3"], [1, 4, 2, 3, 5], adamw=adamw, bc=1, trust=1, div=COEF, wd=0.0,
                                what=f"wd=0 adamw={adamw}")
    assert ratios[3] == H["lr"]
    _same_bits(L.host(3, 0), data[3][0], "p of the tensor whose update is zero")


def test_lamb_repeatable(dev, lib):
    data, steps = state(EDGE, seed=13), steps_for(len(EDGE))
    runs = [run_lamb(lib, dev, data, OFFSETS["rotated"], steps, adamw=1, bc=1, trust=1, div=COEF)[2] for _ in range(2)]
    for t in range(len(EDGE)):
        for d in (0, 2, 3):
            assert torch.equal(runs[0].view(t, d), runs[1].view(t, d))


# ---------------------------------------------------------------------------------------------------------------------
# norms, coefficients, the in-place scale
# ---------------------------------------------------------------------------------------------------------------------
def run_sumsq(lib, dev, xs, offsets, clip_mode, max_norm, table=None, inc=(), what="mk_mt_sumsq"):
    """One call; returns (tsum numpy, G or None, coef or None, the list) after checking every band."""
    L = oc.build_list(dev, [(x,) for x in xs], offsets, (True,))
    nch = sum(oc.chunks(n) for n in L.n)
    (part, pc), (tsum, tc) = guarded((nch,), torch.float64, dev), guarded((L.T,), torch.float64, dev)
    (norm, nc), (coef, cc) = guarded((1,), torch.float32, dev), guarded((1,), torch.float32, dev)
    _ok(lib.mk_mt_sumsq(L.T, L.ptrs, L.n, part.data_ptr(), tsum.data_ptr(), clip_mode, max_norm, norm.data_ptr(), coef.data_ptr(),
                        _ptr(table), oc.i32(inc) if len(inc) else None, len(inc), _st()), what)
    L.check(what)
    for chk, name in ((pc, "partials"), (tc, "tsum"), (nc, "norm_out"), (cc, "coef_out")):
        chk(f"{what}: {name}")
    return tsum.cpu().numpy(), norm.cpu().numpy()[0], coef.cpu().numpy()[0], L, coef


def check_norms(xs, tsum, G, coef, clip_mode, max_norm, what):
    exact = [oc.exact_sumsq(x) for x in xs]
    worst = dict(tsum=0.0, G=0.0, coef=0.0)
    for t, (s, e) in enumerate(exact):
        worst["tsum"] = max(worst["tsum"], oc.scalar_ratio(tsum[t], s, e, f"{what}: tsum[{t}] (n = {len(xs[t])})"))
    check_total([s for s, _ in exact], [e for _, e in exact], G, coef, clip_mode, max_norm, what, worst)
    return worst


def check_total(ts, es, G, coef, clip_mode, max_norm, what, worst):
    sentinel = F(SENTINEL)
    if clip_mode == 0:
        _same_bits(G, sentinel, what + ": norm_out with clip_mode 0")
        _same_bits(coef, sentinel, what + ": coef_out with clip_mode 0")
        return
    Gr, eG, c, ec = oc.clip_ref(ts, es, max_norm, clip_mode)
    worst["G"] = max(worst["G"], oc.scalar_ratio(G, Gr, eG, what + ": G"))
    if clip_mode == 3:
        _same_bits(coef, sentinel, what + ": coef_out with clip_mode 3")
    else:
        worst["coef"] = max(worst["coef"], oc.scalar_ratio(coef, c, ec, what + f": coefficient of clip_mode {clip_mode}"))
        assert (c == 1.0) == (float(coef) == 1.0)


MODES = [(0, 1.0), (1, 1.0), (1, 1e4), (2, 1.0), (2, 1e4), (3, 1.0)]        # clipping and not clipping


@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_sumsq_and_scale_edges_of_walk(dev, lib, off):
    xs = [d[1] for d in state(EDGE, seed=20 + off)]
    worst = dict(tsum=0.0, G=0.0, coef=0.0)
    for mode, max_norm in MODES:
        tsum, G, coef, _, _ = run_sumsq(lib, dev, xs, (off,), mode, max_norm)
        for k, v in check_norms(xs, tsum, G, coef, mode, max_norm, f"off {off} mode {mode} max {max_norm}").items():
            worst[k] = max(worst[k], v)
    _record("mk_mt_sumsq", **worst)
    check_scale(lib, dev, xs, (off,))


def check_scale(lib, dev, xs, offsets):
    L = oc.build_list(dev, [(x,) for x in xs], offsets, (False,))
    cf = dev_scalar(dev, COEF)
    _ok(lib.mk_mt_scale(L.T, L.ptrs, L.n, cf.data_ptr(), _st()), "mk_mt_scale")
    L.check("mk_mt_scale")
    for t, x in enumerate(xs):
        _same_bits(L.host(t, 0), x * F(COEF), f"mk_mt_scale: tensor {t} (n = {len(x)}) against the fp32 product")


@pytest.mark.parametrize("T", [89, 181, 241])
def test_norm_list_splits(dev, lib, T):
    """181: two sum-of-squares launches; 241: also two finalize launches and the unfused total."""
    xs = [d[1] for d in state(split_lengths(T), seed=200 + T)]
    offsets = [(t % 4,) for t in range(T)]
    worst = dict(tsum=0.0, G=0.0, coef=0.0)
    first = None
    for mode, max_norm in MODES:
        tsum, G, coef, _, _ = run_sumsq(lib, dev, xs, offsets, mode, max_norm)
        for k, v in check_norms(xs, tsum, G, coef, mode, max_norm, f"T={T} mode {mode} max {max_norm}").items():
            worst[k] = max(worst[k], v)
        if mode == 1 and max_norm == 1.0:
            again = run_sumsq(lib, dev, xs, offsets, mode, max_norm)
            assert np.array_equal(again[0], tsum) and _bits(again[1]) == _bits(G) and _bits(again[2]) == _bits(coef)
    _record(f"mk_mt_sumsq(T={T})", **worst)
    check_scale(lib, dev, xs, offsets)


@pytest.mark.parametrize("T", [3, 241])
def test_norm_finish_alone(dev, lib, T):
    ts = (np.random.default_rng(T).random(T) * 10.0 ** np.arange(T).clip(max=6) + 0.1).astype(np.float64)
    tsum = poisoned(torch.from_numpy(ts), dev)
    worst = dict(G=0.0, coef=0.0)
    for mode, max_norm in MODES[1:]:
        (norm, nc), (coef, cc) = guarded((1,), torch.float32, dev), guarded((1,), torch.float32, dev)
        _ok(lib.mk_mt_norm_finish(T, tsum.data_ptr(), mode, max_norm, norm.data_ptr(), coef.data_ptr(), None, None, 0, _st()),
            "mk_mt_norm_finish")
        nc("norm_out"), cc("coef_out")
        assert np.array_equal(tsum.cpu().numpy(), ts)
        check_total(list(ts), [0.0] * T, norm.cpu().numpy()[0], coef.cpu().numpy()[0], mode, max_norm, f"T={T} mode {mode}", worst)
    _record("mk_mt_norm_finish", **worst)


def test_sumsq_and_scale_grid_stride(dev, lib):
    x = torch.randn(GRID_N, device=dev, generator=torch.Generator(device=dev).manual_seed(9))
    L = oc.build_list(dev, [(x,)], (1,), (True,))
    (part, pc), (tsum, tc) = guarded((oc.chunks(GRID_N),), torch.float64, dev), guarded((1,), torch.float64, dev)
    (norm, nc), (coef, cc) = guarded((1,), torch.float32, dev), guarded((1,), torch.float32, dev)
    _ok(lib.mk_mt_sumsq(1, L.ptrs, L.n, part.data_ptr(), tsum.data_ptr(), 3, 1.0, norm.data_ptr(), coef.data_ptr(), None, None, 0,
                        _st()), "mk_mt_sumsq")
    L.check("mk_mt_sumsq grid stride")
    pc("partials"), tc("tsum"), nc("norm_out"), cc("coef_out")
    s = float(x.double().square().sum())                   # torch's float64 tree sum: its own error is far below the bound
    r = oc.scalar_ratio(float(tsum[0]), s, oc.sumsq_bound(GRID_N, s), "tsum of the grid-stride tensor")
    per_chunk = x.double().square().view(-1, oc.CHUNK).sum(1)
    oc.worst_ratio(part, per_chunk, oc.CHUNK * oc.U64 * per_chunk, "partials of the grid-stride tensor")
    Gr, eG, _, _ = oc.clip_ref([s], [oc.sumsq_bound(GRID_N, s)], 1.0, 3)
    _record("mk_mt_sumsq(grid)", tsum=r, G=oc.scalar_ratio(float(norm[0]), Gr, eG, "G"))
    S = oc.build_list(dev, [(x,)], (1,), (False,))
    cf = dev_scalar(dev, COEF)
    _ok(lib.mk_mt_scale(1, S.ptrs, S.n, cf.data_ptr(), _st()), "mk_mt_scale")
    S.check("mk_mt_scale grid stride")
    assert torch.equal(S.view(0, 0).view(torch.int32), (x * cf[0]).view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------
# the step table
# ---------------------------------------------------------------------------------------------------------------------
NSLOT = 300


def step_table(dev):
    start = (1 + (np.arange(NSLOT) * 7) % NSLOT).astype(F)                  # 300 distinct counts
    table, chk = guarded((NSLOT,), torch.float32, dev)
    table.copy_(torch.from_numpy(start))
    return table, chk, start


def check_table(table, chk, start, inc, what):
    chk(what + ": step table")
    want = start.copy()
    want[list(inc)] += 1
    assert len(set(inc)) == len(inc)
    _same_bits(table.cpu().numpy(), want, what + ": named slots exactly + 1, the others untouched")
    return want


def adam_from_table(lib, dev, table, chk, want, slots, seed, what, coef=None, coef_dev=None):
    """The update after an increment reads the incremented counts (the reference is evaluated at that step)."""
    data = state(EDGE[-len(slots):], seed=seed)
    L = run_adam(lib, dev, data, OFFSETS["mixed"], slots, 1, coef, table=table, coef_dev=coef_dev)
    chk(what + ": step table after the update")
    _same_bits(table.cpu().numpy(), want, what + ": the update must not write the table")
    steps = [int(want[s]) for s in slots]
    assert len(set(steps)) > 1
    return check_adam(L, data, steps, 1, coef, what)


def test_step_table_fused_subset(dev, lib):
    """``mk_mt_sumsq`` increments a strict subset of the slots in its fused finalize; slots are not in list order."""
    table, chk, start = step_table(dev)
    T = len(EDGE)
    slots = [(11 * t + 3) % NSLOT for t in range(T)][::-1]
    inc = slots[::2]
    xs = [d[1] for d in state(EDGE, seed=30)]
    tsum, G, coef, _, coef_dev = run_sumsq(lib, dev, xs, (2,), 1, 1.0, table=table, inc=inc)
    check_norms(xs, tsum, G, coef, 1, 1.0, "fused increment")
    want = check_table(table, chk, start, inc, "fused increment")
    _record("mk_mt_adam(table)", **adam_from_table(lib, dev, table, chk, want, slots, 31, "after the fused increment",
                                                   coef=float(coef), coef_dev=coef_dev))


@pytest.mark.parametrize("entry", ["sumsq", "norm_finish", "step_inc"])
def test_step_table_241_increments(dev, lib, entry):
    """More increments than one finalize takes: the unfused path with a small T (``mk_mt_sumsq``, ``mk_mt_norm_finish``) and
    ``mk_mt_step_inc`` in two launches."""
    table, chk, start = step_table(dev)
    inc = list(range(NSLOT - 1, NSLOT - 242, -1))
    slots = [60, 299, 150]
    assert len(inc) == 241 and all(s in inc for s in slots)
    xs = [d[1] for d in state((5, 16385, 40), seed=32)]
    if entry == "sumsq":
        tsum, G, coef, _, _ = run_sumsq(lib, dev, xs, (1,), 2, 1.0, table=table, inc=inc)
        check_norms(xs, tsum, G, coef, 2, 1.0, "unfused increment")
    elif entry == "norm_finish":
        ts = np.array([oc.exact_sumsq(x)[0] for x in xs])
        tsum = poisoned(torch.from_numpy(ts), dev)
        (norm, nc), (coef, cc) = guarded((1,), torch.float32, dev), guarded((1,), torch.float32, dev)
        _ok(lib.mk_mt_norm_finish(3, tsum.data_ptr(), 1, 1.0, norm.data_ptr(), coef.data_ptr(), table.data_ptr(), oc.i32(inc),
                                  len(inc), _st()), "mk_mt_norm_finish")
        nc("norm_out"), cc("coef_out")
        check_total(list(ts), [0.0] * 3, norm.cpu().numpy()[0], coef.cpu().numpy()[0], 1, 1.0, "norm_finish with increments",
                    dict(G=0.0, coef=0.0))
    else:
        _ok(lib.mk_mt_step_inc(table.data_ptr(), oc.i32(inc), len(inc), _st()), "mk_mt_step_inc")
    want = check_table(table, chk, start, inc, entry)
    adam_from_table(lib, dev, table, chk, want, slots, 33, f"after {entry}")
