"""``mk_input_assemble``, ``mk_input_assemble_bwd`` and ``mk_history_sums`` (csrc/preproc.hip) held to the three criteria of
tests/kernel_checks.py through the C ABI.

Assembly, each way: every output element is compared BIT FOR BIT with the formula of preproc.hip evaluated in CPU torch fp32 --
``(v - mean) / std``, then ``* mask``, then the cast; backward ``g * mask``, then ``/ std`` -- there is no fma to contract and the
division is correctly rounded on both sides.  All four dtype pairs, with and without per-sample statistics (``std`` in [0.3, 3]),
no mask and a mask list that holds the first and the last dynamic channel, a channel of the second history step and one entry
``>= T (C + Cu)`` that must match nothing, with the mask read from static channel 0, a middle one and the last of three, so a kernel
that ignored ``mask_src`` fails.  ``x``, ``u`` and the output (backward: the incoming and the outgoing gradient) each sit 0 and 1
elements past a 16-byte boundary, independently; the output is guarded, the element in front of an offset view included; every
input lies between NaN bands and must come back bit for bit.  (3, 1, 4, 0, 1, 2800, 3) has 42 000 forward and 33 600 backward
rows, more than the 32 768 a grid covers in one trip.

Sums: ``S1 = sum_t w_t sum x`` and ``S2 = sum_t w_t sum x^2`` against the exact sums (python integers, ``stats_checks.to_int``; the
weights are fp32, so every term is an integer multiple of a power of two) within ``(T H W + 64) 2^-53 sum w |x|^k``: fp64 from the
first addition on in any order (T H W - 1 additions at most), the weight's fma per history step and the fixed folds of 64 lanes,
4 waves and the slabs.  ``x`` and ``u`` at different offsets, workspace and sums guarded, two calls bitwise equal.
"""
import itertools

import numpy as np
import pytest
import torch

import optim_checks as oc
import stats_checks as sc
from kernel_checks import guarded
from stream_checks import bits, code, out_at, put, stream, unchanged

pytestmark = pytest.mark.gpu

# (B, T, C, Cu, Cs, H, W)
SHAPES = [(1, 1, 1, 0, 1, 1, 1), (2, 2, 3, 1, 3, 5, 7), (2, 1, 4, 1, 3, 3, 61), (1, 2, 2, 0, 3, 2, 1441), (3, 1, 4, 0, 1, 2800, 3)]
DTYPES = [torch.float32, torch.bfloat16]
PAIRS = list(itertools.product(DTYPES, DTYPES))
_NAME = {torch.float32: "fp32", torch.bfloat16: "bf16"}
_CACHE = {}


def _sid(s):
    return "x".join(map(str, s))


def problem(shape, dtype):
    """Host inputs of one shape, ``x`` and the upstream gradient in ``dtype``: normal-range values, computed once."""
    key = (shape, dtype)
    if key not in _CACHE:
        B, T, C, Cu, Cs, H, W = shape
        Cn = C + Cu
        g = torch.Generator().manual_seed(500 + 7 * H * W + C)
        r = lambda *s: torch.randn(*s, generator=g)
        x = (2.0 * r(B, T, C, H, W) + 0.5).to(dtype)
        u = r(B, T, Cu, H, W) if Cu else None
        stat = r(Cs, H, W) + 0.25
        mean = r(B, Cn)
        std = 0.3 + 2.7 * torch.rand(B, Cn, generator=g)
        gout = r(B, T * Cn + Cs, H, W).to(dtype)
        _CACHE[key] = (x, u, stat, mean, std, gout)
    return _CACHE[key]


def mask_list(shape):
    """The masked output channels: first and last dynamic channel, one of the second history step, and one entry that is no
    dynamic channel (the first static one), which must match nothing."""
    B, T, C, Cu, Cs, H, W = shape
    Cn, Cd = C + Cu, T * (C + Cu)
    chans = [0, Cd - 1, Cd]
    if T > 1:
        chans.insert(1, Cn + min(1, Cn - 1))
    return list(dict.fromkeys(chans))


def mask_cases(shape):
    """(mask list or None, mask_src): no mask, then every source the issue names."""
    Cs = shape[4]
    return [(None, 0)] + [(mask_list(shape), s) for s in sorted({0, Cs // 2, Cs - 1})]


def forward_ref(shape, x, u, stat, mean, std, chans, src, out_dtype):
    B, T, C, Cu, Cs, H, W = shape
    Cn, Cd = C + Cu, T * (C + Cu)
    v = x.float()
    if Cu:
        v = torch.cat([v, u], dim=2)                                    # [B, T, Cn, H, W]
    if mean is not None:
        v = (v - mean.view(B, 1, Cn, 1, 1)) / std.view(B, 1, Cn, 1, 1)
    v = v.reshape(B, Cd, H, W).clone()
    for oc_ in (chans or []):
        if oc_ < Cd:
            v[:, oc_] = v[:, oc_] * stat[src]
    return torch.cat([v, stat.unsqueeze(0).expand(B, Cs, H, W)], dim=1).to(out_dtype)


def backward_ref(shape, gout, stat, std, chans, src, x_dtype):
    B, T, C, Cu, Cs, H, W = shape
    Cn, Cd = C + Cu, T * (C + Cu)
    g = gout.float()[:, :Cd].clone(memory_format=torch.contiguous_format)
    for oc_ in (chans or []):
        if oc_ < Cd:
            g[:, oc_] = g[:, oc_] * stat[src]
    g = g.view(B, T, Cn, H, W)[:, :, :C]
    if std is not None:
        g = g / std[:, :C].reshape(B, 1, C, 1, 1)
    return g.contiguous().to(x_dtype)


def _mask_dev(chans, dev):
    if chans is None:
        return None, None, 0
    host = torch.tensor(chans, dtype=torch.int32)
    return host.to(dev), host, len(chans)


def _bit_equal(got, want, what):
    bad = bits(got) != bits(want)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the CPU fp32 formula, the first at " \
                                f"{tuple(int(i) for i in torch.nonzero(bad.view(want.shape))[0])}"


@pytest.mark.parametrize("with_stats", [True, False], ids=["stats", "nostats"])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{_NAME[p[0]]}-{_NAME[p[1]]}")
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_assemble_every_element(dev, shape, pair, with_stats):
    from makani_amd import _lib
    lib = _lib.load()
    B, T, C, Cu, Cs, H, W = shape
    xdt, odt = pair
    x, u, stat, mean, std, _ = problem(shape, xdt)
    if not with_stats:
        mean = std = None
    sd, swhole, sflat = put(stat, 0, dev)
    held = [(swhole, sflat)]
    mptr = vptr = None
    if with_stats:
        md, mwhole, mflat = put(mean, 0, dev)
        vd, vwhole, vflat = put(std, 0, dev)
        held += [(mwhole, mflat), (vwhole, vflat)]
        mptr, vptr = md.data_ptr(), vd.data_ptr()
    for chans, src in mask_cases(shape):
        want = forward_ref(shape, x, u, stat, mean, std, chans, src, odt)
        cd, chost, n_mask = _mask_dev(chans, dev)
        for xo, uo, oo in itertools.product((0, 1), repeat=3):
            if uo and not Cu:
                continue
            what = f"mask {chans} from {src}, offsets x {xo} u {uo} out {oo}"
            xd, xwhole, xflat = put(x, xo, dev)
            uptr, uheld = None, []
            if Cu:
                ud, uwhole, uflat = put(u, uo, dev)
                uptr, uheld = ud.data_ptr(), [(uwhole, uflat)]
            out, ochk = out_at(want.shape, odt, oo, dev)
            _lib.check(lib.mk_input_assemble(xd.data_ptr(), code(xdt), uptr, sd.data_ptr(), mptr, vptr,
                                             None if cd is None else cd.data_ptr(), n_mask, src, out.data_ptr(), code(odt),
                                             B, T, C, Cu, Cs, H, W, stream()), "mk_input_assemble")
            torch.cuda.synchronize()
            ochk(what)
            for whole, flat in held + [(xwhole, xflat)] + uheld:
                unchanged(whole, flat, what)
            if cd is not None:
                assert torch.equal(cd.cpu(), chost), f"{what}: the mask list was written"
            _bit_equal(out.cpu(), want, what)
    print("RATIO mk_input_assemble", _sid(shape), f"{_NAME[xdt]}->{_NAME[odt]} stats={with_stats} differing elements=0 worst={0.0:.3f}")


@pytest.mark.parametrize("with_stats", [True, False], ids=["stats", "nostats"])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{_NAME[p[0]]}-{_NAME[p[1]]}")
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_assemble_backward_every_element(dev, shape, pair, with_stats):
    from makani_amd import _lib
    lib = _lib.load()
    B, T, C, Cu, Cs, H, W = shape
    gdt, xdt = pair
    _, _, stat, _, std, gout = problem(shape, gdt)
    if not with_stats:
        std = None
    sd, swhole, sflat = put(stat, 0, dev)
    held = [(swhole, sflat)]
    vptr = None
    if with_stats:
        vd, vwhole, vflat = put(std, 0, dev)
        held.append((vwhole, vflat))
        vptr = vd.data_ptr()
    for chans, src in mask_cases(shape):
        want = backward_ref(shape, gout, stat, std, chans, src, xdt)
        cd, chost, n_mask = _mask_dev(chans, dev)
        for go, xo in itertools.product((0, 1), repeat=2):
            what = f"mask {chans} from {src}, offsets gout {go} gx {xo}"
            gd, gwhole, gflat = put(gout, go, dev)
            gx, xchk = out_at(want.shape, xdt, xo, dev)
            _lib.check(lib.mk_input_assemble_bwd(gd.data_ptr(), code(gdt), sd.data_ptr(), vptr,
                                                 None if cd is None else cd.data_ptr(), n_mask, src, gx.data_ptr(), code(xdt),
                                                 B, T, C, Cu, Cs, H, W, stream()), "mk_input_assemble_bwd")
            torch.cuda.synchronize()
            xchk(what)
            for whole, flat in held + [(gwhole, gflat)]:
                unchanged(whole, flat, what)
            if cd is not None:
                assert torch.equal(cd.cpu(), chost), f"{what}: the mask list was written"
            _bit_equal(gx.cpu(), want, what)
    print("RATIO mk_input_assemble_bwd", _sid(shape), f"{_NAME[gdt]}->{_NAME[xdt]} stats={with_stats} differing elements=0 worst={0.0:.3f}")


# ---------------------------------------------------------------------------------------------------------------------
# mk_history_sums
# ---------------------------------------------------------------------------------------------------------------------
def exact_history_sums(x, u, wt):
    """(truth, mag), each [B, Cn, 2] float64: ``sum_t w_t sum_hw v^k`` exactly, rounded once, and ``sum w |v|^k``."""
    v = x if u is None else np.concatenate([x, u], axis=2)              # [B, T, Cn, H, W] fp32 values
    B, T, Cn = v.shape[:3]
    vi, wi = sc.to_int(v), sc.to_int(wt)
    truth, mag = np.empty((B, Cn, 2)), np.empty((B, Cn, 2))
    for b in range(B):
        for j in range(Cn):
            s1 = s2 = a1 = a2 = 0
            for t in range(T):
                f = vi[b, t, j].ravel()
                sq = int((f * f).sum())
                s1 += int(wi[t]) * int(f.sum())
                a1 += abs(int(wi[t])) * int(np.abs(f).sum())
                s2 += int(wi[t]) * sq
                a2 += abs(int(wi[t])) * sq
            truth[b, j] = s1 / (1 << 298), s2 / (1 << 447)
            mag[b, j] = a1 / (1 << 298), a2 / (1 << 447)
    return truth, mag


def history_problem(dtype, Cu, T, H, W):
    key = ("hist", dtype, Cu, T, H, W)
    if key not in _CACHE:
        B, C = 2, 2
        g = torch.Generator().manual_seed(900 + 5 * H * W + T + Cu)
        x = (1.5 * torch.randn(B, T, C, H, W, generator=g) + 0.75).to(dtype)
        u = torch.randn(B, T, Cu, H, W, generator=g) - 0.5 if Cu else None
        wt = torch.rand(T, generator=g) + 0.25
        wt = wt / wt.sum()
        truth = exact_history_sums(x.float().numpy(), None if u is None else u.numpy(), wt.numpy())
        _CACHE[key] = (x, u, wt, truth)
    return _CACHE[key]


@pytest.mark.parametrize("W", [1, 9, 61, 1441])
@pytest.mark.parametrize("H", [1, 17])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("Cu", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_history_sums_against_the_exact_sums(dev, dtype, Cu, T, H, W):
    from makani_amd import _lib
    lib = _lib.load()
    x, u, wt, (want, mag) = history_problem(dtype, Cu, T, H, W)
    B, C = x.shape[0], x.shape[2]
    bound = (T * H * W + 64) * 2.0 ** -53 * mag
    td, twhole, tflat = put(wt, 0, dev)
    worst = 0.0
    for xo, uo in ((0, 1), (1, 0), (3, 2)):
        what = f"offsets x {xo} u {uo}"
        xd, xwhole, xflat = put(x, xo, dev)
        held = [(xwhole, xflat), (twhole, tflat)]
        uptr = None
        if Cu:
            ud, uwhole, uflat = put(u, uo, dev)
            held.append((uwhole, uflat))
            uptr = ud.data_ptr()
        ws, wchk = guarded((lib.mk_history_workspace(B, C + Cu, H),), torch.float64, dev)
        sums, schk = guarded((B, C + Cu, 2), torch.float64, dev)
        runs = []
        for _ in range(2):
            _lib.check(lib.mk_history_sums(xd.data_ptr(), code(dtype), uptr, td.data_ptr(), ws.data_ptr(), sums.data_ptr(),
                                           B, T, C, Cu, H, W, stream()), "mk_history_sums")
            torch.cuda.synchronize()
            wchk(what + ": workspace")
            schk(what + ": sums")
            runs.append(sums.cpu().numpy())
        assert np.array_equal(runs[0], runs[1]), f"{what}: the sums of two calls differ"
        for whole, flat in held:
            unchanged(whole, flat, what)
        worst = max(worst, oc.worst_ratio(runs[1], want, bound, what))
    print("RATIO mk_history_sums", f"B{B} T{T} C{C} Cu{Cu} H{H} W{W}", dtype, f"worst={worst:.3f}")
