"""Reference, magnitudes and bounds for the trailing-axis layer norm kernels (csrc/toknorm.hip); a plain module like
attn_checks.py.

Reference: float64 on the operands as they are (``reference``): ``s = x + r``, ``mean``, biased ``var``, ``rstd``,
``xh = (s - mean) rstd``, ``y = w xh + b`` and, with ``g = gy + gy2``, ``gx = rstd (w g - mean_row(w g) - xh mean_row(w g xh)) + gs``,
``gw = sum_rows g xh``, ``gb = sum_rows g``.

Bounds, every element, with ``u = 2^-24`` and ``e = |xh| + rstd (|s| + mean_row|s|)`` -- what ``xh`` is off by, in units of u,
when ``s``, the mean and the difference are each rounded once (the second term is the cancellation in ``s - mean``):

    |y  - ref| <= [ulp_bf16 if bf16] + C_Y  u (|w| e + |b|)
    |gx - ref| <= [ulp_bf16 if bf16] + C_GX u mag_gx,
                  mag_gx = rstd (|w g| + S1 + |xh| S2 + e S2 + |xh| mean_row(|w g| e)) + |gs|,  S1 = mean_row|w g|,  S2 = mean_row|w g xh|
    |gw - ref| <= C_GW u sum_rows |g| e,        |gb - ref| <= C_GB u sum_rows |g|
    |mean - ref| <= C_STAT u mean_row|s|,       |rstd - ref| <= C_STAT u rstd (1 + rstd mean_row(|xh| (|s| + mean_row|s|)))

(the last line: the variance is off by the roundings of ``(s - mean)^2``, ``2 |s - mean| u (|s| + |mean|)`` each, and rstd by half
of that relative to ``var + eps``).  The bf16 ulp is the one of ``kernel_checks.bf16_elementwise``.

The constants are NOT taken from the kernels.  ``emulate`` is a CPU emulation of the kernels' arithmetic in fp32 torch ops: the
sum in fp32, the reduction tree (a thread adds the 8 elements of a vector and its vectors in order, the 64 lanes fold by an
xor butterfly, the 8 waves of a workgroup in order; rows of up to 2048 elements belong to one wavefront, longer ones to 512
threads), the two-pass variance, fused multiply-adds where the kernels spell ``fmaf`` (formed in float64 and rounded: the
product of two fp32 numbers is exact there), the fp32 partial column sums per wavefront / workgroup and the float64 finish.
Over ``EMU_SHAPES`` x ``EMU_DISTS`` x ``EMU_SEEDS`` seeds (fp32 ``x`` from the distribution, a bf16 N(0, 1) residual, fp32 and
bf16 results) its worst ratios to the units above are the ``EMU_WORST_*`` figures; each constant is twice that figure,
rounded up, the factor 2 for the reduction order and the hardware's reciprocal square root.  tests/test_toknorm_cpu.py asserts
that the emulation stays within HALF of each constant.
"""
import math

import torch

import kernel_checks as kc

U = 2.0 ** -24
WAVE_MAX = 2048                  # rows up to here belong to one wavefront (64 threads), longer ones to 512 threads
BWD_WAVE_GRID, BWD_BLOCK_GRID = 1024, 256

EMU_SHAPES = [(5000, 7), (300, 48), (130, 384), (40, 1030), (300, 2056), (6, 16200)]      # (rows, L)
EMU_DISTS = {"n53": (5.0, 3.0), "n01": (0.0, 1.0), "n50": (50.0, 0.1)}                    # x ~ N(mean, std^2)
EMU_SEEDS = 2
# worst ratios of the emulation over EMU_SHAPES x EMU_DISTS x EMU_SEEDS (measured on the CPU, see the module docstring)
EMU_WORST_Y = 2.65
EMU_WORST_GX = 2.86
EMU_WORST_GW = 1.37
EMU_WORST_GB = 1.60
EMU_WORST_STAT = 3.54
C_Y = 6.0
C_GX = 6.0
C_GW = 3.0
C_GB = 4.0
C_STAT = 8.0


def make_inputs(rows, L, dist="n01", seed=0, x_dtype=torch.float32, r_dtype=torch.bfloat16):
    """x from the distribution, r, gy, gs N(0, 1), gy2 bf16 N(0, 1), w N(1, 0.5^2), b N(0, 0.5^2): a dict of CPU tensors."""
    g = torch.Generator().manual_seed(seed * 1000003 + rows * 131 + L)
    m, sd = EMU_DISTS[dist]
    n = lambda *shape: torch.randn(*shape, generator=g)
    return dict(x=(m + sd * n(rows, L)).to(x_dtype), r=n(rows, L).to(r_dtype), w=1.0 + 0.5 * n(L), b=0.5 * n(L), gy=n(rows, L),
                gy2=n(rows, L).bfloat16(), gs=n(rows, L))


def _d(t, like):
    return torch.zeros_like(like) if t is None else t.double().cpu()


def reference(x, r=None, w=None, b=None, eps=1e-5, gy=None, gy2=None, gs=None):
    """float64 values and the units of the bounds; the gradients when any of gy, gy2, gs is given."""
    x = x.double().cpu()
    rows, L = x.shape
    s = x + _d(r, x)
    w = torch.ones(L, dtype=torch.float64) if w is None else w.double().cpu()
    b = torch.zeros(L, dtype=torch.float64) if b is None else b.double().cpu()
    mean = s.mean(1, keepdim=True)
    var = (s - mean).square().mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (s - mean) * rstd
    sabs = s.abs().mean(1, keepdim=True)
    e = xh.abs() + rstd * (s.abs() + sabs)
    ref = dict(s=s, y=w * xh + b, unit_y=w.abs() * e + b.abs(), mean=mean[:, 0], rstd=rstd[:, 0], unit_mean=sabs[:, 0],
               unit_rstd=(rstd * (1.0 + rstd * (xh.abs() * (s.abs() + sabs)).mean(1, keepdim=True)))[:, 0])
    if gy is not None or gy2 is not None or gs is not None:
        g = _d(gy, x) + _d(gy2, x)
        gs = _d(gs, x)
        wg = w * g
        S1, S2 = wg.abs().mean(1, keepdim=True), (wg * xh).abs().mean(1, keepdim=True)
        ref.update(gx=rstd * (wg - wg.mean(1, keepdim=True) - xh * (wg * xh).mean(1, keepdim=True)) + gs,
                   unit_gx=rstd * (wg.abs() + S1 + xh.abs() * S2 + e * S2 + xh.abs() * (wg.abs() * e).mean(1, keepdim=True)) + gs.abs(),
                   gw=(g * xh).sum(0), unit_gw=(g.abs() * e).sum(0), gb=g.sum(0), unit_gb=g.abs().sum(0))
    return ref


def excess_ratio(got, ref64, unit64):
    """``(|got - ref| - [ulp_bf16 if got is bf16]) / (u unit)`` per element; an element without a unit must be exact."""
    g = got.detach().double().cpu()
    assert tuple(g.shape) == tuple(ref64.shape) == tuple(unit64.shape), (tuple(g.shape), tuple(ref64.shape), tuple(unit64.shape))
    err = (g - ref64).abs()
    if got.dtype == torch.bfloat16:
        rms = ref64.square().mean().sqrt()
        err = (err - kc.bf16_ulp(torch.maximum(torch.maximum(g.abs(), ref64.abs()), rms / 256))).clamp_min(0.0)
    unit = U * unit64
    return torch.where(unit > 0, err / unit.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).to(err.dtype))


def check(got, ref64, unit64, c, what=""):
    """Asserts that every element is finite and within ``c`` units (plus one bf16 ulp for a bf16 result); returns the worst ratio."""
    bad = ~torch.isfinite(got.detach().float())
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements are NaN or Inf"
    ratio = excess_ratio(got, ref64, unit64)
    flat = int(torch.argmax(ratio))
    worst = float(ratio.flatten()[flat])
    if not worst <= c:
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ratio.shape))
        raise AssertionError(f"{what}: worst |got - ref| / (u unit) = {worst:.2f} (limit {c}) at {idx}: got = {float(got[idx])!r}, "
                             f"ref = {float(ref64[idx])!r}, unit = {float(unit64[idx]):.3e}; {int((ratio > c).sum())} of {ratio.numel()} "
                             f"elements exceed the limit")
    return worst


def check_forward(ref, y=None, y2=None, stats=None, what=""):
    """The worst ratios of whatever is given: a dict."""
    out = {}
    if y is not None:
        out["y"] = check(y, ref["y"], ref["unit_y"], C_Y, f"{what} y")
    if y2 is not None:
        assert y2.dtype == torch.bfloat16
        out["y2"] = check(y2, ref["y"], ref["unit_y"], C_Y, f"{what} y2")
    if stats is not None:
        out["mean"] = check(stats[:, 0], ref["mean"], ref["unit_mean"], C_STAT, f"{what} mean")
        out["rstd"] = check(stats[:, 1], ref["rstd"], ref["unit_rstd"], C_STAT, f"{what} rstd")
    return out


def check_backward(ref, gx=None, gr=None, gw=None, gb=None, what=""):
    out = {}
    if gx is not None:
        out["gx"] = check(gx, ref["gx"], ref["unit_gx"], C_GX, f"{what} gx")
    if gr is not None:
        out["gr"] = check(gr, ref["gx"], ref["unit_gx"], C_GX, f"{what} gr")
    if gw is not None:
        out["gw"] = check(gw, ref["gw"], ref["unit_gw"], C_GW, f"{what} gw")
    if gb is not None:
        out["gb"] = check(gb, ref["gb"], ref["unit_gb"], C_GB, f"{what} gb")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the emulation
# ---------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def _team(L):
    return 64 if L <= WAVE_MAX else 512


def _tree(a, b=None):
    """The kernels' row sum of ``a`` (``b`` None) or of ``a * b`` accumulated by fused multiply-adds, ``[rows, L]`` fp32 -> ``[rows, 1]``."""
    rows, L = a.shape
    T = _team(L)
    nch = -(-(-(-L // 8)) // T)
    pad = nch * T * 8 - L

    def cut(t):
        return torch.nn.functional.pad(t, (0, pad)).view(rows, nch, T, 8)

    a = cut(a)
    b = None if b is None else cut(b)
    acc = torch.zeros(rows, T)
    for k in range(nch):
        for j in range(8):
            acc = acc + a[:, k, :, j] if b is None else _fma(a[:, k, :, j], b[:, k, :, j], acc)
    acc = acc.view(rows, T // 64, 64)
    lanes = torch.arange(64)
    for o in (1, 2, 4, 8, 16, 32):
        acc = acc + acc[..., lanes ^ o]
    waves = acc[..., 0]
    s = waves[:, 0]
    for q in range(1, waves.shape[1]):
        s = s + waves[:, q]
    return s[:, None]


def _column_sums(a, b=None):
    """The kernels' ``sum_rows a`` (or ``a * b`` by fused multiply-adds): fp32 per wavefront / workgroup over its rows in order,
    the four wavefronts of a workgroup in order in fp32, the workgroups in float64."""
    rows, L = a.shape
    wave = L <= WAVE_MAX
    teams = min(-(-rows // 4), BWD_WAVE_GRID) * 4 if wave else min(rows, BWD_BLOCK_GRID)
    acc = torch.zeros(teams, L)
    for lo in range(0, rows, teams):
        n = min(teams, rows - lo)
        acc[:n] = acc[:n] + a[lo:lo + n] if b is None else _fma(a[lo:lo + n], b[lo:lo + n], acc[:n])
    if wave:
        acc = acc.view(teams // 4, 4, L)
        fold = acc[:, 0]
        for q in range(1, 4):
            fold = fold + acc[:, q]
        acc = fold
    return acc.double().sum(0).float()


def emulate(x, r=None, w=None, b=None, eps=1e-5, gy=None, gy2=None, gs=None, y_dtype=torch.float32):
    """The kernels' arithmetic on the CPU: y (``y_dtype``), y2 (bf16), s, stats and, with a gradient, gx (x's dtype), gw, gb."""
    rows, L = x.shape
    fl = torch.tensor(float(L))
    s = x.float() if r is None else x.float() + r.float()
    wf = torch.ones(L) if w is None else w.float()
    bf = torch.zeros(L) if b is None else b.float()
    mean = _tree(s) / fl
    d = s - mean
    rstd = 1.0 / torch.sqrt(_tree(d, d) / fl + torch.tensor(float(eps)))
    xh = d * rstd
    v = _fma(wf.expand_as(xh), xh, bf.expand_as(xh))
    out = dict(y=v.to(y_dtype), y2=v.bfloat16(), s=s, stats=torch.cat([mean, rstd], 1))
    if gy is not None or gy2 is not None or gs is not None:
        g = torch.zeros_like(s)
        if gy is not None:
            g = gy.float() if gy2 is None else gy.float() + gy2.float()
        elif gy2 is not None:
            g = gy2.float()
        wg = wf * g
        m1, m2 = _tree(wg) / fl, _tree(wg, xh) / fl
        gx = rstd * ((wg - m1) - xh * m2)
        if gs is not None:
            gx = gx + gs.float()
        out.update(gx=gx.to(x.dtype), gw=_column_sums(g, xh), gb=_column_sums(g))
    return out


def emulation_worst(shapes=None, seeds=EMU_SEEDS):
    """The worst ratios of the emulation: a dict over y, gx, gw, gb, stat (fp32 and bf16 results both count)."""
    worst = dict(y=0.0, gx=0.0, gw=0.0, gb=0.0, stat=0.0)
    for rows, L in (EMU_SHAPES if shapes is None else shapes):
        for dist in EMU_DISTS:
            for seed in range(seeds):
                t = make_inputs(rows, L, dist, seed)
                ref = reference(t["x"], t["r"], t["w"], t["b"], 1e-5, t["gy"], t["gy2"], t["gs"])
                for lowp in (False, True):
                    x = t["x"].bfloat16() if lowp else t["x"]
                    if lowp:
                        ref = reference(x, t["r"], t["w"], t["b"], 1e-5, t["gy"], t["gy2"], t["gs"])
                    emu = emulate(x, t["r"], t["w"], t["b"], 1e-5, t["gy"], t["gy2"], t["gs"], torch.bfloat16 if lowp else torch.float32)
                    worst["y"] = max(worst["y"], float(excess_ratio(emu["y"], ref["y"], ref["unit_y"]).max()),
                                     float(excess_ratio(emu["y2"], ref["y"], ref["unit_y"]).max()))
                    worst["gx"] = max(worst["gx"], float(excess_ratio(emu["gx"], ref["gx"], ref["unit_gx"]).max()))
                    worst["gw"] = max(worst["gw"], float(excess_ratio(emu["gw"], ref["gw"], ref["unit_gw"]).max()))
                    worst["gb"] = max(worst["gb"], float(excess_ratio(emu["gb"], ref["gb"], ref["unit_gb"]).max()))
                    worst["stat"] = max(worst["stat"], float(excess_ratio(emu["stats"][:, 0], ref["mean"], ref["unit_mean"]).max()),
                                        float(excess_ratio(emu["stats"][:, 1], ref["rstd"], ref["unit_rstd"]).max()))
    return worst


if __name__ == "__main__":
    for name, v in emulation_worst().items():
        print(f"EMU_WORST_{name.upper()} = {v:.3f}   -> constant {math.ceil(2 * v)}")
