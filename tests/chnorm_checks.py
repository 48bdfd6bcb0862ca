"""Reference, magnitudes and bounds for the channel layer norm kernels (csrc/chnorm.hip); a plain module like toknorm_checks.py.

The mathematics is that of the trailing-axis norm with rows = (b, p) and L = C: ``rows`` / ``field`` map ``[B, C, P]`` to
``[B P, C]`` and back, and the float64 reference, the units and the check functions are those of toknorm_checks.py
(``reference`` without residual, second gradient or ``gs``; ``excess_ratio``; ``check``), with ``u = 2^-24``:

    |z  - ref| <= [ulp_bf16 if bf16] + C_Y  u unit_y         z = w xh + b, the plain result
    |gx - ref| <= [ulp_bf16 if bf16] + C_GX u unit_gx,       |gw - ref| <= C_GW u unit_gw,       |gb - ref| <= C_GB u unit_gb
    |mean - ref| <= C_STAT u unit_mean,                      |rstd - ref| <= C_STAT u unit_rstd   (per pixel)

New here: the fused exact GELU.  The forward applies ``Act<TO>`` (by the dtype ``y`` is stored in), the backward ``Act<TX>`` (by
the dtype of ``x``); ``Act<float>`` is ``erff`` (+ ``__expf`` for the derivative), ``Act<bf16>`` the Abramowitz-Stegun 7.1.26 normal
CDF of csrc/gelu.h, |error| < 0.75e-7 absolute on the CDF.  The reference is the exact GELU in float64 either way.

    y = gelu(z):        unit_y(fused) = GELU_GRAD_MAX unit_y(z) + |gelu(z)| [+ (0.75e-7 / u) |z| for Act<bf16>]
    g = gy gelu'(z):    g is off by |gy| (max|gelu''| dz + d'), max|gelu''| = 2 phi(0) = 0.80, dz in units of unit_y(z),
                        d' the absolute error of the derivative formula in fp32 (``DGELU``: measured on the CPU against float64
                        over z in [-12, 12] by ``dgelu_abs_error``, recorded as ``EMU_DGELU_*``, allowed twice that);
                        in units of u:  dg = |gy| (0.80 unit_y(z) + d' / u)

and ``dg`` enters the units of the gradients, which otherwise take ``|g|``, the way ``|g|`` itself does:

    unit_gx += rstd (|w| dg + mean_row(|w| dg) + |xh| mean_row(|w| dg |xh|)),    unit_gw += sum_rows dg |xh|,    unit_gb += sum_rows dg

The constants are NOT taken from the kernels.  ``emulate`` is a CPU emulation of the kernels' arithmetic in fp32 torch ops, as the
header of csrc/chnorm.hip states it.  Forward: a lane adds the channels c = rg, rg + 64, ... of its row group in increasing c, the
64 partials are added in the order 0 ... 63 and divided by ``(float)C``; the variance accumulates ``d d`` by ``fmaf`` in the same
order; ``rstd = 1 / sqrtf(var + eps)``; ``z = fmaf(w, (x - m) r, b)``.  Backward: ``s1 += w g`` unfused, ``s2 = fmaf(w g, xh, s2)``,
folded the same way; ``gx = r ((w g - m1) - xh m2)``; ``gw`` / ``gb``: a lane's V pixels by ``fmaf`` / add, an xor tree over the 8
lanes of a row, fp32 accumulation over the workgroup's tiles in the order blockIdx, + grid, ..., the workgroups' slots in float64.
The tile width (8 V = 32 or 64 pixels, by the wider of x and gy) and the grid are parameters, so the multi-tile order is the
kernel's at shapes small enough for the CPU.  Fused multiply-adds are formed in float64 and rounded (the product of two fp32
numbers is exact there).  Over ``EMU_SHAPES`` (with at least 3 and up to 32 tiles per workgroup) x toknorm_checks.EMU_DISTS x
``EMU_PAIRS`` x plain / fused x ``EMU_SEEDS`` seeds (one for a shape of more than 2^20 elements) its worst ratios to the units
above are the ``EMU_WORST_*`` figures; each constant is twice that figure, rounded up, the factor 2 for the hardware's erff / exp
/ reciprocal and its square root.
tests/test_chnorm_cpu.py asserts that the emulation stays within HALF of each constant.
"""
import math

import torch

import kernel_checks as kc
import toknorm_checks as tc
from toknorm_checks import U, check, excess_ratio        # noqa: F401  (the tests take them from here)

F32, BF16 = torch.float32, torch.bfloat16
K_RG, K_LANES = 64, 8                 # row groups of a workgroup; lanes along a channel row of a tile
BWD_GRID = 1024                       # kBwdGrid: at most this many persistent workgroups
GELU2_MAX = 0.80                      # max |gelu''| = 2 phi(0) = 0.7979
AS_CDF_ERR = 0.75e-7                  # |error| of the Abramowitz-Stegun CDF that csrc/gelu.h documents (1.5e-7 on erf)

# |formula in fp32 - gelu'(z) in float64|, worst over 2^20 + 1 points of [-12, 12] (``dgelu_abs_error``, measured on the CPU)
EMU_DGELU = {F32: 1.343e-7, BF16: 2.852e-7}
DGELU = {F32: 2.7e-7, BF16: 5.8e-7}   # twice, rounded up

# (B, C, P, backward grid): one short tile; C over 64 and no multiple of it with a tail; whole tiles; the model width; two wide
# ones; 213 / 108 tiles on 64 workgroups (3 and 4 per workgroup, a ragged tile in the middle); 32 tiles per workgroup; C = 3;
# 3300 pixels at a width beyond the backward's on-chip limit (the worst ratio over many pixels grows with their number, and the
# GPU tests run this shape; more than a million elements: one seed)
EMU_SHAPES = [(2, 5, 15, BWD_GRID), (1, 73, 36, BWD_GRID), (1, 64, 96, BWD_GRID), (1, 384, 100, BWD_GRID), (1, 600, 40, BWD_GRID),
              (1, 1216, 12, BWD_GRID), (3, 4, 2250, 64), (1, 8, 8192, 8), (3000, 3, 1, 256), (1100, 557, 3, BWD_GRID)]
EMU_PAIRS = [(F32, F32), (BF16, BF16), (BF16, F32), (F32, BF16)]            # (x dtype, y and gy dtype)
EMU_SEEDS = 2
# worst ratios of the emulation over EMU_SHAPES x EMU_DISTS x EMU_PAIRS x {plain, fused} x EMU_SEEDS (measured on the CPU)
EMU_WORST_Y = 5.447
EMU_WORST_GX = 4.479
EMU_WORST_GW = 1.289
EMU_WORST_GB = 1.612
EMU_WORST_STAT = 9.595
C_Y = 11.0
C_GX = 9.0
C_GW = 3.0
C_GB = 4.0
C_STAT = 20.0


def rows(t):
    """``[B, C, P] -> [B P, C]`` (a copy)."""
    B, C, P = t.shape
    return t.permute(0, 2, 1).reshape(B * P, C)


def field(t, B):
    """``[B P, C] -> [B, C, P]`` (a copy)."""
    R, C = t.shape
    return t.view(B, R // B, C).permute(0, 2, 1).contiguous()


def bwd_tile_px(x_dtype, g_dtype):
    """Pixels of a backward tile: eight 16-byte vectors of the wider of x and gy."""
    return K_LANES * 16 // max(torch.empty((), dtype=x_dtype).element_size(), torch.empty((), dtype=g_dtype).element_size())


def make_inputs(B, C, P, dist="n53", seed=0, x_dtype=F32, g_dtype=F32):
    """x from the distribution, gy N(0, 1), w N(1, 0.5^2), b N(0, 0.5^2): a dict of CPU tensors, the fields ``[B, C, P]``."""
    g = torch.Generator().manual_seed(seed * 1000003 + B * 7919 + C * 131 + P)
    m, sd = tc.EMU_DISTS[dist]
    n = lambda *shape: torch.randn(*shape, generator=g)
    return dict(x=(m + sd * n(B, C, P)).to(x_dtype), gy=n(B, C, P).to(g_dtype), w=1.0 + 0.5 * n(C), b=0.5 * n(C))


def reference(x, w=None, b=None, eps=1e-6, gy=None, fuse=False, act_fwd=F32, act_bwd=F32):
    """float64 values and the units of the bounds, everything in the rows layout ``[B P, C]`` (stats ``[B P]``).  ``act_fwd`` /
    ``act_bwd``: the dtype ``y`` is stored in and the dtype of ``x``, which select the kernels' GELU formulas."""
    xr = rows(x.double().cpu())
    L = xr.shape[1]
    plain = tc.reference(xr, None, w, b, eps)
    z, unit_z = plain["y"], plain["unit_y"]
    ref = dict(plain, z=z, unit_z=unit_z)
    if fuse:
        ref["y"] = kc.gelu64(z)
        ref["unit_y"] = kc.GELU_GRAD_MAX * unit_z + ref["y"].abs() + (AS_CDF_ERR / U * z.abs() if act_fwd == BF16 else 0.0)
    if gy is not None:
        gyr = rows(gy.double().cpu())
        g = gyr * kc.gelu_grad64(z) if fuse else gyr
        full = tc.reference(xr, None, w, b, eps, gy=g)
        ref.update({k: full[k] for k in ("gx", "unit_gx", "gw", "unit_gw", "gb", "unit_gb")})
        if fuse:
            wa = torch.ones(L, dtype=torch.float64) if w is None else w.double().cpu().abs()
            rstd = plain["rstd"][:, None]
            xha = ((xr - plain["mean"][:, None]) * rstd).abs()
            dg = gyr.abs() * (GELU2_MAX * unit_z + DGELU[act_bwd] / U)
            wdg = wa * dg
            ref["unit_gx"] = ref["unit_gx"] + rstd * (wdg + wdg.mean(1, keepdim=True) + xha * (wdg * xha).mean(1, keepdim=True))
            ref["unit_gw"] = ref["unit_gw"] + (dg * xha).sum(0)
            ref["unit_gb"] = ref["unit_gb"] + dg.sum(0)
    return ref


def check_forward(ref, y=None, stats=None, what=""):
    """``y [B P, C]`` and ``stats [B P, 2]`` against the reference: the worst ratios of whatever is given, a dict."""
    out = {}
    if y is not None:
        out["y"] = check(y, ref["y"], ref["unit_y"], C_Y, f"{what} y")
    if stats is not None:
        out["mean"] = check(stats[:, 0], ref["mean"], ref["unit_mean"], C_STAT, f"{what} mean")
        out["rstd"] = check(stats[:, 1], ref["rstd"], ref["unit_rstd"], C_STAT, f"{what} rstd")
    return out


def check_backward(ref, gx=None, gw=None, gb=None, what=""):
    out = {}
    if gx is not None:
        out["gx"] = check(gx, ref["gx"], ref["unit_gx"], C_GX, f"{what} gx")
    if gw is not None:
        out["gw"] = check(gw, ref["gw"], ref["unit_gw"], C_GW, f"{what} gw")
    if gb is not None:
        out["gb"] = check(gb, ref["gb"], ref["unit_gb"], C_GB, f"{what} gb")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the emulation
# ---------------------------------------------------------------------------------------------------------------------
_fma = tc._fma


def _f(v):
    return torch.tensor(v, dtype=F32)


def _cdf_pdf(x):
    """``normal_cdf_pdf`` of csrc/gelu.h in fp32."""
    z = x.abs() * _f(0.70710678118654752)
    t = 1.0 / _fma(_f(0.3275911), z, _f(1.0))
    q = _fma(_f(1.061405429), t, _f(-1.453152027))
    for c in (1.421413741, -0.284496736, 0.254829592):
        q = _fma(q, t, _f(c))
    e = torch.exp2(_f(-1.4426950408889634) * z * z)
    half_erfc = _f(0.5) * q * t * e
    return torch.where(x < 0, half_erfc, 1.0 - half_erfc), _f(0.3989422804014327) * e


def gelu_emu(z, act):
    if act == BF16:
        return z * _cdf_pdf(z)[0]
    return _f(0.5) * z * (1.0 + torch.erf(z * _f(0.70710678118654752440)))


def gelu_grad_emu(z, act):
    if act == BF16:
        Phi, phi = _cdf_pdf(z)
        return _fma(z, phi, Phi)
    return _f(0.5) * (1.0 + torch.erf(z * _f(0.70710678118654752440))) + z * _f(0.39894228040143267794) * torch.exp(_f(-0.5) * z * z)


def dgelu_abs_error(act, n=(1 << 20) + 1):
    z = torch.linspace(-12.0, 12.0, n, dtype=torch.float64).float()
    return float((gelu_grad_emu(z, act).double() - kc.gelu_grad64(z.double())).abs().max())


def _chan_sum(a, b=None):
    """The kernels' sum over the channels of ``a`` (or of ``a b`` by fused multiply-adds), ``[R, C]`` fp32 -> ``[R, 1]``: row group
    rg adds c = rg, rg + 64, ... in increasing c, the 64 partials are added in the order 0 ... 63."""
    R, C = a.shape
    nch = -(-C // K_RG)
    pad = nch * K_RG - C
    cut = lambda t: torch.nn.functional.pad(t, (0, pad)).view(R, nch, K_RG)
    a = cut(a)
    b = None if b is None else cut(b)
    acc = torch.zeros(R, K_RG)
    for k in range(nch):
        acc = acc + a[:, k] if b is None else _fma(a[:, k], b[:, k], acc)
    s = torch.zeros(R)
    for rg in range(K_RG):
        s = s + acc[:, rg]
    return s[:, None]


def _tile_sums(g, xh, B, tp, grid, drop=None):
    """The kernels' ``sum_{b, p} g xh`` (``xh`` None: ``sum g``) per channel, ``[B P, C]`` fp32 -> ``[C]``: per tile of ``tp``
    pixels a lane's V pixels in order, the xor tree over the 8 lanes, the workgroup's tiles in fp32 in the order blockIdx,
    + grid, ..., the workgroups in float64.  ``drop = (workgroup, iteration)``: that tile's sums are lost (a defect)."""
    R, C = g.shape
    P, V = R // B, tp // K_LANES
    tps = -(-P // tp)

    def tiles(t):      # [B P, C] -> [B tps, C, 8, V], pixels past the field zero
        t = torch.nn.functional.pad(t.view(B, P, C).permute(0, 2, 1), (0, tps * tp - P))
        return t.reshape(B, C, tps, K_LANES, V).permute(0, 2, 1, 3, 4).reshape(B * tps, C, K_LANES, V)

    g = tiles(g)
    xh = None if xh is None else tiles(xh)
    a = torch.zeros(B * tps, C, K_LANES)
    for i in range(V):
        a = a + g[..., i] if xh is None else _fma(g[..., i], xh[..., i], a)
    lanes = torch.arange(K_LANES)
    for o in (1, 2, 4):
        a = a + a[..., lanes ^ o]
    a = a[..., 0]
    ntiles = B * tps
    grid = min(ntiles, grid)
    acc = torch.zeros(grid, C)
    for it, lo in enumerate(range(0, ntiles, grid)):
        n = min(grid, ntiles - lo)
        add = a[lo:lo + n].clone()
        if drop is not None and drop[1] == it and drop[0] < n:
            add[drop[0]] = 0.0
        acc[:n] = acc[:n] + add
    return acc.double().sum(0).float()


def emulate(x, w=None, b=None, eps=1e-6, gy=None, fuse=False, y_dtype=F32, grid=BWD_GRID, defect=None):
    """The kernels' arithmetic on the CPU for ``x [B, C, P]``: y (``y_dtype``) and gx (x's dtype) in the rows layout, stats
    ``[B P, 2]``, gw, gb.  ``defect`` (for tests/test_chnorm_cpu.py): "drop_tile": workgroup 0 loses the channel sums of its
    second tile; "neighbour_stats": pixel 1 takes the (mean, rstd) of pixel 0; "one_pass": ``var = E[x^2] - mean^2``."""
    B, C, P = x.shape
    fl = _f(float(C))
    s = rows(x).float()
    wf = torch.ones(C) if w is None else w.float()
    bf = torch.zeros(C) if b is None else b.float()
    mean = _chan_sum(s) / fl
    d = s - mean
    var = _chan_sum(d, d) / fl
    if defect == "one_pass":
        var = (_chan_sum(s, s) / fl - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + _f(float(eps)))
    if defect == "neighbour_stats":
        mean, rstd = mean.clone(), rstd.clone()
        mean[1], rstd[1] = mean[0], rstd[0]
        d = s - mean
    xh = d * rstd
    z = _fma(wf.expand_as(xh), xh, bf.expand_as(xh))
    out = dict(y=(gelu_emu(z, y_dtype) if fuse else z).to(y_dtype), stats=torch.cat([mean, rstd], 1))
    if gy is not None:
        g = rows(gy).float()
        if fuse:
            g = g * gelu_grad_emu(z, x.dtype)
        wg = wf * g
        m1, m2 = _chan_sum(wg) / fl, _chan_sum(wg, xh) / fl
        tp = bwd_tile_px(x.dtype, gy.dtype)
        drop = (0, 1) if defect == "drop_tile" else None
        out.update(gx=(rstd * ((wg - m1) - xh * m2)).to(x.dtype), gw=_tile_sums(g, xh, B, tp, grid, drop), gb=_tile_sums(g, None, B, tp, grid, drop))
    return out


def ratios(emu, ref):
    """The worst ratio of every result of ``emulate`` to its unit: a dict over y, gx, gw, gb, stat."""
    out = dict(y=float(excess_ratio(emu["y"], ref["y"], ref["unit_y"]).max()),
               stat=max(float(excess_ratio(emu["stats"][:, 0], ref["mean"], ref["unit_mean"]).max()),
                        float(excess_ratio(emu["stats"][:, 1], ref["rstd"], ref["unit_rstd"]).max())))
    for k in ("gx", "gw", "gb"):
        if k in emu:
            out[k] = float(excess_ratio(emu[k], ref[k], ref["unit_" + k]).max())
    return out


def emulation_worst(shapes=None, seeds=EMU_SEEDS):
    worst = dict(y=0.0, gx=0.0, gw=0.0, gb=0.0, stat=0.0)
    for B, C, P, grid in (EMU_SHAPES if shapes is None else shapes):
        for dist in tc.EMU_DISTS:
            for seed in range(seeds if B * C * P <= 1 << 20 else 1):
                for xd, gd in EMU_PAIRS:
                    t = make_inputs(B, C, P, dist, seed, xd, gd)
                    for fuse in (False, True):
                        ref = reference(t["x"], t["w"], t["b"], 1e-6, t["gy"], fuse, gd, xd)
                        emu = emulate(t["x"], t["w"], t["b"], 1e-6, t["gy"], fuse, gd, grid)
                        for k, v in ratios(emu, ref).items():
                            worst[k] = max(worst[k], v)
    return worst


if __name__ == "__main__":
    for act, name in ((F32, "F32"), (BF16, "BF16")):
        print(f"EMU_DGELU[{name}] = {dgelu_abs_error(act):.3e}")
    for name, v in emulation_worst().items():
        print(f"EMU_WORST_{name.upper()} = {v:.3f}   -> constant {math.ceil(2 * v)}")
