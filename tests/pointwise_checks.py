"""Reference, magnitudes and bounds for the instance norm and the streaming helpers of csrc/pointwise.hip; a plain module like
chnorm_checks.py, whose GELU terms (``GELU2_MAX``, ``DGELU``, ``AS_CDF_ERR``, the fp32 formulas) it shares.

A field is ``x [rows = B C][P]``, row r takes the parameters of channel ``r % C``.  Reference: float64 on the operands as they are.
What is bounded is the kernels' DOCUMENTED arithmetic, one-pass sums: ``rowsum2_kernel`` forms ``sum x`` and ``sum x^2`` (fp32 per
thread over the 4 x 8 elements it visits, a shuffle fold over the wave, four waves, fp64 across workgroups) and the apply pass
``var = E[x^2] - mean^2`` in fp64.  The rounding of ``sum x^2`` is relative to ``sum x^2``, not to the variance, so with
``u = 2^-24``, per row,

    |mean - ref| <= C_MEAN u mean|x|
    |rstd - ref| <= C_RSTD u unit_rstd,    unit_rstd = rstd (1 + rstd^2 mean(x^2)) = rstd kappa

THE RSTD UNIT GROWS AS (mean / std)^2: ``rstd^2 mean(x^2) = 1 + (mean / std)^2``.  That is the price of the one-pass sums, which the
irfft epilogue and ``pce_gemm(want_row_sums=True)`` produce as well; the two-pass unit of toknorm_checks.py,
``rstd (1 + rstd mean(|xh| (|x| + mean|x|)))``, grows as ``mean / std`` only.  The emulation below (``conditioning_table``, 8 rows
each of P = 2112, 8184, 16392 and 115200, fp32) reaches, as |rstd - ref| / ref and as ratios to either unit:

    input         rstd relative error    in two-pass units    in one-pass units
    N(5, 3^2)     3.3e-7                 1.4                  1.2
    N(50, 1)      1.7e-4                 34                   1.1
    N(50, 0.1^2)  2.6e-2                 537                  1.7

tests/test_pointwise_cpu.py pins both columns: within half of ``C_RSTD`` in one-pass units, more than 20 times the two-pass
unit at N(50, 1).  Everything downstream carries ``kappa``:

    y = fmaf(x, sc, sh), sc = rstd w, sh = b - mean sc:
        unit_y = |x sc| + |mean sc| + |b|  +  |sc| mean|x|  +  |w xh| kappa          (roundings; what d mean and d rstd move it by)
    backward, on the saved fp32 (mean, rstd): xh is off by e u, e = |xh| (1 + kappa) + rstd (|x| + 2 mean|x|), and
        gx = k (g - m1 - xh m2), k = w rstd:
        unit_gx = |k| (|g| + S1 + |xh| S2 + e S2 + |xh| mean(|g| e)) + |gx| kappa,   S1 = mean|g|, S2 = mean|g xh|
        unit_gb = sum|g|,   unit_gw = sum|g| e        (per row: the workspace sums; per channel: the parameter gradients)
    fused GELU: as in chnorm_checks.py, ``Act<T>`` by the field's dtype both ways;
        unit_y(fused) = GELU_GRAD_MAX unit_y + |gelu(z)| [+ (0.75e-7 / u) |z| for bf16]
        dg = |gy| (0.80 (|w| e + |b|) + d' / u) enters unit_gx, unit_gw, unit_gb the way |g| does
    mk_instnorm_coeffs:  unit_sc = |w| unit_rstd + |sc|,   unit_sh = |b| + 2 |mean sc| + |sc| mean|x| + |mean| unit_sc
    mk_affine_add, y = r + fmaf(z, a, b):  unit = |a z + b| + |y|        (one fused multiply-add and one addition)
    mk_bias_gelu_fwd, y = gelu(x + b):     unit = GELU_GRAD_MAX |x + b| + |y| [+ (0.75e-7 / u) |x + b| for bf16]
    mk_bias_gelu_bwd, gx = gy gelu'(x + b): unit = |gy| (0.80 |x + b| + d' / u) + |gx|;  gbias = sum gx: unit = sum of the former,
        and, the workgroups' sums being added by fp32 atomics, ``kernel_checks.x3_slack_sum`` over the workgroups per channel

The constants are NOT taken from the kernels: ``emulate_instnorm`` and the small emulations next to it are the kernels' arithmetic in
fp32 torch ops on the CPU, the ``EMU_WORST`` figures their worst ratios over ``EMU_P`` x ``EMU_DISTS`` x fp32 / bf16 x plain / fused x ``EMU_SEEDS`` seeds,
each constant twice its figure, rounded up.  ``python tests/pointwise_checks.py`` prints them and the table.
"""
import math

import torch

import chnorm_checks as cc
import kernel_checks as kc
from toknorm_checks import U, check, excess_ratio        # noqa: F401

F32, BF16 = torch.float32, torch.bfloat16
K_T, K_E, K_STEPS = 256, 8, 4
CHUNK = K_T * K_E * K_STEPS                               # kChunk: the elements of a row one workgroup visits
EPS = 1e-6

EMU_DISTS = {"n53": (5.0, 3.0), "n501": (50.0, 1.0)}      # what the GPU tests run
TABLE_DISTS = {"n53": (5.0, 3.0), "n501": (50.0, 1.0), "n5001": (50.0, 0.1)}
EMU_P = [8, 8184, 8192, 8200, 16392]
EMU_SEEDS = 6                                             # the GPU tests draw their inputs with seeds 0 ... 5
# worst ratios of the emulations (measured on the CPU) and the constants, twice that, rounded up
EMU_WORST = dict(mean=2.443, rstd=2.183, y=2.166, gx=2.155, gw=1.294, gb=1.294, sc=2.182, sh=2.181, affine=0.998, bg_y=1.299, bg_gx=0.466,
                 bg_gb=0.096)
C = dict(mean=5.0, rstd=5.0, y=5.0, gx=5.0, gw=3.0, gb=3.0, sc=5.0, sh=5.0, affine=2.0, bg_y=3.0, bg_gx=1.0, bg_gb=1.0)
# the conditioning table of the docstring: dist -> (relative error of rstd, ratio to the two-pass unit, ratio to the one-pass unit)
EMU_TABLE = {"n53": (3.25e-7, 1.44, 1.15), "n501": (1.68e-4, 33.96, 1.07), "n5001": (2.57e-2, 537.17, 1.71)}


def make_inputs(rows, P, nch, dist="n53", seed=0, dtype=F32):
    """x from the distribution, gy, r N(0, 1), w N(1, 0.5^2), b N(0, 0.5^2) per channel: CPU tensors."""
    g = torch.Generator().manual_seed(seed * 1000003 + rows * 7919 + P)
    m, sd = TABLE_DISTS[dist]
    n = lambda *shape: torch.randn(*shape, generator=g)
    return dict(x=(m + sd * n(rows, P)).to(dtype), gy=n(rows, P).to(dtype), r=n(rows, P).to(dtype), w=1.0 + 0.5 * n(nch), b=0.5 * n(nch))


def _per_row(v, rows, nch):
    """The parameter of every row, ``[rows, 1]`` float64."""
    return v.double()[torch.arange(rows) % nch][:, None]


def reference(x, w, b, nch, eps=EPS):
    """float64 values and the units of the forward for ``x [rows, P]`` (``w`` / ``b`` None: 1 / 0), and the intermediates the other
    functions take."""
    x = x.double().cpu()
    rows, P = x.shape
    dt = x.dtype
    wr = torch.ones(rows, 1, dtype=dt) if w is None else _per_row(w, rows, nch)
    br = torch.zeros(rows, 1, dtype=dt) if b is None else _per_row(b, rows, nch)
    mean = x.mean(1, keepdim=True)
    var = (x - mean).square().mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (x - mean) * rstd
    xabs = x.abs().mean(1, keepdim=True)
    kappa = 1.0 + rstd * rstd * x.square().mean(1, keepdim=True)
    sc = rstd * wr
    sh = br - mean * sc
    z = wr * xh + br
    unit_z = (x * sc).abs() + (mean * sc).abs() + br.abs() + sc.abs() * xabs + (wr * xh).abs() * kappa
    ref = dict(mean=mean[:, 0], rstd=rstd[:, 0], unit_mean=xabs[:, 0], unit_rstd=(rstd * kappa)[:, 0],
               unit_rstd_two_pass=(rstd * (1.0 + rstd * (xh.abs() * (x.abs() + xabs)).mean(1, keepdim=True)))[:, 0],
               sums=torch.cat([x.sum(1, keepdim=True), x.square().sum(1, keepdim=True)], 1), z=z, y=z, unit_y=unit_z,
               sc=sc[:, 0], sh=sh[:, 0], unit_sc=(wr.abs() * rstd * kappa + sc.abs())[:, 0])
    ref["unit_sh"] = (br.abs() + 2 * (mean * sc).abs() + sc.abs() * xabs)[:, 0] + mean[:, 0].abs() * ref["unit_sc"]
    return ref, dict(x=x, wr=wr, br=br, mean=mean, rstd=rstd, xh=xh, xabs=xabs, kappa=kappa, z=z, unit_z=unit_z)


def forward_units(ref, mid, fuse, act):
    """The units of ``y`` with the activation of dtype ``act`` fused (in place in ``ref``)."""
    if fuse:
        z = mid["z"]
        ref["y"] = kc.gelu64(z)
        ref["unit_y"] = kc.GELU_GRAD_MAX * mid["unit_z"] + ref["y"].abs() + (cc.AS_CDF_ERR / U * z.abs() if act == BF16 else 0.0)
    return ref


def backward_reference(ref, mid, gy, fuse, act, nch):
    """gx and its unit; the row sums ``bsums [rows, 2] = (sum g, sum g xh)`` and the parameter gradients ``gw, gb [nch]`` (summed over
    the rows of a channel) with their units (in place in ``ref``)."""
    gy = gy.double().cpu()
    x, wr, br, rstd, xh, xabs, kappa, z = (mid[k] for k in ("x", "wr", "br", "rstd", "xh", "xabs", "kappa", "z"))
    rows = x.shape[0]
    g = gy * kc.gelu_grad64(z) if fuse else gy
    k = wr * rstd
    e = xh.abs() * (1.0 + kappa) + rstd * (x.abs() + 2 * xabs)
    gx = k * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    S1, S2 = g.abs().mean(1, keepdim=True), (g * xh).abs().mean(1, keepdim=True)
    unit_gx = k.abs() * (g.abs() + S1 + xh.abs() * S2 + e * S2 + xh.abs() * (g.abs() * e).mean(1, keepdim=True)) + gx.abs() * kappa
    unit_s1, unit_s2 = g.abs().sum(1), (g.abs() * e).sum(1)
    if fuse:
        dg = gy.abs() * (cc.GELU2_MAX * (wr.abs() * e + br.abs()) + cc.DGELU[act] / U)
        unit_gx = unit_gx + k.abs() * (dg + dg.mean(1, keepdim=True) + xh.abs() * (dg * xh.abs()).mean(1, keepdim=True))
        unit_s1, unit_s2 = unit_s1 + dg.sum(1), unit_s2 + (dg * xh.abs()).sum(1)
    chan = lambda v: v.view(rows // nch, nch).sum(0)
    s1, s2 = g.sum(1), (g * xh).sum(1)
    ref.update(gx=gx, unit_gx=unit_gx, bsums=torch.stack([s1, s2], 1), unit_bsums=torch.stack([unit_s1, unit_s2], 1),
               gw=chan(s2), unit_gw=chan(unit_s2), gb=chan(s1), unit_gb=chan(unit_s1))
    return ref


def instnorm_reference(x, w, b, nch, eps=EPS, gy=None, fuse=False):
    """Everything of the instance norm at once; the activation is that of x's dtype."""
    ref, mid = reference(x, w, b, nch, eps)
    forward_units(ref, mid, fuse, x.dtype)
    if gy is not None:
        backward_reference(ref, mid, gy, fuse, x.dtype, nch)
    return ref


# ---------------------------------------------------------------------------------------------------------------------
# the emulations
# ---------------------------------------------------------------------------------------------------------------------
_fma, _f = cc._fma, cc._f


def row_sums(a, b=None):
    """``rowsum2_kernel`` / ``instnorm_bwd_sums_kernel``: ``sum a`` (or ``sum a b`` by fused multiply-adds) per row, ``[rows, P]`` fp32
    -> ``[rows]`` float64.  A thread adds the 8 elements of each of its 4 steps in order in fp32, the 64 lanes fold by the
    ``shfl_down`` tree, the four waves are added in order, the workgroups in float64 (every per-workgroup value is exact)."""
    rows, P = a.shape
    nwg = -(-P // CHUNK)
    cut = lambda t: torch.nn.functional.pad(t, (0, nwg * CHUNK - P)).view(rows, nwg, K_STEPS, K_T, K_E)
    a = cut(a)
    b = None if b is None else cut(b)
    acc = torch.zeros(rows, nwg, K_T)
    for s in range(K_STEPS):
        for i in range(K_E):
            acc = acc + a[:, :, s, :, i] if b is None else _fma(a[:, :, s, :, i], b[:, :, s, :, i], acc)
    v = acc.view(rows, nwg, 4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v[..., :o] + v[..., o:2 * o]
    v = v[..., 0]
    wg = ((v[..., 0] + v[..., 1]) + v[..., 2]) + v[..., 3]
    return wg.double().sum(1)


def emulate_instnorm(x, w, b, nch, eps=EPS, gy=None, fuse=False):
    """The kernels' arithmetic on the CPU: sums ``[rows, 2]`` float64, stats ``[rows, 2]``, affine ``[rows, 2]``, y and, with ``gy``,
    bsums ``[rows, 2]`` float64, gx, gw, gb."""
    rows, P = x.shape
    xf = x.float()
    idx = torch.arange(rows) % nch
    wr = (torch.ones(nch) if w is None else w.float())[idx][:, None]
    br = (torch.zeros(nch) if b is None else b.float())[idx][:, None]
    sums = torch.stack([row_sums(xf), row_sums(xf, xf)], 1)
    mean_d = sums[:, 0] / P
    var_d = (sums[:, 1] / P - mean_d * mean_d).clamp_min(0.0)
    mean, rstd = mean_d.float()[:, None], (1.0 / torch.sqrt(var_d + float(_f(eps)))).float()[:, None]
    sc = rstd * wr
    sh = br - mean * sc
    z = _fma(xf, sc.expand_as(xf), sh.expand_as(xf))
    out = dict(sums=sums, stats=torch.cat([mean, rstd], 1), affine=torch.cat([sc, sh], 1), y=(cc.gelu_emu(z, x.dtype) if fuse else z).to(x.dtype))
    if gy is not None:
        xh = (xf - mean) * rstd
        g = gy.float()
        if fuse:
            g = g * cc.gelu_grad_emu(_fma(xh, wr.expand_as(xh), br.expand_as(xh)), x.dtype)
        s1, s2 = row_sums(g), row_sums(g, xh)
        m1, m2 = (s1 / P).float()[:, None], (s2 / P).float()[:, None]
        gx = (wr * rstd) * ((g - m1) - xh * m2)
        chan = lambda v: v.view(rows // nch, nch).sum(0).float()
        out.update(bsums=torch.stack([s1, s2], 1), gx=gx.to(x.dtype), gw=chan(s2), gb=chan(s1))
    return out


def affine_add_reference(r, z, affine):
    r, z, a = r.double().cpu(), z.double().cpu(), affine.double().cpu()
    t = a[:, :1] * z + a[:, 1:]
    return r + t, t.abs() + (r + t).abs()


def bias_gelu_reference(x, bias, nch, gy=None):
    """(y, unit_y) or, with ``gy``, (gx, unit_gx, gbias, unit_gbias); the activation is that of x's dtype."""
    act = x.dtype
    xd = x.double().cpu()
    rows = xd.shape[0]
    v = xd + (0.0 if bias is None else _per_row(bias, rows, nch))
    if gy is None:
        y = kc.gelu64(v)
        return y, kc.GELU_GRAD_MAX * v.abs() + y.abs() + (cc.AS_CDF_ERR / U * v.abs() if act == BF16 else 0.0)
    gyd = gy.double().cpu()
    gx = gyd * kc.gelu_grad64(v)
    unit = gyd.abs() * (cc.GELU2_MAX * v.abs() + cc.DGELU[act] / U) + gx.abs()
    chan = lambda t: t.sum(1).view(rows // nch, nch).sum(0)
    return gx, unit, chan(gx), chan(unit)


def gbias_slack(gx64, nch, P):
    """fp32 atomic adds of the workgroups' sums of a channel: ``x3_slack_sum`` over their number, on ``sum|gx|``."""
    rows = gx64.shape[0]
    return kc.x3_slack_sum((rows // nch) * -(-P // CHUNK), gx64.abs().sum(1).view(rows // nch, nch).sum(0))


def emulate_bias_gelu(x, bias, nch, gy=None):
    rows, P = x.shape
    v = x.float() + (0.0 if bias is None else bias.float()[torch.arange(rows) % nch][:, None])
    if gy is None:
        return cc.gelu_emu(v, x.dtype).to(x.dtype)
    g = gy.float() * cc.gelu_grad_emu(v, x.dtype)
    wg = row_sums(g).float()                       # one workgroup's fp32 sums added in fp32 (one order of the atomics)
    gb = torch.zeros(nch)
    for r in range(rows):
        gb[r % nch] = gb[r % nch] + wg[r]
    return g.to(x.dtype), gb


def _worst(out, key, v):
    out[key] = max(out.get(key, 0.0), float(v.max()))


def emulation_worst(seeds=EMU_SEEDS):
    worst = {}
    rows, nch = 6, 3
    for P in EMU_P:
        for dist in EMU_DISTS:
            for dtype in (F32, BF16):
                for seed in range(seeds):
                    t = make_inputs(rows, P, nch, dist, seed, dtype)
                    for fuse in (False, True):
                        ref = instnorm_reference(t["x"], t["w"], t["b"], nch, EPS, t["gy"], fuse)
                        emu = emulate_instnorm(t["x"], t["w"], t["b"], nch, EPS, t["gy"], fuse)
                        _worst(worst, "mean", excess_ratio(emu["stats"][:, 0], ref["mean"], ref["unit_mean"]))
                        _worst(worst, "rstd", excess_ratio(emu["stats"][:, 1], ref["rstd"], ref["unit_rstd"]))
                        _worst(worst, "sc", excess_ratio(emu["affine"][:, 0], ref["sc"], ref["unit_sc"]))
                        _worst(worst, "sh", excess_ratio(emu["affine"][:, 1], ref["sh"], ref["unit_sh"]))
                        for k in ("y", "gx", "gw", "gb"):
                            _worst(worst, k, excess_ratio(emu[k], ref[k], ref["unit_" + k]))
                        for q, k in ((0, "gb"), (1, "gw")):
                            _worst(worst, k, excess_ratio(emu["bsums"][:, q].float(), ref["bsums"][:, q], ref["unit_bsums"][:, q]))
                    aff = torch.stack([t["w"][torch.arange(rows) % nch], t["b"][torch.arange(rows) % nch]], 1)
                    y64, unit = affine_add_reference(t["r"], t["gy"], aff)
                    got = (t["r"].float() + _fma(t["gy"].float(), aff[:, :1].expand(rows, P), aff[:, 1:].expand(rows, P))).to(dtype)
                    _worst(worst, "affine", excess_ratio(got, y64, unit))
                    z = make_inputs(rows, P, nch, "n53", seed + 7, dtype)["gy"]                 # pre-activations N(0, 1)
                    y64, unit = bias_gelu_reference(z, t["b"], nch)
                    _worst(worst, "bg_y", excess_ratio(emulate_bias_gelu(z, t["b"], nch), y64, unit))
                    gx64, unit, gb64, unit_gb = bias_gelu_reference(z, t["b"], nch, t["gy"])
                    gx, gb = emulate_bias_gelu(z, t["b"], nch, t["gy"])
                    _worst(worst, "bg_gx", excess_ratio(gx, gx64, unit))
                    _worst(worst, "bg_gb", excess_ratio(gb, gb64, unit_gb))
    return worst


def conditioning_table(lengths=(2112, 8184, 16392, 115200), rows=8):
    """dist -> (worst |rstd - ref| / ref, worst ratio to the two-pass unit, worst ratio to the one-pass unit) of the emulation."""
    out = {}
    for dist in TABLE_DISTS:
        rel = two = one = 0.0
        for P in lengths:
            t = make_inputs(rows, P, 1, dist, 0)
            ref, _ = reference(t["x"], None, None, 1)
            rstd = emulate_instnorm(t["x"], None, None, 1)["stats"][:, 1]
            rel = max(rel, float(((rstd.double() - ref["rstd"]).abs() / ref["rstd"]).max()))
            two = max(two, float(excess_ratio(rstd, ref["rstd"], ref["unit_rstd_two_pass"]).max()))
            one = max(one, float(excess_ratio(rstd, ref["rstd"], ref["unit_rstd"]).max()))
        out[dist] = (rel, two, one)
    return out


if __name__ == "__main__":
    for name, v in emulation_worst().items():
        print(f"EMU_WORST[{name}] = {v:.3f}   -> constant {math.ceil(2 * v)}")
    for dist, (rel, two, one) in conditioning_table().items():
        print(f"{dist}: rstd relative error {rel:.2e}, {two:.2f} two-pass units, {one:.2f} one-pass units")
