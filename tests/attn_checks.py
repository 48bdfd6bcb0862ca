"""Reference, magnitudes and bounds for the attention kernels (csrc/attn.hip); a plain module like kernel_checks.py.

Reference: float64 softmax attention and its gradients on the bf16 operands as they are (``reference``).

Forward bound, every element (``P`` the float64 softmax, ``mag = P @ |V|``):

    |o - ref| <= ulp_bf16(max(|o|, |ref|, rms / 256)) + 2 * 2^-9 * mag + score_slack

The factor 2 is derived: ``P`` is rounded to bf16 once in the numerator (2^-9 relative per term) and the row sum may be taken
over the rounded terms (another 2^-9).  ``score_slack = 2 (D + 4) 2^-23 scale max_j(|q_i| . |k_j|) mag`` covers the fp32
accumulation of the scores: a score off by ``e`` changes a softmax weight by at most ``e`` relative, numerator and denominator.

Backward bound, the same form: one bf16 ulp plus ``c * 2^-9 * mag``, with the float64 expressions of the gradients evaluated
on absolute values as magnitudes:

    mag_dV = P^T @ |dO|,   |dS|_mag = P o (|dO| @ |V|^T + rowsum(|dO| o |O|)),
    mag_dQ = scale |dS|_mag @ |K|,   mag_dK = scale |dS|_mag^T @ |Q|.

The constants are NOT taken from the kernels.  ``emulate`` is a CPU emulation of the kernels' rounding points in fp32 torch
ops: ``P`` and ``dS`` rounded to bf16 before their second products, delta from the stored bf16 ``O``, fp32 elsewhere, the row
sum over the unrounded or over the rounded weights.  At (N, D, input scale) = (65, 32, 1), (200, 64, 1), (257, 128, 1),
(200, 48, 3), (129, 64, 0.3) (``EMU_SHAPES``, ``EMU_SEEDS`` draws each; q and k carry the input scale) its worst ratios of ``(|x - ref| - ulp) / (2^-9 mag)``,
and of ``|lse - ref|`` to ``lse_unit``, are the ``EMU_WORST_*`` figures below; each constant is twice that figure, rounded up,
the factor 2 for the accumulation order and the hardware exp2.  tests/test_attn_cpu.py asserts that the emulation stays
within HALF of each constant, and that the forward emulation stays below the forward bound with its factor at 1.
"""
import math

import torch

import kernel_checks as kc

EMU_SHAPES = [(65, 32, 1.0), (200, 64, 1.0), (257, 128, 1.0), (200, 48, 3.0), (129, 64, 0.3)]

FWD_C = 2.0                      # derived, see above
# worst ratios of the emulation over EMU_SHAPES, both row-sum variants (measured on the CPU, see the module docstring)
EMU_SEEDS = 4
EMU_WORST_FWD1 = 0.79            # |o - ref| over the forward bound with its factor at 1
EMU_WORST_DV = 1.46
EMU_WORST_DQ = 0.46
EMU_WORST_DK = 0.43
EMU_WORST_LSE = 2.37             # the row sum over rounded weights; over unrounded ones 0.10
DV_C = 3.0
DQ_C = 1.0
DK_C = 1.0
LSE_C = 5.0


def reference(q, k, v, go=None, scale=None):
    """float64 attention on ``[..., N, D]`` operands.  Returns a dict: o, lse, P and, with ``go``, dq, dk, dv and the magnitudes."""
    q, k, v = q.double(), k.double(), v.double()
    scale = 1.0 / math.sqrt(q.shape[-1]) if scale is None else scale
    s = scale * q @ k.transpose(-1, -2)
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    o = p @ v
    r = dict(o=o, lse=lse, P=p, scale=scale, mag_o=p @ v.abs(),
             smag=scale * (q.abs() @ k.abs().transpose(-1, -2)).amax(dim=-1))          # scale max_j |q_i| . |k_j|, per row
    if go is not None:
        go = go.double()
        dp = go @ v.transpose(-1, -2)
        delta = (go * o).sum(-1, keepdim=True)
        ds = p * (dp - delta)
        ds_mag = p * (go.abs() @ v.abs().transpose(-1, -2) + (go.abs() * o.abs()).sum(-1, keepdim=True))
        r.update(dv=p.transpose(-1, -2) @ go, dq=scale * ds @ k, dk=scale * ds.transpose(-1, -2) @ q,
                 mag_dv=p.transpose(-1, -2) @ go.abs(), mag_dq=scale * ds_mag @ k.abs(),
                 mag_dk=scale * ds_mag.transpose(-1, -2) @ q.abs())
    return r


def score_slack(ref, D):
    return 2.0 * (D + 4) * 2.0 ** -23 * ref["smag"][..., None] * ref["mag_o"]


def fwd_slack(ref, D, c=FWD_C):
    return c * 2.0 ** -9 * ref["mag_o"] + score_slack(ref, D)


def lse_unit(ref, D):
    """The unit of the lse bound.  A row sum over bf16-rounded weights is off by ``sum_j p_j e_j`` relative, ``|e_j| <= 2^-9``
    independent: ``2^-9 sqrt(sum_j P_ij^2)`` in the root mean square (a dropped key is ``P_ij`` itself, hundreds of units).  An fp32
    evaluation adds, to first order, the accumulation of the largest score and the roundings of the maximum, the logarithm
    and their sum."""
    return 2.0 ** -9 * ref["P"].square().sum(-1).sqrt() + 2.0 ** -23 * ((D + 4) * ref["smag"] + ref["lse"].abs() + 1.0)


def check_forward(o, ref, D, what="", c=FWD_C):
    return kc.bf16_elementwise(o, ref["o"], fwd_slack(ref, D, c), what=f"{what} o")


def check_lse(lse, ref, D, what="", c=LSE_C):
    got = lse.double().to(ref["lse"].device)
    assert bool(torch.isfinite(got).all()), f"{what} lse: not finite"
    ratio = (got - ref["lse"]).abs() / lse_unit(ref, D)
    worst = float(ratio.max())
    assert worst <= c, f"{what} lse: worst |lse - ref| / unit = {worst:.3f} (limit {c})"
    return worst


def check_backward(dq, dk, dv, ref, what="", cq=DQ_C, ck=DK_C, cv=DV_C):
    return (kc.bf16_elementwise(dq, ref["dq"], cq * 2.0 ** -9 * ref["mag_dq"], what=f"{what} dq"),
            kc.bf16_elementwise(dk, ref["dk"], ck * 2.0 ** -9 * ref["mag_dk"], what=f"{what} dk"),
            kc.bf16_elementwise(dv, ref["dv"], cv * 2.0 ** -9 * ref["mag_dv"], what=f"{what} dv"))


def excess_ratio(y, ref64, mag64):
    """Worst ``(|y - ref| - ulp_bf16) / (2^-9 mag)``: the constant a result needs in front of ``2^-9 mag``."""
    yd, ref = y.double(), ref64.double()
    rms = ref.square().mean().sqrt()
    ulp = kc.bf16_ulp(torch.maximum(torch.maximum(yd.abs(), ref.abs()), rms / 256))
    return float((((yd - ref).abs() - ulp).clamp_min(0.0) / (2.0 ** -9 * mag64)).max())


def _bf(t):
    return t.bfloat16().float()


def emulate(q, k, v, go, scale=None, rounded_sum=False):
    """The kernels' arithmetic in fp32 torch ops on the CPU (bf16 operands ``[..., N, D]``): o, lse, dq, dk, dv as the kernels
    store them (bf16, lse fp32).  ``rounded_sum``: the row sum runs over the bf16-rounded weights."""
    q, k, v, go = q.float(), k.float(), v.float(), go.float()
    scale = 1.0 / math.sqrt(q.shape[-1]) if scale is None else scale
    s = (q @ k.transpose(-1, -2)) * scale
    m = s.amax(dim=-1, keepdim=True)
    e = torch.exp(s - m)
    row = (_bf(e) if rounded_sum else e).sum(-1, keepdim=True)
    o = ((_bf(e) @ v) / row).bfloat16()
    lse = m + torch.log(row)
    p = torch.exp(s - lse)
    delta = (go * o.float()).sum(-1, keepdim=True)
    ds = _bf(p * (go @ v.transpose(-1, -2) - delta))
    dv = (_bf(p).transpose(-1, -2) @ go).bfloat16()
    dq = (scale * (ds @ k)).bfloat16()
    dk = (scale * (ds.transpose(-1, -2) @ q)).bfloat16()
    return dict(o=o, lse=lse[..., 0], dq=dq, dk=dk, dv=dv)


def make_inputs(N, D, in_scale=1.0, seed=0, lead=(), Nk=None):
    """bf16 q, k (N(0, 1) times the input scale), v and dO (N(0, 1)) of shape ``lead + (N, D)`` on the CPU."""
    g = torch.Generator().manual_seed(seed * 1000003 + N * 131 + D)
    Nk = N if Nk is None else Nk
    q = (torch.randn(*lead, N, D, generator=g) * in_scale).bfloat16()
    k = (torch.randn(*lead, Nk, D, generator=g) * in_scale).bfloat16()
    v = torch.randn(*lead, Nk, D, generator=g).bfloat16()
    go = torch.randn(*lead, N, D, generator=g).bfloat16()
    return q, k, v, go


def check_refusal_texts(lib, prefix, max_head, unit):
    """Every refusal of the four entry points ``<prefix>_fwd / _bwd_delta / _bwd_dkv / _bwd_dq`` (``mk_attn`` with head sizes to
    128 and strides in units of 8, ``mk_attn_x3`` with 64 and 4): code 1 and the exact text of ``mk_last_error()``, before any
    launch -- no device is touched.  Returns the number of refusals checked."""
    import ctypes
    P = 4096
    good = [64 * 40, 40, 40 * 3] * 6

    def call(entry, D=32, N=5, first=P, strides=good, lse=P, delta=P):
        st = None if strides is None else (ctypes.c_longlong * len(strides))(*strides)
        sp = None if st is None else ctypes.addressof(st)
        fn = getattr(lib, f"{prefix}_{entry}")
        if entry == "fwd":
            rc = fn(first, P, P, P, lse, 1, 2, N, N, D, sp, 1.0, None)
        elif entry == "bwd_delta":
            rc = fn(first, P, delta, 1, 2, N, D, sp, None)
        elif entry == "bwd_dkv":
            rc = fn(first, P, P, P, lse, delta, P, P, 1, 2, N, N, D, sp, 1.0, None)
        else:
            rc = fn(first, P, P, P, lse, delta, P, 1, 2, N, N, D, sp, 1.0, None)
        return rc, lib.mk_last_error().decode()

    head = f"head size must be a multiple of 16 in 16 ... {max_head}"
    shared = [(dict(D=24), head), (dict(D=max_head + 16), head), (dict(N=0), "bad sizes"), (dict(first=None), "null pointer"),
              (dict(first=P + 8), "operand not 16-byte aligned"),
              (dict(strides=[64 * 40, 40, 40 * 3 + unit // 2] + good[3:]), f"strides must be non-negative multiples of {unit} elements"),
              (dict(strides=[64, 40, 16] + good[3:]), "token stride smaller than the head size"), (dict(strides=None), "null strides")]
    both = "lse / delta null or not 4-byte aligned"
    own = dict(fwd=[(dict(lse=P + 2), "lse not 4-byte aligned")],
               bwd_delta=[(dict(delta=None), "delta null or not 4-byte aligned"), (dict(delta=P + 2), "delta null or not 4-byte aligned")],
               bwd_dkv=[(dict(lse=None), both), (dict(delta=None), both), (dict(lse=P + 2), both), (dict(delta=P + 2), both)])
    own["bwd_dq"] = own["bwd_dkv"]
    n = 0
    for entry, cases in own.items():
        for kw, text in shared + cases:
            rc, msg = call(entry, **kw)
            assert (rc, msg) == (1, f"{prefix}_{entry}: {text}"), (entry, kw, rc, msg)
            n += 1
    return n
