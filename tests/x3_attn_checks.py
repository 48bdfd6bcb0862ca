"""Reference, units and bounds for the fp32 attention kernels on the bf16x3 arithmetic (csrc/x3_attn.hip); a plain module like
attn_checks.py and kernel_checks.py.

Reference: ``attn_checks.reference`` on the fp32 operands: float64 softmax attention, its gradients and its magnitudes
``mag_o``, ``mag_dv``, ``mag_dq``, ``mag_dk``, ``smag``.

Bounds, every element, ``C`` times a unit:

    o      2^-23 mag_o  (1 + smag_i)         the first term is the second product (an fp32-accurate contraction is off by a small
                                             multiple of 2^-23 |A| @ |B|, kernel_checks.x3_elementwise); the second covers the score
                                             error and the rounding of the exponent's argument: a score off by e changes a softmax
                                             weight by at most e relative, in numerator and denominator, and an fp32-accurate score
                                             is off by a small multiple of 2^-23 smag_i
    dq     2^-23 mag_dq (1 + smag_i)         the same form, the query's own row
    dk, dv 2^-23 mag_dk (1 + max_i smag_i)   a key's gradient sums over all queries: every term carries the relative error of its
                                             query's row, which the worst row bounds
    lse    2^-23 (smag_i + |lse_i| + 1)

``attn_checks.score_slack`` is NOT used: its worst-case factor 2 (D + 4) is wider than what one missing 2^-16-weight piece
product costs.

The constants are NOT taken from the kernels.  ``emulate`` is the kernels' arithmetic in fp32 torch ops on the CPU: the
``kernel_checks.x3_split`` pieces of every operand of the two forward and the five backward products, the six piece products in
the engine's order per 16-k sub-step with fp32 accumulation (the two products contracted over the head axis, S and dP, run
piece-major over the whole axis as the kernels' ``head_product`` does: a dominant term meets fewer roundings), the online
softmax over key tiles of 64 in the log2 domain, ``P`` and ``dS`` split before their second products, delta from the stored
fp32 ``O``.  Over ``EMU_SHAPES`` (those of attn_checks plus one at
D = 16; q and k carry the input scale), ``EMU_SEEDS`` draws each, its worst ratios of ``|x - ref|`` to the unit are the
``EMU_WORST_*`` figures below; each constant is twice that figure, rounded up, the factor 2 for the accumulation order and the
hardware exp2 (the rule of ``attn_checks`` and ``X3_C``).  tests/test_x3_attn_cpu.py asserts that the emulation stays within HALF
of each constant, and that each planted defect (``emulate(drop=...)``: one of the three 2^-16-weight piece products of one of
the seven matrix products left out; ``drop_key``: one key missing from one row) exceeds its bound at ``DEFECT_SHAPES``, which
are shapes of the GPU test (tests/test_x3_attn_gpu.py): q, k of scale 1 and at most 259 keys, because the ratio of a dropped
piece falls as 1 / sqrt(K) and with a nearly flat softmax (input scale 0.3) a dropped score piece reaches only about 2 units.
"""
import math

import torch

import attn_checks as ac
import kernel_checks as kc

EMU_SHAPES = ac.EMU_SHAPES + [(259, 16, 1.0)]
EMU_SEEDS = 3
# worst ratios of the emulation over EMU_SHAPES (measured on the CPU, see the module docstring)
EMU_WORST_O = 0.53               # at (200, 48, 3.0)
EMU_WORST_LSE = 0.74             # at (200, 48, 3.0)
EMU_WORST_DV = 0.75              # at (129, 64, 0.3)
EMU_WORST_DQ = 0.24              # at (129, 64, 0.3)
EMU_WORST_DK = 0.19              # at (259, 16, 1.0)
O_C = 2.0
LSE_C = 2.0
DV_C = 2.0
DQ_C = 1.0
DK_C = 1.0

PRODUCTS = ("s", "pv", "bs", "dp", "dv", "dq", "dk")      # S = q k^T and O = P v;  S again, dP = dO v^T, dV, dQ, dK
DROPS = (0, 1, 2)                                         # the 2^-16-weight products in the engine's order: al bh, ah bl, am bm
DEFECT_SHAPES = [(129, 48), (259, 64), (65, 16)]          # (N, D) with Nq = Nk = N, input scale 1

_PA, _PB = (2, 0, 1, 1, 0, 0), (0, 2, 1, 0, 1, 0)
_LOG2E, _LN2 = 1.4426950408889634, 0.6931471805599453
_TK = 64


def make_inputs(N, D, in_scale=1.0, seed=0, lead=(), Nk=None):
    """fp32 q, k (N(0, 1) times the input scale), v and dO (N(0, 1)) of shape ``lead + (N, D)`` on the CPU."""
    g = torch.Generator().manual_seed(seed * 1000003 + N * 131 + D)
    Nk = N if Nk is None else Nk
    q = torch.randn(*lead, N, D, generator=g) * in_scale
    k = torch.randn(*lead, Nk, D, generator=g) * in_scale
    v = torch.randn(*lead, Nk, D, generator=g)
    go = torch.randn(*lead, N, D, generator=g)
    return q, k, v, go


# ---------------------------------------------------------------------------------------------------------------------
# units and checks
# ---------------------------------------------------------------------------------------------------------------------
def units(ref):
    """The units of o, lse and, where the reference holds gradients, dq, dk, dv (float64, shaped like the results)."""
    smag = ref["smag"]
    row = (1.0 + smag)[..., None]
    u = dict(o=2.0 ** -23 * ref["mag_o"] * row, lse=2.0 ** -23 * (smag + ref["lse"].abs() + 1.0))
    if "dq" in ref:
        worst = (1.0 + smag.amax(dim=-1))[..., None, None]
        u.update(dq=2.0 ** -23 * ref["mag_dq"] * row, dk=2.0 ** -23 * ref["mag_dk"] * worst, dv=2.0 ** -23 * ref["mag_dv"] * worst)
    return u


CONSTANTS = dict(o=O_C, lse=LSE_C, dq=DQ_C, dk=DK_C, dv=DV_C)


def ratio(y, ref64, unit64):
    """Worst ``|y - ref| / unit`` (inf for a result that is not finite)."""
    yd = y.double().to(ref64.device)
    if not bool(torch.isfinite(yd).all()):
        return float("inf")
    return float(((yd - ref64).abs() / unit64).max())


def ratios(res, ref):
    """name -> worst ratio for every result of ``res`` (a dict as ``emulate`` returns it) that has a unit."""
    u = units(ref)
    return {n: ratio(res[n], ref[n], u[n]) for n in u if n in res}


def check(name, y, ref, what=""):
    """Asserts that every element of the result ``name`` (o, lse, dq, dk, dv) is finite and within its bound; returns the worst
    ratio to the unit."""
    u = units(ref)[name]
    return kc.x3_elementwise(y, ref[name], u * 2.0 ** 23, c=CONSTANTS[name], what=f"{what} {name}")


# ---------------------------------------------------------------------------------------------------------------------
# the emulation
# ---------------------------------------------------------------------------------------------------------------------
def x3_matmul(a, b, drop=None, piece_major=False):
    """``a [..., M, K] @ b [..., K, N]`` as the kernels evaluate it: both operands split into three bf16 pieces, the six piece
    products in the engine's order per 16-k sub-step, one fp32 addition per 16-k piece product.  ``piece_major``: the order of
    the products contracted over the head axis (``head_product`` of the kernels): the first of the six for every sub-step, then
    the second, ... so that the h h products come last.  ``drop``: that one of the six is left out."""
    A, Bp = kc.x3_split(a.float(), exact=False), kc.x3_split(b.float(), exact=False)
    steps = range(0, a.shape[-1], 16)
    order = [(t, k0) for t in range(6) for k0 in steps] if piece_major else [(t, k0) for k0 in steps for t in range(6)]
    acc = torch.zeros(*a.shape[:-1], b.shape[-1], dtype=torch.float32)
    for t, k0 in order:
        if t != drop:
            acc = acc + A[_PA[t]][..., k0:k0 + 16] @ Bp[_PB[t]][..., k0:k0 + 16, :]
    return acc


def emulate(q, k, v, go=None, scale=None, drop=None, drop_key=None):
    """The kernels' arithmetic in fp32 torch ops on the CPU (fp32 operands ``[..., N, D]``): o, lse and, with ``go``, dq, dk, dv.
    ``drop = (product, t)``: piece product ``t`` of that matrix product (``PRODUCTS``) is not issued.  ``drop_key = (i, j)``: the
    forward of query row i does not see key j."""
    q, k, v = q.float(), k.float(), v.float()
    D, Nq, Nk = q.shape[-1], q.shape[-2], k.shape[-2]
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    c = torch.tensor(scale, dtype=torch.float32) * torch.tensor(_LOG2E, dtype=torch.float32)

    def dropped(name):
        return drop[1] if (drop is not None and drop[0] == name) else None

    m = torch.full(q.shape[:-1], -math.inf, dtype=torch.float32)
    l = torch.zeros(q.shape[:-1], dtype=torch.float32)
    o = torch.zeros_like(q)
    for k0 in range(0, Nk, _TK):
        kt, vt = k[..., k0:k0 + _TK, :], v[..., k0:k0 + _TK, :]
        s = x3_matmul(q, kt.transpose(-1, -2), dropped("s"), True) * c
        if drop_key is not None and k0 <= drop_key[1] < k0 + _TK:
            s[..., drop_key[0], drop_key[1] - k0] = -math.inf
        mn = torch.maximum(m, s.amax(dim=-1))
        alpha = torch.exp2(m - mn)
        e = torch.exp2(s - mn[..., None])
        l = l * alpha + e.sum(-1)
        o = o * alpha[..., None] + x3_matmul(e, vt, dropped("pv"))
        m = mn
    o = o * (1.0 / l)[..., None]
    lse = (m + torch.log2(l)) * torch.tensor(_LN2, dtype=torch.float32)
    res = dict(o=o, lse=lse)
    if go is None:
        return res
    go = go.float()
    lse2 = (lse * torch.tensor(_LOG2E, dtype=torch.float32))[..., None]
    p = torch.exp2(x3_matmul(q, k.transpose(-1, -2), dropped("bs"), True) * c - lse2)
    delta = (go * o).sum(-1, keepdim=True)
    ds = p * (x3_matmul(go, v.transpose(-1, -2), dropped("dp"), True) - delta)
    sc = torch.tensor(scale, dtype=torch.float32)
    res.update(dv=x3_matmul(p.transpose(-1, -2), go, dropped("dv")),
               dq=x3_matmul(ds, k, dropped("dq")) * sc,
               dk=x3_matmul(ds.transpose(-1, -2), q, dropped("dk")) * sc)
    return res
