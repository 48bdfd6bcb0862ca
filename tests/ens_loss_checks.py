"""What the tests of the ensemble CRPS loss share (a plain module, imported by tests/test_ens_loss_cpu.py,
tests/test_ens_loss_dist_cpu.py and tests/test_ens_loss_gpu.py): inputs with ties, a temperature-like channel and NaN points,
and a numpy float64 restatement of the gradient that shares no step with a sort or with autograd.

The forward reference is ``ens_checks.sums`` (``a`` and ``g`` from ALL PAIRS).  The gradient of
``sum_bc gs[b, c, 0] S0[b, c] + gs[b, c, 1] S1[b, c]`` with respect to member e of a point is

    w_h (gs0 sgn(x_e - y) / E + gs1 2 (L_e - G_e) / E^2),      L_e = #{f : x_f < x_e},  G_e = #{f : x_f > x_e}

with the counts formed here by COMPARISON, member by member, as integers, and multiplied out in float64.  If the target or a
member of a point is NaN, every member of that point has a NaN gradient.

Bounds (derived, not tuned):

* a float64 evaluation (the torch formulation on float64 members): the reference and the value are each a handful of float64
  operations on terms of magnitude at most ``|w| (|gs0| / E + 2 |gs1| (E - 1) / E^2)``; ``float64_bound`` allows
  ``16 2^-53 |w| (|gs0| / E + 2 |gs1| / E)`` per element;
* a kernel that forms the value in float64 and rounds it ONCE to the gradient's dtype: ``(u + 2^-40) |r|`` per element with
  ``u = 2^-24`` for fp32 and ``2^-8`` for bf16 (``rounded_bound``), and exactly zero where the reference is zero."""
import functools

import numpy as np

import ens_checks as ec

U = 2.0 ** -53
ROUND = {"float32": 2.0 ** -24, "bfloat16": 2.0 ** -8}


@functools.lru_cache(maxsize=None)
def problem(shape, dtype="float32", kind="normal", seed=0):
    """``(ens [B, E, C, H, W], tar [B, C, H, W], wrow [H], gs [B, C, 2] float64)``, members rounded to ``dtype``.  ``kind``:
    ``"normal"`` is ``ens_checks.problem`` (channel 0 temperature-like: offset 250, spread 1); ``"ties"`` has integer members and
    targets in -2 ... 2; ``"nan"`` is ``"normal"`` with a NaN member and a NaN target at known points (``NAN_POINTS``).  ``gs`` is
    random with a zero and a negative entry.  Shared between tests: do not write to the arrays."""
    B, E, C, H, W = shape
    rng = np.random.default_rng(seed + 77 * E + sum(shape))
    if kind == "ties":
        ens = rng.integers(-2, 3, size=shape).astype(np.float32)
        tar = rng.integers(-2, 3, size=(B, C, H, W)).astype(np.float32)
        wrow = ec.rounded(rng.uniform(0.1, 1.0, size=H) / (H * W), "float32")
    else:
        ens, tar, wrow = (np.array(a) for a in ec.problem(shape, dtype, seed))
        if kind == "nan":
            for (b, c, h, w), where in nan_points(shape):
                if where == "member":
                    ens[b, E - 1, c, h, w] = np.nan
                else:
                    tar[b, c, h, w] = np.nan
    gs = rng.standard_normal((B, C, 2))
    gs.reshape(-1)[0] = 0.0
    gs.reshape(-1)[1] = -abs(gs.reshape(-1)[1]) - 0.5
    for a in (ens, tar, wrow, gs):
        a.setflags(write=False)
    return ens, tar, wrow, gs


def nan_points(shape):
    """The NaN points of ``problem(..., kind="nan")``: ``((b, c, h, w), "member" | "target")``, the last point of the first
    field (a member) and the first point of the last field (the target)."""
    B, E, C, H, W = shape
    return [((0, 0, H - 1, W - 1), "member"), ((B - 1, C - 1, 0, 0), "target")]


def counts(ens):
    """``(L, G)`` int64 ``[B, E, C, H, W]``: the members below and above each member, by comparison, member by member."""
    L, G = np.zeros(ens.shape, dtype=np.int64), np.zeros(ens.shape, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for f in range(ens.shape[1]):
            L += ens[:, f:f + 1] < ens
            G += ens[:, f:f + 1] > ens
    return L, G


def signs(ens, tar):
    """``sgn(x_e - y)`` int64, 0 for a tie."""
    with np.errstate(invalid="ignore"):
        return (ens > tar[:, None]).astype(np.int64) - (ens < tar[:, None]).astype(np.int64)


def _per_field(a):
    return np.asarray(a, dtype=np.float64)[:, None, :, None, None]           # [B, C] -> [B, 1, C, 1, 1]


def grad(ens, tar, wrow, gs):
    """The gradient ``[B, E, C, H, W]`` float64 by the closed form of the module docstring; NaN at every member of a NaN point."""
    E = ens.shape[1]
    L, G = counts(ens)
    w = wrow.astype(np.float64).reshape(1, 1, 1, -1, 1)
    r = w * (_per_field(gs[..., 0]) * signs(ens, tar) / E + _per_field(gs[..., 1]) * (2 * (L - G)) / (E * E))
    return np.where(ec.bad_points(ens, tar)[:, None], np.nan, r)


def float64_bound(ens, wrow, gs):
    E = ens.shape[1]
    w = np.abs(wrow.astype(np.float64)).reshape(1, 1, 1, -1, 1)
    return np.broadcast_to(16 * U * w * (_per_field(np.abs(gs[..., 0])) / E + 2 * _per_field(np.abs(gs[..., 1])) / E), ens.shape)


def assert_grad(got, ens, tar, wrow, gs, bound, what=""):
    """``got`` against ``grad``: NaN exactly at all members of the NaN points, exactly zero where the reference is, and
    ``|got - r| <= bound`` elsewhere (``bound``: an array, or a dtype name for the once-rounded bound).  Prints the worst
    error over the bound before it asserts."""
    got = np.asarray(got, dtype=np.float64)
    want = grad(ens, tar, wrow, gs)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN pattern", int(np.isnan(got).sum()), int(nan.sum()))
    lim = (ROUND[bound] + 2.0 ** -40) * np.abs(want) if isinstance(bound, str) else bound
    zero = (want == 0) & ~nan
    assert (got[zero] == 0).all(), (what, "not zero where sgn = 0 and L = G", int((got[zero] != 0).sum()))
    rest = ~nan & ~zero
    err = np.abs(got - want)[rest]
    worst = float((err / lim[rest]).max()) if err.size else 0.0
    print(f"{what}: worst gradient error / bound = {worst:.3e} over {err.size} elements, {int(zero.sum())} exact zeros, {int(nan.sum())} NaN")
    assert worst <= 1.0, (what, worst)
