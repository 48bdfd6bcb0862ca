"""Checks of the checker of the optimizer kernels (tests/optim_checks.py), without a GPU: an fp32 emulation of the arithmetic of
``AdamOp::one``, ``LambCoef::moments`` / ``update``, ``Lamb2Op::one`` (csrc/optim.hip) and ``adam1`` (csrc/adam.hip) in numpy float32
must meet the derived per-element bounds on every input set, and every mutation a kernel could plausibly suffer must miss them.

Each ``fmaf`` is a float64 product-sum rounded once to fp32.  The build uses hipcc's default ``-ffp-contract``, so every
``a - b c`` the source spells with separate operators is run in all the forms the compiler may choose: rounded product, fused, and
(AdamW: ``p decay - ss q``) fused on the other product.

Input sets: N(0, 1) state; gradients (and moments) 1e-3 and 1e-4 of the state; v at 1e-6 and at 1e4 of g^2; the L2 cancellation
set ``g ~ -wd p / coef``, where the gradient the moments see is the rounding residue of two terms a million times larger; steps
1, 3 and 1000; gradient multiplier 1 and 0.37.  Worst error / bound over all of them, 100 000 elements each (records of this
emulation, not limits): AdamW / Adam p 0.54, m 0.53, v 0.61; LAMB m 0.57, v 0.65, stage-2 p 0.51.
"""
import itertools

import numpy as np
import pytest

import optim_checks as oc

F = np.float32
N = 100_000
HYPER = dict(lr=oc.f32(1e-2), beta1=oc.f32(0.9), beta2=oc.f32(0.95), eps=oc.f32(1e-8), wd=oc.f32(0.1))
SETS = {"normal": (1.0, 1.0, False), "g1e-3": (1e-3, 1.0, False), "g1e-4": (1e-4, 1.0, False), "v1e-6": (1.0, 1e-6, False),
        "v1e4": (1.0, 1e4, False), "l2-cancel": (1.0, 1e-6, True)}
STEPS = (1, 3, 1000)
COEFS = (1.0, oc.f32(0.37))


def fma(a, b, c):
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F)


def inputs(name, coef, seed=0, n=N, divide=False):
    """(p, g, m, v) of an input set; ``divide``: the gradient is divided by ``coef`` (LAMB) instead of multiplied."""
    gs, vs, cancel = SETS[name]
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(F)
    g = (rng.standard_normal(n) * gs).astype(F)
    if cancel:
        scale = np.float64(coef) if divide else 1.0 / np.float64(coef)
        g = (-np.float64(HYPER["wd"]) * p * scale * (1 + rng.standard_normal(n) * 1e-6)).astype(F)
    m = (rng.standard_normal(n) * gs).astype(F)
    v = ((rng.standard_normal(n) * gs) ** 2 * vs).astype(F)
    return p, g, m, v


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' arithmetic in fp32
# ---------------------------------------------------------------------------------------------------------------------
def adam_emul(p, g, m, v, *, lr, beta1, beta2, eps, wd, adamw, coef, step, variant=0, apply_coef=True):
    """``AdamOp::one`` with the scalars of ``adam_kernel``; returns (p', m', v')."""
    lr, b1, b2, eps, wd, gc = (F(x) for x in (lr, beta1, beta2, eps, wd, coef if apply_coef else 1.0))
    bc1, _, bc2s = (F(x) for x in oc.bias_corrections(float(b1), float(b2), step))
    decay = F(1) - lr * wd if adamw else F(1)
    l2 = F(0) if adamw else wd
    ss = lr / bc1
    gg = fma(l2, p, g * gc)
    pp = p * decay
    mm = fma(b1, m, (F(1) - b1) * gg)
    vv = fma(b2, v, (F(1) - b2) * gg * gg)
    q = mm / (np.sqrt(vv) / bc2s + eps)
    if variant == 0:
        out = pp - ss * q
    elif variant == 1:
        out = fma(-ss, q, pp)
    else:
        out = fma(p, decay, -(ss * q))
    assert out.dtype == mm.dtype == vv.dtype == F
    return out, mm, vv


def adam1_emul(p, g, m, v, *, lr, beta1, beta2, eps, wd, step, variant=0):
    """``adam1`` of csrc/adam.hip with the scalars of ``mk_adam_step``."""
    lr, b1, b2, eps, wd = (F(x) for x in (lr, beta1, beta2, eps, wd))
    bc1, _, bc2s = (F(x) for x in oc.bias_corrections(float(b1), float(b2), step))
    gg = fma(wd, p, g)
    mm = fma(b1, m, (F(1) - b1) * gg)
    vv = fma(b2, v, (F(1) - b2) * gg * gg)
    q = mm / (np.sqrt(vv) / bc2s + eps)
    return (p - (lr / bc1) * q if variant == 0 else fma(-(lr / bc1), q, p)), mm, vv


def lamb_update_emul(m, v, p, k):
    u = (m / F(k["bc1"])) / (np.sqrt(v / F(k["bc2"])) + F(k["eps"]))
    return fma(F(k["wd"]), p, u) if k["adamw"] else u


def lamb1_emul(p, g, m, v, k):
    """``LambCoef::moments``: (m', v', u) and the fp64 sums of squares of p and u."""
    gg = g / F(k["div"])
    if not k["adamw"]:
        gg = fma(F(k["wd"]), p, gg)
    mm = fma(F(k["b1"]), m, F(k["b3"]) * gg)
    vv = fma(F(k["b2"]), v, (F(1) - F(k["b2"])) * gg * gg)
    u = lamb_update_emul(mm, vv, p, k)
    assert u.dtype == F
    return mm, vv, u, float((np.float64(p) ** 2).sum()), float((np.float64(u) ** 2).sum())


def lamb2_emul(p, mm, vv, k, sp, su, *, lr, trust, variant=0, u_from=None):
    """``lamb2_kernel`` / ``Lamb2Op::one``; ``u_from``: the parameter the update is formed from (the mutation)."""
    pn, un = F(np.sqrt(sp)), F(np.sqrt(su))
    ratio = F(lr) * (pn / un) if (trust and pn != 0 and un != 0) else F(lr)
    u = lamb_update_emul(mm, vv, p if u_from is None else u_from, k)
    return (p - ratio * u) if variant == 0 else fma(-ratio, u, p)


def lamb_k(adamw, div, step, bias_correction=1):
    return oc.lamb_scalars(beta1=HYPER["beta1"], beta2=HYPER["beta2"], beta3=oc.f32(1.0 - HYPER["beta1"]), eps=oc.f32(1e-6),
                           wd=HYPER["wd"], adamw=adamw, bias_correction=bias_correction, div=div, step=step)


# ---------------------------------------------------------------------------------------------------------------------
# the emulation meets the bounds
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adamw", [1, 0])
@pytest.mark.parametrize("name", list(SETS))
def test_adam_emulation_meets_the_bounds(name, adamw):
    worst = dict(p=0.0, m=0.0, v=0.0)
    for step, coef in itertools.product(STEPS, COEFS):
        p, g, m, v = inputs(name, coef)
        ref = oc.adam_ref(p, g, m, v, adamw=adamw, coef=coef, step=step, **HYPER)
        for variant in (0, 1, 2) if adamw else (0, 1):
            pp, mm, vv = adam_emul(p, g, m, v, adamw=adamw, coef=coef, step=step, variant=variant, **HYPER)
            what = f"{name} adamw={adamw} step={step} coef={coef} variant={variant}"
            for key, got in (("p", pp), ("m", mm), ("v", vv)):
                worst[key] = max(worst[key], oc.worst_ratio(got, ref[key], ref["e_" + key], f"{what}: {key}"))
    print(f"adam {name} adamw={adamw}: worst error / bound p {worst['p']:.2f} m {worst['m']:.2f} v {worst['v']:.2f}")
    assert max(worst.values()) > 0.05, "the bounds are far from the arithmetic: a bound this loose checks nothing"


@pytest.mark.parametrize("name", list(SETS))
def test_adam_step_emulation_meets_the_bounds(name):
    """``mk_adam_step`` is the L2 mode without a multiplier."""
    for step in STEPS:
        p, g, m, v = inputs(name, 1.0)
        ref = oc.adam_ref(p, g, m, v, adamw=0, coef=1.0, step=step, **HYPER)
        for variant in (0, 1):
            got = adam1_emul(p, g, m, v, step=step, variant=variant, **HYPER)
            for key, x in zip("pmv", got):
                oc.worst_ratio(x, ref[key], ref["e_" + key], f"{name} step={step} variant={variant}: {key}")


@pytest.mark.parametrize("adamw", [1, 0])
@pytest.mark.parametrize("name", list(SETS))
def test_lamb_emulation_meets_the_bounds(name, adamw):
    worst = dict(p=0.0, m=0.0, v=0.0, su=0.0)
    for step, div, trust, bc in itertools.product(STEPS, COEFS, (1, 0), (1, 0)):
        if not bc and step != 3:
            continue
        p, g, m, v = inputs(name, div, divide=True)
        k = lamb_k(adamw, div, step, bc)
        mm, vv, u, sp, su = lamb1_emul(p, g, m, v, k)
        r1 = oc.lamb1_ref(p, g, m, v, k)
        what = f"{name} adamw={adamw} step={step} div={div} trust={trust} bc={bc}"
        worst["m"] = max(worst["m"], oc.worst_ratio(mm, r1["m"], r1["e_m"], what + ": m"))
        worst["v"] = max(worst["v"], oc.worst_ratio(vv, r1["v"], r1["e_v"], what + ": v"))
        oc.worst_ratio(u, r1["u"], r1["e_u"], what + ": u")
        oc.scalar_ratio(sp, r1["sp"], r1["e_sp"], what + ": sum p^2")
        worst["su"] = max(worst["su"], oc.scalar_ratio(su, r1["su"], r1["e_su"], what + ": sum u^2"))
        r2 = oc.lamb2_ref(p, mm, vv, k, lr=HYPER["lr"], trust=trust)
        for variant in (0, 1):
            pp = lamb2_emul(p, mm, vv, k, sp, su, lr=HYPER["lr"], trust=trust, variant=variant)
            worst["p"] = max(worst["p"], oc.worst_ratio(pp, r2["p"], r2["e_p"], what + f" variant={variant}: p"))
    print(f"lamb {name} adamw={adamw}: worst error / bound p {worst['p']:.2f} m {worst['m']:.2f} v {worst['v']:.2f} "
          f"sum u^2 {worst['su']:.2f}")
    assert max(worst["p"], worst["m"], worst["v"]) > 0.05


# ---------------------------------------------------------------------------------------------------------------------
# mutations miss them
# ---------------------------------------------------------------------------------------------------------------------
def _chosen(upd):
    """An element whose |upd| is at least the set's median (one with m' ~ 0 could hide a skipped update legitimately)."""
    a = np.abs(upd)
    return int(np.argmin(np.where(a >= np.median(a), a, np.inf)))      # the smallest such: the hardest to see


@pytest.mark.parametrize("adamw", [1, 0])
@pytest.mark.parametrize("coef", COEFS)
@pytest.mark.parametrize("name", list(SETS))
def test_adam_mutations_exceed_the_bound(name, coef, adamw):
    p, g, m, v = inputs(name, coef, n=20_000)
    kw = dict(adamw=adamw, coef=coef, **HYPER)
    for step in STEPS:
        ref = oc.adam_ref(p, g, m, v, step=step, **kw)
        pp, mm, vv = adam_emul(p, g, m, v, step=step, **kw)
        i = _chosen(ref["upd"])
        skipped = pp.copy()
        skipped[i] = p[i]
        assert oc.exceeds(skipped, ref["p"], ref["e_p"]) > 1.0, f"step {step}: a skipped update stays inside the bound"
        twice = pp.copy()
        twice[i] = adam_emul(pp[i:i + 1], g[i:i + 1], mm[i:i + 1], vv[i:i + 1], step=step, **kw)[0][0]
        assert oc.exceeds(twice, ref["p"], ref["e_p"]) > 1.0, f"step {step}: an element updated twice stays inside the bound"
        for key, old, new in (("m", m, mm), ("v", v, vv)):
            skipped = new.copy()
            skipped[i] = old[i]
            assert oc.exceeds(skipped, ref[key], ref["e_" + key]) > 1.0, f"step {step}: a skipped {key} stays inside the bound"
        if coef != 1.0:
            plain = adam_emul(p, g, m, v, step=step, apply_coef=False, **kw)
            for key, x in zip("pmv", plain):
                assert oc.exceeds(x, ref[key], ref["e_" + key]) > 1.0, f"step {step}: {key} without the gradient multiplier"
    for mine, other in ((1, 2), (2, 1)):
        ref = oc.adam_ref(p, g, m, v, step=mine, **kw)
        pp = adam_emul(p, g, m, v, step=other, **kw)[0]
        assert oc.exceeds(pp, ref["p"], ref["e_p"]) > 1.0, f"step {other} for {mine} stays inside the bound"
        # ... and on the element where it shows least
        assert np.median(np.abs(np.float64(pp) - ref["p"]) / ref["e_p"]) > 1.0


@pytest.mark.parametrize("adamw", [1, 0])
@pytest.mark.parametrize("div", COEFS)
@pytest.mark.parametrize("name", list(SETS))
def test_lamb_mutations_exceed_the_bound(name, div, adamw):
    lr = HYPER["lr"]
    p, g, m, v = inputs(name, div, n=20_000, divide=True)
    for step in STEPS:
        k = lamb_k(adamw, div, step)
        mm, vv, u, sp, su = lamb1_emul(p, g, m, v, k)
        r1 = oc.lamb1_ref(p, g, m, v, k)
        r2 = oc.lamb2_ref(p, mm, vv, k, lr=lr, trust=1)
        pp = lamb2_emul(p, mm, vv, k, sp, su, lr=lr, trust=1)
        i = _chosen(r2["ratio"] * r1["u"])
        skipped = pp.copy()
        skipped[i] = p[i]
        assert oc.exceeds(skipped, r2["p"], r2["e_p"]) > 1.0, f"step {step}: a skipped update stays inside the bound"
        twice = pp.copy()
        twice[i] = lamb2_emul(pp[i:i + 1], mm[i:i + 1], vv[i:i + 1], k, sp, su, lr=lr, trust=1)[0]
        assert oc.exceeds(twice, r2["p"], r2["e_p"]) > 1.0, f"step {step}: an element updated twice stays inside the bound"
        # the neighbour tensor (the same state, parameters three times as large) and its trust ratio
        p3 = (F(3) * p).astype(F)
        _, _, _, sp3, su3 = lamb1_emul(p3, g, m, v, k)
        assert oc.exceeds(lamb2_emul(p, mm, vv, k, sp3, su3, lr=lr, trust=1), r2["p"], r2["e_p"]) > 1.0, \
            f"step {step}: the neighbour's ratio stays inside the bound"
        # the sums of another tensor show in tsum too
        assert abs(su3 - r1["su"]) > r1["e_su"] or abs(sp3 - r1["sp"]) > r1["e_sp"]
        if div != 1.0:
            kp = dict(k, div=1.0)
            plain = lamb1_emul(p, g, m, v, kp)
            assert oc.exceeds(plain[0], r1["m"], r1["e_m"]) > 1.0 and oc.exceeds(plain[1], r1["v"], r1["e_v"]) > 1.0, \
                f"step {step}: moments without the gradient divisor stay inside the bound"
        if adamw:
            new = lamb2_emul(p, mm, vv, k, sp, su, lr=lr, trust=1, u_from=pp)
            assert oc.exceeds(new, r2["p"], r2["e_p"]) > 1.0, f"step {step}: u from the new parameter stays inside the bound"
            u_new = lamb_update_emul(mm, vv, pp, k)
            assert abs(float((np.float64(u_new) ** 2).sum()) - r1["su"]) > r1["e_su"], \
                f"step {step}: sum u^2 from the new parameter stays inside the bound"
    k1, k2 = lamb_k(adamw, div, 1), lamb_k(adamw, div, 2)
    mm, vv, u, sp, su = lamb1_emul(p, g, m, v, k1)
    r2 = oc.lamb2_ref(p, mm, vv, k1, lr=lr, trust=0)
    assert oc.exceeds(lamb2_emul(p, mm, vv, k2, sp, su, lr=lr, trust=0), r2["p"], r2["e_p"]) > 1.0, \
        "step 2 for step 1 stays inside the bound"


# ---------------------------------------------------------------------------------------------------------------------
# norm, coefficients, the checks themselves
# ---------------------------------------------------------------------------------------------------------------------
def test_clip_reference_and_bounds():
    rng = np.random.default_rng(3)
    xs = [(rng.standard_normal(n) * s).astype(F) for n, s in ((5, 1.0), (40, 3.0), (1000, 0.1))]
    sums = [oc.exact_sumsq(x) for x in xs]
    ts, es = [s for s, _ in sums], [e for _, e in sums]
    kernel_ts = [float((np.float64(x) ** 2).sum()) for x in xs]             # any fp64 order
    for got, (s, e) in zip(kernel_ts, sums):
        oc.scalar_ratio(got, s, e, "tsum")
    G64 = np.sqrt(np.sum(kernel_ts))
    G = F(G64)
    for mode, max_norm in ((1, 50.0), (1, 2.0), (2, 50.0), (2, 2.0), (3, 2.0)):
        Gr, eG, c, ec = oc.clip_ref(ts, es, max_norm, mode)
        oc.scalar_ratio(G, Gr, eG, "G")
        assert eG < 2 * oc.U * Gr
        if mode == 1:
            got = F(max_norm) / (G + F(1e-6))
            oc.scalar_ratio(got if got < 1 else F(1), c, ec, "torch coefficient")
        elif mode == 2:
            oc.scalar_ratio(G / F(max_norm) if G > F(max_norm) else F(1), c, ec, "apex divisor")
        else:
            assert c is None
    # a tensor left out of the total lies outside
    Gr, eG, _, _ = oc.clip_ref(ts, es, 2.0, 3)
    assert abs(np.sqrt(np.sum(kernel_ts[:2])) - Gr) > eG


def test_worst_ratio_reports_and_zero_bounds():
    ref, b = np.array([1.0, 0.0, 2.0]), np.array([1e-7, 0.0, 1e-7])
    assert oc.worst_ratio(np.array([1.0, 0.0, 2.0], dtype=F), ref, b) == 0.0
    with pytest.raises(AssertionError, match="flat index 1"):
        oc.worst_ratio(np.array([1.0, 1e-30, 2.0]), ref, b, "zero bound")
    with pytest.raises(AssertionError, match="NaN"):
        oc.worst_ratio(np.array([1.0, np.nan, 2.0]), ref, b)
    with pytest.raises(AssertionError, match="flat index 2"):
        oc.worst_ratio(np.array([1.0, 0.0, 2.000001]), ref, b)
    import torch
    assert oc.worst_ratio(torch.tensor([1.0, 0.0, 2.0]), torch.tensor(ref), torch.tensor(b)) == 0.0
    with pytest.raises(AssertionError, match="flat index 2"):
        oc.worst_ratio(torch.tensor([1.0, 0.0, 2.001]), torch.tensor(ref), torch.tensor(b))


def test_references_agree_between_numpy_and_torch():
    import torch
    p, g, m, v = inputs("normal", 0.37, n=1000)
    a = oc.adam_ref(p, g, m, v, adamw=0, coef=oc.f32(0.37), step=3, **HYPER)
    b = oc.adam_ref(*(torch.from_numpy(x) for x in (p, g, m, v)), adamw=0, coef=oc.f32(0.37), step=3, **HYPER)
    for key in ("p", "m", "v", "e_p", "e_m", "e_v"):
        np.testing.assert_allclose(b[key].numpy(), a[key], rtol=1e-13, atol=0)
    k = lamb_k(1, oc.f32(0.37), 3)
    a, b = oc.lamb1_ref(p, g, m, v, k), oc.lamb1_ref(*(torch.from_numpy(x) for x in (p, g, m, v)), k)
    np.testing.assert_allclose(b["e_m"].numpy(), a["e_m"], rtol=1e-13)
    assert abs(a["su"] - b["su"]) < 1e-12 * a["su"]


def test_build_list_on_the_host():
    """The builder on CPU tensors: offsets, bands, the read-only comparison, and that a stray store is seen."""
    import torch
    data = [(np.arange(1, 6, dtype=F), np.ones(5, dtype=F)), (np.arange(3, dtype=F) + 7, np.ones(3, dtype=F))]
    L = oc.build_list(torch.device("cpu"), data, [(1, 3), (0, 2)], (False, True))
    assert L.T == 2 and L.D == 2 and list(L.n) == [5, 3]
    assert [p % 16 for p in L.ptrs] == [4, 12, 0, 8]
    assert np.array_equal(L.host(0, 0), data[0][0]) and np.array_equal(L.host(1, 1), data[1][1])
    L.check("untouched")
    L.view(0, 0)[2] = 5.0                                   # inside: allowed
    L.check("inside")
    base = L.view(0, 0)
    torch.as_strided(base, (1,), (1,), base.storage_offset() - 1)[0] = 1.0
    with pytest.raises(AssertionError, match="in front of the offset view"):
        L.check("lead")
    L = oc.build_list(torch.device("cpu"), data, (1, 3), (False, True))
    base = L.view(1, 0)
    torch.as_strided(base, (1,), (1,), base.storage_offset() + 3)[0] = 1.0
    with pytest.raises(AssertionError, match="guard band"):
        L.check("band")
    L = oc.build_list(torch.device("cpu"), data, (1, 3), (False, True))
    L.view(0, 1)[4] = 2.0
    with pytest.raises(AssertionError, match="read-only"):
        L.check("gradient")
    # a read in front of an offset read-only view meets a NaN
    base = L.view(1, 1)
    assert bool(torch.isnan(torch.as_strided(base, (1,), (1,), base.storage_offset() - 1)).all())
