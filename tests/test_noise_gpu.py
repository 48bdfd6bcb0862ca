"""GPU tests of csrc/noise.hip through the C ABI (guarded state, poisoned tables), of ``ops.noise_spectrum``, of
``noise.SphericalNoise`` on the 32 x 64 Legendre-Gauss grid (``lmax`` 32, ``mmax`` 33) and of the members that take its fields.
The coefficients are held per element and per component to the derived bound of tests/noise_checks.py against the numpy
restatement (which the CPU tests hold the torch formulation to first); shards, repeats and graph replays are compared bit for
bit.

Largest error / bound measured on an MI355X: 0.277 for the coefficients, 0.131 after AR(1) updates, 0.014 for ``sample``, and
0.137 of twice the bound between ``MK_NOISE=hip`` and ``torch``; every run prints its figures."""
import math

import numpy as np
import pytest
import torch

import kernel_checks as kc
import noise_checks as nc
from oracle import sht as osht

pytestmark = pytest.mark.gpu

NLAT, NLON, LMAX, MMAX = 32, 64, 32, 33
NAN_C = complex(float("nan"), float("nan"))
ids = lambda s: f"seed{nc.SEEDS.index(s)}"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from makani_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _sigmas(L, l_off=0):
    return (0.5 + 1.0 / (1.0 + np.arange(l_off, l_off + L))).astype(np.float32)


def _scale(BC):
    return np.linspace(0.25, 2.0, BC).astype(np.float32)


def launch(dev, L, M, BC, seed, t, l_off=0, m_off=0, row0=0, row_scale=None, phi=0.0, state=None, sigma=None):
    """One call of mk_noise_spectrum: the state between sentinel bands (or ``state``: a ``(view, check)`` pair to update), the
    tables between NaN bands.  Returns (numpy state, the pair)."""
    from makani_amd import _lib
    lib = _lib.load()
    view, check = kc.guarded((L, M, BC), torch.complex64, dev) if state is None else state
    sig = kc.poisoned(torch.from_numpy(_sigmas(L, l_off) if sigma is None else sigma), dev)
    rs = None if row_scale is None else kc.poisoned(torch.from_numpy(row_scale), dev)
    assert view.data_ptr() % 16 == 0
    rc = lib.mk_noise_spectrum(view.data_ptr(), sig.data_ptr(), None if rs is None else rs.data_ptr(), L, M, BC, l_off, m_off, row0,
                               seed - (1 << 64) if seed >= 1 << 63 else seed, t, None, phi, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "mk_noise_spectrum")
    torch.cuda.synchronize()
    check(f"state {L}x{M}x{BC}")
    return view.cpu().numpy(), (view, check)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# the kernel against the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", nc.SEEDS, ids=ids)
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("BC", [1, 5, 6, 66])
def test_coefficients_within_the_bound_and_the_shard_is_the_slice(dev, BC, scaled, seed):
    rs = _scale(BC) if scaled else None
    full, _ = launch(dev, LMAX, MMAX, BC, seed, 3, row_scale=rs)
    xi, bound, _ = nc.restate(_sigmas(LMAX), LMAX, MMAX, BC, seed, 3, row_scale=rs)
    ratio = nc.worst_ratio(full, xi, bound)
    L, M, l_off, m_off = 9, 11, 16, 22
    shard, _ = launch(dev, L, M, BC, seed, 3, l_off, m_off, row_scale=rs)
    sxi, sbound, _ = nc.restate(_sigmas(L, l_off), L, M, BC, seed, 3, l_off, m_off, row_scale=rs)
    sratio = nc.worst_ratio(shard, sxi, sbound)
    print(f"[noise gpu] BC={BC} scaled={scaled} seed={seed:#x}: worst error / bound {ratio:.3f} (full), {sratio:.3f} (shard)")
    assert ratio <= 1.0 and sratio <= 1.0
    assert (sbound == 0).any() and (full[:, 0].imag == 0).all()
    assert np.array_equal(_bits(shard), _bits(full[l_off:l_off + L, m_off:m_off + M]))


def test_rows_are_global(dev):
    full, _ = launch(dev, 9, 11, 10, nc.SEEDS[1], 1)
    part, _ = launch(dev, 9, 11, 5, nc.SEEDS[1], 1, row0=4)
    assert np.array_equal(_bits(part), _bits(full[:, :, 4:9]))


def test_a_fresh_draw_does_not_read_the_state(dev):
    for BC in (5, 6):
        pair = kc.guarded((LMAX, MMAX, BC), torch.complex64, dev, fill=NAN_C)
        assert bool(torch.isnan(torch.view_as_real(pair[0])).all())
        got, _ = launch(dev, LMAX, MMAX, BC, 0, 0, state=pair)
        assert np.isfinite(nc.components(got)).all()
        below = np.arange(LMAX)[:, None] < np.arange(MMAX)[None, :]
        assert (_bits(got[below]) == 0).all() and (got[~below] != 0).all()


@pytest.mark.parametrize("BC", [5, 6])
def test_ar1_updates_follow_the_restated_recursion(dev, BC):
    L, M, l_off, m_off, phi, seed = 9, 11, 4, 6, 0.5, nc.SEEDS[1]
    rs = _scale(BC)
    got, pair = launch(dev, L, M, BC, seed, 0, l_off, m_off, row_scale=rs)
    S, bS, _ = nc.restate(_sigmas(L, l_off), L, M, BC, seed, 0, l_off, m_off, row_scale=rs)
    for t in (1, 2):
        got, pair = launch(dev, L, M, BC, seed, t, l_off, m_off, row_scale=rs, phi=phi, state=pair)
        xi, bxi, _ = nc.restate(_sigmas(L, l_off), L, M, BC, seed, t, l_off, m_off, row_scale=rs)
        S, bS = nc.ar1(S, bS, xi, bxi, phi)
        bS = np.where(bxi == 0, 0.0, bS)
        ratio = nc.worst_ratio(got, S, bS)
        print(f"[noise gpu] AR(1) BC={BC} update {t}: worst error / bound {ratio:.3f}")
        assert ratio <= 1.0
    assert nc.worst_ratio(got, xi, bxi) > 1e3                 # not simply the latest draw


def test_two_runs_give_equal_bits(dev):
    for phi in (0.0, 0.5):
        runs = []
        for _ in range(2):
            got, pair = launch(dev, LMAX, MMAX, 66, nc.SEEDS[1], 0)
            if phi:
                got, pair = launch(dev, LMAX, MMAX, 66, nc.SEEDS[1], 1, phi=phi, state=pair)
            runs.append(got)
        assert np.array_equal(_bits(runs[0]), _bits(runs[1]))


def test_element_offsets_beyond_2_31_bytes(dev):
    """A 2.2 GB state (32 x 33 x 2^18): the last rows, whose byte offsets need more than 32 bits, and the first are the small
    draws of those rows, bit for bit."""
    from makani_amd import ops
    BC, seed = 2 ** 18, nc.SEEDS[1]
    sig = torch.from_numpy(_sigmas(LMAX)).to(dev)
    big = torch.empty((LMAX, MMAX, BC), dtype=torch.complex64, device=dev)
    assert big.numel() * 8 > 2 ** 31
    ops.noise_spectrum(big, sig, seed, t=2)
    for row0 in (0, BC - 6):
        small = torch.full((LMAX, MMAX, 6), NAN_C, dtype=torch.complex64, device=dev)
        ops.noise_spectrum(small, sig, seed, t=2, row0=row0)
        assert torch.equal(torch.view_as_real(big[:, :, row0:row0 + 6].contiguous()), torch.view_as_real(small))
    xi, bound, _ = nc.restate(_sigmas(LMAX), LMAX, MMAX, 6, seed, 2, row0=BC - 6)
    assert nc.worst_ratio(small.cpu().numpy(), xi, bound) <= 1.0
    del big


# ---------------------------------------------------------------------------------------------------------------------
# the op and the module
# ---------------------------------------------------------------------------------------------------------------------
def _module(dev, seed, phi=0.0, sigma=1.0, spectrum=None, row_scale=None):
    from makani_amd.noise import SphericalNoise, degree_sigmas
    from makani_amd.sht import InverseRealSHT
    isht = InverseRealSHT(NLAT, NLON, LMAX, MMAX, "legendre-gauss")
    sig = degree_sigmas(np.ones(LMAX) if spectrum is None else spectrum, sigma, MMAX)
    return SphericalNoise(isht, sig, seed=seed, phi=phi, row_scale=row_scale).to(dev), sig.astype(np.float32)


def _eager(dev, sig32, BC, seed, t):
    from makani_amd import ops
    st = torch.full((LMAX, MMAX, BC), NAN_C, dtype=torch.complex64, device=dev)
    return ops.noise_spectrum(st, torch.from_numpy(sig32).to(dev), seed, t=t)


def test_a_captured_call_draws_anew_on_every_replay(dev, monkeypatch):
    monkeypatch.setenv("MK_NOISE", "hip")
    seed, BC = nc.SEEDS[1], 6
    mod, sig32 = _module(dev, seed)
    first = mod.coefficients(BC).clone()                    # draw 0, also the warm-up
    assert torch.equal(torch.view_as_real(first), torch.view_as_real(_eager(dev, sig32, BC, seed, 0)))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = mod.coefficients(BC)
    states = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        states.append(out.clone())
    assert int(mod.draws) == 3
    for t, s in zip((1, 2), states):
        assert torch.equal(torch.view_as_real(s), torch.view_as_real(_eager(dev, sig32, BC, seed, t))), t
    assert not torch.equal(torch.view_as_real(states[0]), torch.view_as_real(states[1]))


def _synthesis_bound(c, noise_bound):
    """Per element of the synthesised field ``[rows, nlat, nlon]``: the bound of the inverse transform against the float64 oracle
    on the same coefficients, plus the coefficients' own bound carried through it.  With ``mag[r, k] = sum_m w_m sum_l |P_lm(k)|
    (|Re c| + |Im c|)`` (``w_0 = 1``, ``w_m = 2``: what the real inverse FFT adds up, every factor ``cos`` / ``sin`` at most 1):

    * the Legendre synthesis, per component ``c 2^-23 (|P| @ |c|)`` with the engine's ``c`` of tests/kernel_checks.py (``X3_C`` for
      the bf16x3 engine, ``F32_C`` for fp32 MFMA): ``2 c`` units of ``2^-24`` of ``mag``;
    * the fp32 rounding of the package's Legendre table against the oracle's float64 one: 1 unit;
    * the inverse FFT, ``log2(nlon)`` stages of one rounded twiddle (1), one complex product (2) and one sum (1): ``4 log2(nlon)``
      units;
    * the coefficient bound ``b`` through the same sums, ``sum_m w_m sum_l |P| sqrt 2 b`` (``|cos| + |sin| <= sqrt 2``)."""
    from makani_amd import ops
    P = np.abs(osht.InverseRealSHT(NLAT, NLON, LMAX, MMAX, "legendre-gauss", dtype=np.float64).pct)         # [m, l, k]
    w = np.full(MMAX, 2.0)
    w[0] = 1.0
    engine = kc.X3_C if ops.SPECTRAL_GEMM == "bf16x3" else kc.F32_C
    units = 2.0 * engine + 1.0 + 4.0 * math.log2(NLON)
    mag = np.einsum("m,mlk,lmr->rk", w, P, np.abs(c.real) + np.abs(c.imag))
    carried = np.einsum("m,mlk,lmr->rk", w, P, math.sqrt(2.0) * noise_bound)
    return (units * nc.U * mag + carried)[:, :, None]


@pytest.mark.parametrize("seed", nc.SEEDS, ids=ids)
def test_sample_is_the_oracle_inverse_of_the_restated_coefficients(dev, monkeypatch, seed):
    monkeypatch.setenv("MK_NOISE", "hip")
    rows = 7
    rs = _scale(rows)
    mod, sig32 = _module(dev, seed, sigma=0.7, spectrum=(2.0 * np.arange(LMAX) + 1.0) ** -1.0, row_scale=rs)
    x = mod.sample(rows)
    assert x.shape == (rows, NLAT, NLON) and x.dtype == torch.float32 and int(mod.draws) == 1
    xi, bound, _ = nc.restate(sig32, LMAX, MMAX, rows, seed, 0, row_scale=rs)
    want = osht.InverseRealSHT(NLAT, NLON, LMAX, MMAX, "legendre-gauss", dtype=np.float64)(np.moveaxis(xi, -1, 0))
    lim = _synthesis_bound(xi, bound)
    err = np.abs(x.cpu().numpy().astype(np.float64) - want)
    print(f"[noise gpu] sample seed={seed:#x}: worst error / bound {float((err / lim).max()):.3f}")
    assert (err <= lim).all() and float(np.abs(want).max()) > 0.1


@pytest.mark.parametrize("seed", nc.SEEDS, ids=ids)
def test_area_mean_variance_is_sigma_squared(dev, monkeypatch, seed):
    """White spectrum, 63 rows, t = 3: the mean over rows of the area-weighted variance within 5 standard errors of sigma^2,
    one standard error ``sqrt(2 / 1024) / sqrt(63)`` relative (1024 real degrees of freedom per field).  The restatement alone
    gives 1.0 and 0.6 standard errors for these inputs (tests/test_noise_cpu.py)."""
    from makani_amd import ops
    monkeypatch.setenv("MK_NOISE", "hip")
    rows, sigma = 63, 0.7
    mod, sig32 = _module(dev, seed, sigma=sigma)
    st = torch.empty((LMAX, MMAX, rows), dtype=torch.complex64, device=dev)
    ops.noise_spectrum(st, mod.sigma_l, seed, t=3)
    x = mod.inverse_transform.inverse_packed(st).cpu().numpy()
    _, w = osht.quadrature("legendre-gauss", NLAT)
    se = math.sqrt(2.0 / 1024.0) / math.sqrt(rows)
    off = (nc.area_variance(x, w).mean() / sigma ** 2 - 1.0) / se
    print(f"[noise gpu] variance seed={seed:#x}: ratio {1.0 + off * se:.4f}, {off:+.2f} standard errors")
    assert abs(off) <= 5.0


@pytest.mark.parametrize("BC", [5, 66])
def test_torch_formulation_on_the_device_agrees_with_hip(dev, monkeypatch, BC):
    from makani_amd import ops
    seed, rs = nc.SEEDS[1], _scale(BC)
    sig, rsd = torch.from_numpy(_sigmas(LMAX)).to(dev), torch.from_numpy(rs).to(dev)
    xi, bound, _ = nc.restate(_sigmas(LMAX), LMAX, MMAX, BC, seed, 3, row_scale=rs)
    out = {}
    for mode in ("hip", "torch"):
        monkeypatch.setenv("MK_NOISE", mode)
        st = torch.full((LMAX, MMAX, BC), NAN_C, dtype=torch.complex64, device=dev)
        fresh = ops.noise_spectrum(st, sig, seed, t=1, t_dev=torch.tensor([2], dtype=torch.int32, device=dev), row_scale=rsd).clone()
        assert nc.worst_ratio(fresh.cpu().numpy(), xi, bound) <= 1.0
        out[mode] = (fresh, ops.noise_spectrum(st, sig, seed, t=4, phi=0.5, row_scale=rsd).clone())
    ratio = nc.worst_ratio(out["hip"][0].cpu().numpy(), out["torch"][0].cpu().numpy(), bound, factor=2.0)
    x4, b4, _ = nc.restate(_sigmas(LMAX), LMAX, MMAX, BC, seed, 4, row_scale=rs)
    _, bar = nc.ar1(xi, bound, x4, b4, 0.5)
    ar = nc.worst_ratio(out["hip"][1].cpu().numpy(), out["torch"][1].cpu().numpy(), np.where(bound == 0, 0.0, bar), factor=2.0)
    print(f"[noise gpu] hip against torch BC={BC}: worst difference / (2 bound) {ratio:.3f}, after an AR(1) step {ar:.3f}")
    assert ratio <= 1.0 and ar <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# the members
# ---------------------------------------------------------------------------------------------------------------------
def test_perturb_members_adds_the_documented_rows(dev, monkeypatch):
    from makani_amd.ensemble import perturb_members
    monkeypatch.setenv("MK_NOISE", "hip")
    B, E, C, std, seed = 2, 3, 3, 0.25, nc.SEEDS[1]
    x = torch.randn(B, C, NLAT, NLON, generator=torch.Generator().manual_seed(3)).to(dev)
    mod, _ = _module(dev, seed)
    twin, _ = _module(dev, seed)
    y = perturb_members(x, E, std, noise=mod).view(B, E, C, NLAT, NLON)
    z = twin.sample(B * (E - 1) * C).view(B, E - 1, C, NLAT, NLON)
    assert torch.equal(y[:, 0], x)
    assert torch.equal(y[:, 1:], x[:, None] + std * z)
    assert not torch.equal(z[:, 0], z[:, 1]) and float(z.abs().max()) > 0.5
    assert torch.equal(perturb_members(x, E, 0.0, noise=mod).view(B, E, C, NLAT, NLON)[:, 2], x)


def test_rollout_step_noise_feeds_back_only_to_the_perturbed_members(dev, tmp_path, monkeypatch):
    """Two steps of E = 3 members of the small package SFNO of the ensemble tests: with ``step_noise_std > 0`` the predictions of
    step 0 are those without it, the state fed back differs from the prediction on members 1 and 2 only, by ``step_noise_std``
    times the module's next sample, and the control's second step is untouched."""
    from makani_amd.ensemble import EnsembleScores
    from makani_amd.inference import EnsembleRollout
    from makani_amd.noise import SphericalNoise, degree_sigmas
    from makani_amd.sht import InverseRealSHT
    from test_rollout_cpu import C as CR, build, make_params, make_problem
    from test_stepper_gpu import _sfno
    monkeypatch.setenv("MK_NOISE", "hip")
    H, W, B, steps, T, E, std = 64, 128, 1, 2, 2, 3, 0.2
    params = make_params(H, W, tmp_path, steps=steps, n_history=T - 1)
    prob = make_problem(B, T, H, W, steps, seed=4)
    sig = degree_sigmas((2.0 * np.arange(LMAX) + 1.0) ** -1.0, 1.0, MMAX)

    def noise():
        return SphericalNoise(InverseRealSHT(H, W, LMAX, MMAX, "legendre-gauss"), sig, seed=nc.SEEDS[1], phi=0.5).to(dev)

    res = {}
    for step_std in (0.0, std):
        fed = []
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            wrap, _, _ = build(params, prob, dev, model=_sfno(dev, T * (CR + 1) + 3, CR, H, W))
            sc = EnsembleScores(params, E, dev)
            ro = EnsembleRollout(params, wrap, sc, E, noise_std=0.1, noise=noise(), step_noise_std=step_std)
            feedback = ro.feedback
            ro.feedback = lambda pred: fed.append((pred.clone(), feedback(pred).clone())) or fed[-1][1]
            out = ro.run(prob.inp.to(dev), prob.tar.to(dev), output_channels=[0, 1, 2])
        res[step_std] = (out, sc.finalize(), fed, ro)
    plain, noisy = res[0.0], res[std]
    assert torch.equal(noisy[0][0], plain[0][0])                                   # step 0: the same predictions and scores
    assert torch.equal(noisy[1]["crps"][0], plain[1]["crps"][0])
    assert all(torch.equal(p, f) for p, f in plain[2])
    pred, back = (t.view((B, E) + tuple(t.shape[1:])) for t in noisy[2][0])
    assert torch.equal(pred, plain[2][0][0].view(pred.shape))
    assert torch.equal(back[:, 0], pred[:, 0])
    assert all(not torch.equal(back[:, e], pred[:, e]) for e in range(1, E))
    twin = noise()
    twin.sample(B * (E - 1) * T * CR)                                             # the initial perturbation took draw 0
    z = twin.sample(B * (E - 1) * CR).view(B, E - 1, CR, H, W)
    assert torch.equal(back[:, 1:], pred[:, 1:] + std * z.to(pred.dtype))
    assert torch.equal(noisy[0][1][:, 0], plain[0][1][:, 0])                       # the control never sees the forcing
    assert all(not torch.equal(noisy[0][1][:, e], plain[0][1][:, e]) for e in range(1, E))
    assert int(noisy[3].noise.draws) == 1 + steps and int(plain[3].noise.draws) == 1
