"""CPU tests of the spherical noise: the Philox words of the C library against the Random123 known answers and the numpy
restatement (tests/noise_checks.py), ``ops.noise_spectrum`` on CPU tensors (the torch formulation) within the derived bound of
that restatement, the bound's teeth, ``degree_sigmas``, the refusals of ``mk_noise_spectrum`` (before any launch: no GPU needed),
the ``MK_NOISE`` switch, and that ``perturb_members`` without a noise module is what it was."""
import math
import re

import numpy as np
import pytest
import torch

import capi_checks as capi
import noise_checks as nc

from makani_amd import _lib, ops
from oracle import sht as osht

BIG_SEED = nc.SEEDS[1]          # top bit set: travels as a negative long long


def _sigmas(L, l_off=0):
    """A positive fp32 table that differs from degree to degree."""
    return (0.5 + 1.0 / (1.0 + np.arange(l_off, l_off + L))).astype(np.float32)


def _draw(L, M, BC, seed, t, l_off=0, m_off=0, row0=0, row_scale=None, phi=0.0, state=None, t_dev=None, sigma=None):
    state = torch.full((L, M, BC), complex(float("nan"), float("nan")), dtype=torch.complex64) if state is None else state
    sigma = _sigmas(L, l_off) if sigma is None else sigma
    ops.noise_spectrum(state, torch.from_numpy(sigma), seed, t=t, t_dev=t_dev, phi=phi, l_off=l_off, m_off=m_off, row0=row0,
                       row_scale=None if row_scale is None else torch.from_numpy(row_scale))
    return state


# ---------------------------------------------------------------------------------------------------------------------
# the words
# ---------------------------------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_known_answers():
    for ctr, key, want in nc.KNOWN_ANSWERS:
        assert tuple(int(w) for w in nc.philox(*ctr, *key)) == want


def test_library_words_are_the_known_answers_and_the_restatement():
    lib = _lib.load()
    for ctr, key, want in nc.KNOWN_ANSWERS:
        assert tuple(ops.noise_words(key[0] | (key[1] << 32), *ctr)) == want
    for q, l, m, t in [(0, 0, 0, 0), (5, 31, 17, 3), (2 ** 32 - 1, 2 ** 31 - 1, 240, 2 ** 31 - 1)]:
        for seed in nc.SEEDS + (2 ** 64 - 1,):
            assert ops.noise_words(seed, q, l, m, t) == nc.words(seed, q, l, m, t), (seed, q, l, m, t)
    # the raw ABI: the seed as a two's complement long long, the words as two's complement ints
    out = (np.zeros(4, dtype=np.int32))
    assert lib.mk_noise_words(BIG_SEED - (1 << 64), 7, 3, 2, 1, out.ctypes.data) == 0
    assert [int(v) for v in out.view(np.uint32)] == nc.words(BIG_SEED, 7, 3, 2, 1)


def test_torch_rounds_are_the_known_answers():
    """The int64 rounds the torch formulation draws from (``ops._philox_torch``: products that wrap past int63)."""
    for ctr, key, want in nc.KNOWN_ANSWERS:
        got = ops._philox_torch(*(torch.tensor([c], dtype=torch.int64) for c in ctr), key[0] | (key[1] << 32))
        assert tuple(int(w) for w in got) == want


# ---------------------------------------------------------------------------------------------------------------------
# the torch formulation against the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", nc.SEEDS, ids=["seed0", "seedbig"])
@pytest.mark.parametrize("t", [0, 3])
@pytest.mark.parametrize("BC", [1, 5, 6])
def test_torch_formulation_within_the_bound_and_shards_are_slices(BC, t, seed):
    L, M, l_off, m_off = 9, 11, 16, 22
    rs = np.linspace(0.25, 2.0, BC).astype(np.float32)
    for scale in (None, rs):
        got = _draw(L, M, BC, seed, t, l_off, m_off, row_scale=scale).numpy()
        xi, bound, _ = nc.restate(_sigmas(L, l_off), L, M, BC, seed, t, l_off, m_off, row_scale=scale)
        assert (bound == 0).sum() == BC * sum(1 for l in range(L) for m in range(M) if l_off + l < m_off + m) > 0
        ratio = nc.worst_ratio(got, xi, bound)
        print(f"[noise cpu] BC={BC} t={t} seed={seed:#x} scale={scale is not None}: worst error / bound {ratio:.3f}")
        assert ratio <= 1.0
    # the shard is the slice of the full draw, bit for bit
    full = _draw(32, 33, BC, seed, t, sigma=_sigmas(32)).numpy()
    shard = _draw(L, M, BC, seed, t, l_off, m_off, sigma=_sigmas(32)[l_off:l_off + L]).numpy()
    assert np.array_equal(shard.view(np.uint32), np.ascontiguousarray(full[l_off:l_off + L, m_off:m_off + M]).view(np.uint32))
    assert (full[:, 0].imag == 0).all() and (full[1:, 1].imag != 0).any()          # order 0 is real, the others are not


def test_rows_are_global_and_the_step_counts():
    """``row0`` shifts the rows (a row shard is a slice), ``t`` and ``t_dev`` add, and different steps differ."""
    full = _draw(6, 7, 6, BIG_SEED, 2)
    part = _draw(6, 7, 4, BIG_SEED, 2, row0=2)
    assert torch.equal(torch.view_as_real(part), torch.view_as_real(full[:, :, 2:]))
    by_dev = _draw(6, 7, 6, BIG_SEED, 0, t_dev=torch.tensor([2], dtype=torch.int32))
    assert torch.equal(torch.view_as_real(by_dev), torch.view_as_real(full))
    assert not torch.equal(torch.view_as_real(_draw(6, 7, 6, BIG_SEED, 3)), torch.view_as_real(full))
    assert not torch.equal(torch.view_as_real(_draw(6, 7, 6, 1, 2)), torch.view_as_real(full))


@pytest.mark.parametrize("variant", ["swap", "nosqrt2", "odd01"])
def test_the_bound_is_not_vacuous(variant):
    """A draw with the parts swapped, without the 1 / sqrt 2, or with the odd row on the even row's words is outside the bound."""
    L, M, BC = 9, 11, 6
    got = _draw(L, M, BC, BIG_SEED, 3).numpy()
    xi, bound, _ = nc.restate(_sigmas(L), L, M, BC, BIG_SEED, 3, variant=variant)
    assert nc.worst_ratio(got, xi, bound) > 1e3


def test_ar1_steps_follow_the_restated_recursion():
    L, M, BC, phi, seed = 9, 11, 5, 0.5, BIG_SEED
    state = _draw(L, M, BC, seed, 0)
    S, bS, _ = nc.restate(_sigmas(L), L, M, BC, seed, 0)
    for t in (1, 2):
        _draw(L, M, BC, seed, t, phi=phi, state=state)
        xi, bxi, _ = nc.restate(_sigmas(L), L, M, BC, seed, t)
        S, bS = nc.ar1(S, bS, xi, bxi, phi)
        bS = np.where(bxi == 0, 0.0, bS)
        ratio = nc.worst_ratio(state.numpy(), S, bS)
        print(f"[noise cpu] AR(1) update {t}: worst error / bound {ratio:.3f}")
        assert ratio <= 1.0
    fresh, _, _ = nc.restate(_sigmas(L), L, M, BC, seed, 2)
    assert nc.worst_ratio(state.numpy(), fresh, bxi) > 1e3            # it is not simply the latest draw


# ---------------------------------------------------------------------------------------------------------------------
# spectra and the variance
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lmax,mmax", [(32, 33), (32, 12), (240, 241)])
def test_degree_sigmas_normalise_the_area_mean_variance(lmax, mmax):
    from makani_amd import noise
    for S in (noise.power_law_spectrum(lmax, 1.5), noise.diffusion_spectrum(lmax, 3e-3), np.ones(lmax)):
        for sigma in (1.0, 0.3):
            sig = noise.degree_sigmas(S, sigma, mmax)
            assert sig.dtype == np.float64 and sig.shape == (lmax,)
            n = 1.0 + 2.0 * np.minimum(np.arange(lmax), mmax - 1)
            assert abs(np.sum(n * sig ** 2) / (4.0 * math.pi) - sigma ** 2) <= 1e-12
    assert np.array_equal(noise.power_law_spectrum(4, 2.0), np.array([1.0, 1 / 9, 1 / 25, 1 / 49]))
    assert np.allclose(noise.diffusion_spectrum(3, 0.5), np.exp([-0.0, -1.0, -3.0]), rtol=1e-15)
    with pytest.raises(ValueError):
        noise.degree_sigmas(np.zeros(4), 1.0, 5)


@pytest.mark.parametrize("seed,want", zip(nc.SEEDS, (1.0, 0.6)), ids=["seed0", "seedbig"])
def test_restated_field_has_the_prescribed_variance(seed, want):
    """The premise of the GPU statistics test, on the restatement alone: white spectrum, 63 rows, T = 3, the 32 x 64
    Legendre-Gauss grid; the mean over rows of the area-weighted variance lies ``want`` standard errors from sigma^2."""
    from makani_amd import noise
    L, M, rows, sigma = 32, 33, 63, 0.7
    sig = noise.degree_sigmas(np.ones(L), sigma, M).astype(np.float32)
    xi, _, _ = nc.restate(sig, L, M, rows, seed, 3)
    x = osht.InverseRealSHT(32, 64, L, M, "legendre-gauss", dtype=np.float64)(np.moveaxis(xi, -1, 0))
    _, w = osht.quadrature("legendre-gauss", 32)
    se = math.sqrt(2.0 / 1024.0) / math.sqrt(rows)
    dev = (nc.area_variance(x, w).mean() / sigma ** 2 - 1.0) / se
    print(f"[noise cpu] seed {seed:#x}: variance ratio {1.0 + dev * se:.4f}, {dev:+.2f} standard errors")
    assert abs(dev) <= 5.0 and abs(abs(dev) - want) < 0.1


# ---------------------------------------------------------------------------------------------------------------------
# the C entry points refuse before any launch
# ---------------------------------------------------------------------------------------------------------------------
_A = capi.A
_OK = dict(state=_A, sigma_l=_A, row_scale=None, L=9, M=11, BC=6, l_off=0, m_off=0, row0=0, seed=1, t=0, t_dev=None, phi=0.0)
NOISE_REJECTED = [      # the argument mk_noise_spectrum must refuse (everything else valid), the message
    (dict(state=None), "null pointer"),
    (dict(sigma_l=None), "null pointer"),
    (dict(state=_A + 8), "state is not 16-byte aligned"),
    (dict(state=_A + 8, BC=5), "state is not 16-byte aligned"),
    (dict(sigma_l=_A + 2), "a table is not 4-byte aligned"),
    (dict(L=0), "bad sizes"),
    (dict(M=0), "bad sizes"),
    (dict(BC=0), "bad sizes"),
    (dict(l_off=-1), "negative offset"),
    (dict(m_off=-1), "negative offset"),
    (dict(l_off=2 ** 31 - 5), "global degree or order out of range"),
    (dict(row0=3), "row0 must be even and non-negative"),
    (dict(row0=-2), "row0 must be even and non-negative"),
    (dict(row0=2 ** 33 - 4), "the row pair index q passes 2^32"),
    (dict(BC=2 ** 33 + 1), "the row pair index q passes 2^32"),
    (dict(BC=2 ** 40), "too many rows"),
    (dict(phi=1.0), "phi outside [0, 1)"),
    (dict(phi=-0.25), "phi outside [0, 1)"),
    (dict(phi=float("nan")), "phi outside [0, 1)"),
    (dict(L=2 ** 20, M=2 ** 20, BC=2 ** 5), "L * M * ceil(BC / 2) beyond the kernel's 32-bit index (2^31 threads)"),
    (dict(L=2 ** 10, M=2 ** 10, BC=2 ** 12), "L * M * ceil(BC / 2) beyond the kernel's 32-bit index (2^31 threads)"),      # exactly 2^31
]


@pytest.mark.parametrize("bad,msg", NOISE_REJECTED, ids=[f"{'-'.join(f'{k}={v}' for k, v in b.items())}" for b, _ in NOISE_REJECTED])
def test_noise_spectrum_refuses_bad_input_before_any_launch(bad, msg):
    a = dict(_OK, **bad)
    capi.assert_refused("mk_noise_spectrum", tuple(a[k] for k in _OK), msg)


def test_the_last_valid_pair_index_is_not_refused_for_its_size():
    """row0 = 2^33 - 6 with 6 rows ends at pair 2^32 - 1: the refusal, if any, is not about q (the null state is, first)."""
    a = dict(_OK, row0=2 ** 33 - 6, state=None)
    capi.assert_refused("mk_noise_spectrum", tuple(a[k] for k in _OK), "null pointer")


@pytest.mark.parametrize("args,msg", [((1, 0, 0, 0, 0, None), "null pointer"), ((1, 2 ** 32, 0, 0, 0, _A), "q outside [0, 2^32)"),
                                      ((1, -1, 0, 0, 0, _A), "q outside [0, 2^32)")])
def test_noise_words_refuses_bad_input(args, msg):
    lib = _lib.load()
    lib.mk_quadrature(7, 10, 0, 0)
    assert lib.mk_noise_words(*args) == 1
    assert lib.mk_last_error() == f"mk_noise_words: {msg}".encode()


def test_op_refuses_what_it_cannot_draw():
    st = torch.zeros(4, 5, 3, dtype=torch.complex64)
    sig = torch.ones(4)
    for kw in (dict(seed=-1), dict(seed=2 ** 64), dict(phi=1.0), dict(row0=1), dict(l_off=-1), dict(t=-1)):
        with pytest.raises(ValueError):
            ops.noise_spectrum(st, sig, **dict(dict(seed=0), **kw))
    with pytest.raises(ValueError):
        ops.noise_spectrum(st.to(torch.complex128), sig, 0)
    with pytest.raises(ValueError):
        ops.noise_spectrum(st, torch.ones(5), 0)
    with pytest.raises(ValueError):
        ops.noise_spectrum(st, sig, 0, row_scale=torch.ones(4))
    with pytest.raises(ValueError):
        ops.noise_spectrum(st, sig, 0, t_dev=torch.zeros(1, dtype=torch.int64))


# ---------------------------------------------------------------------------------------------------------------------
# the switch, the module on the CPU, the members
# ---------------------------------------------------------------------------------------------------------------------
def test_mk_noise_validates_like_the_other_switches(monkeypatch):
    assert ops.KNOBS["MK_NOISE"] == ("hip", "torch") and ops.NOISE_DEFAULT in ops.KNOBS["MK_NOISE"]
    st, sig = torch.zeros(4, 5, 3, dtype=torch.complex64), torch.ones(4)
    for v in ops.KNOBS["MK_NOISE"]:
        monkeypatch.setenv("MK_NOISE", v)
        ops.noise_spectrum(st, sig, 0)                      # CPU tensors take the torch formulation under either value
    monkeypatch.setenv("MK_NOISE", "bogus")
    with pytest.raises(ValueError, match=re.escape("unknown MK_NOISE 'bogus' (hip | torch)")):
        ops.noise_spectrum(st, sig, 0)


class _Grid:
    """What ``SphericalNoise`` asks of a transform, without its tables: the coefficients need no synthesis."""
    lmax, mmax, nlat, nlon = 9, 11, 12, 24

    def inverse_packed(self, c, out_dtype=torch.float32):
        raise AssertionError("not called")


def test_module_counts_draws_and_keeps_an_ar1_state():
    from makani_amd.noise import SphericalNoise
    sig = _sigmas(9).astype(np.float64)
    white = SphericalNoise(_Grid(), sig, seed=BIG_SEED)
    a = white.coefficients(5).clone()
    b = white.coefficients(5).clone()
    assert int(white.draws) == 2 and white.state.shape == (9, 11, 5)
    assert torch.equal(torch.view_as_real(a), torch.view_as_real(_draw(9, 11, 5, BIG_SEED, 0)))
    assert torch.equal(torch.view_as_real(b), torch.view_as_real(_draw(9, 11, 5, BIG_SEED, 1)))
    white.reset()
    assert int(white.draws) == 0 and white.state is None
    assert torch.equal(torch.view_as_real(white.coefficients(5)), torch.view_as_real(a))
    red = SphericalNoise(_Grid(), sig, seed=BIG_SEED, phi=0.5, row_scale=np.full(5, 2.0, dtype=np.float32))
    first = red.coefficients(5).clone()
    assert torch.equal(torch.view_as_real(first), torch.view_as_real(_draw(9, 11, 5, BIG_SEED, 0, row_scale=np.full(5, 2.0, np.float32))))
    second = red.coefficients(5)
    want = _draw(9, 11, 5, BIG_SEED, 1, row_scale=np.full(5, 2.0, np.float32), phi=0.5, state=first.clone())
    assert torch.equal(torch.view_as_real(second), torch.view_as_real(want))
    assert "sigma_l" not in red.state_dict() and "draws" not in red.state_dict()
    with pytest.raises(ValueError):
        red.coefficients(6)                                  # the row scale has five entries
    with pytest.raises(ValueError):
        SphericalNoise(_Grid(), sig[:-1])
    with pytest.raises(ValueError):
        SphericalNoise(_Grid(), sig, phi=1.0)


def test_perturb_members_without_noise_is_what_it_was():
    from makani_amd.ensemble import perturb_members
    x = torch.randn(2, 3, 4, 6, generator=torch.Generator().manual_seed(1))
    B, E, std = 2, 3, 0.25
    want = x.repeat_interleave(E, dim=0)
    want.view(B, E, 3, 4, 6)[:, 1:] += std * torch.randn((B, E - 1, 3, 4, 6), generator=torch.Generator().manual_seed(5))
    assert torch.equal(perturb_members(x, E, std, generator=torch.Generator().manual_seed(5)), want)
    assert torch.equal(perturb_members(x, E, std, generator=torch.Generator().manual_seed(5), noise=None), want)
    assert torch.equal(perturb_members(x, E, 0.0), x.repeat_interleave(E, dim=0))


def test_perturb_members_takes_the_documented_rows_of_a_noise_module():
    """A stand-in module that returns its row numbers: member 0 is the input, member e of sample b gets rows
    ``(b (E - 1) + e - 1) C + c``."""
    from makani_amd.ensemble import perturb_members

    class Rows:
        def sample(self, rows, batch=None, row0=0, out_dtype=torch.float32):
            self.asked = (rows, batch)
            return torch.arange(rows, dtype=torch.float32).view(rows, 1, 1).expand(rows, 4, 6)

    B, E, C = 2, 3, 5
    x = torch.zeros(B, C, 4, 6)
    mod = Rows()
    y = perturb_members(x, E, 2.0, noise=mod).view(B, E, C, 4, 6)
    assert mod.asked == (B * (E - 1) * C, B * (E - 1))
    assert not y[:, 0].any()
    for b in range(B):
        for e in range(1, E):
            for c in range(C):
                assert (y[b, e, c] == 2.0 * ((b * (E - 1) + e - 1) * C + c)).all()
