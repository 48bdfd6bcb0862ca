"""Correlated noise on the sphere for ensemble members: an isotropic Gaussian random field with a prescribed spectrum.

White grid noise (``noise_std * torch.randn``) has no spatial correlation, a variance per unit area that grows towards the
poles of an equiangular grid, and nearly all of its power in degrees the first ``RealSHT`` of a network truncates away.  Here
the spherical-harmonic coefficients are drawn independently with a variance per degree (``ops.noise_spectrum``: one HIP pass
straight into the packed spectrum ``[L, M, BC]``, reproducible, capturable, independent of the sharding), optionally evolved
as an AR(1) process from call to call, and synthesised by the inverse transform the caller hands over.  The reference has no
such component; DESIGN section 41 has the definitions and the error bounds.

    isht = InverseRealSHT(nlat, nlon, lmax, mmax, grid)
    noise = SphericalNoise(isht, degree_sigmas(power_law_spectrum(lmax, 2.0), 1.0, mmax), seed=7).to(device)
    field = noise.sample(rows)                                   # [rows, nlat, nlon], unit area-mean variance
"""
import math

import numpy as np
import torch
import torch.nn as nn

from . import ops


def power_law_spectrum(lmax, alpha):
    """``S_l = (2 l + 1)^-alpha`` for l = 0 ... lmax - 1 (float64): ``alpha = 0`` is white, larger is smoother."""
    return (2.0 * np.arange(int(lmax), dtype=np.float64) + 1.0) ** -float(alpha)


def diffusion_spectrum(lmax, kT):
    """``S_l = exp(-kT l (l + 1))`` (float64): white noise after diffusion on the unit sphere for a time ``kT``."""
    l = np.arange(int(lmax), dtype=np.float64)
    return np.exp(-float(kT) * l * (l + 1.0))


def degree_sigmas(S, sigma, mmax):
    """The standard deviation per degree, float64 ``[lmax]``, that gives the synthesised field the area-mean variance ``sigma^2``:
    ``sigma_l = sigma sqrt(S_l / (sum_l n_l S_l / 4 pi))`` with ``n_l = 1 + 2 min(l, mmax - 1)`` the real degrees of freedom the
    truncation keeps of degree l (order 0 is real, every order m > 0 stands for +-m in the real inverse FFT), the harmonics
    orthonormal on the unit sphere."""
    S = np.asarray(S, dtype=np.float64).reshape(-1)
    if S.size < 1 or not np.isfinite(S).all() or (S < 0).any() or not (S > 0).any():
        raise ValueError("degree_sigmas: the spectrum must be finite, non-negative and not all zero")
    n = 1.0 + 2.0 * np.minimum(np.arange(S.size), int(mmax) - 1)
    return float(sigma) * np.sqrt(S / (np.sum(n * S) / (4.0 * math.pi)))


class SphericalNoise(nn.Module):
    """An isotropic Gaussian random field, white in time (``phi == 0``) or AR(1) with lag-one correlation ``phi``, on the grid of
    ``inverse_transform`` (an ``InverseRealSHT`` or ``DistributedInverseRealSHT``, which supplies ``lmax``, ``mmax``, the grid and,
    sharded, this rank's offsets and extents).  ``sigmas`` is float ``[lmax]`` (``degree_sigmas``), ``seed`` an int in [0, 2^64),
    ``row_scale`` an optional factor per row (fp32 ``[rows]``, e.g. a per-channel amplitude repeated over the batch).

    The draw of ``(row, degree, order)`` at call number T depends on exactly those four and the seed: a shard draws the slice of
    the unsharded field, and two modules with one seed agree.  The call counter lives on the device and is advanced by a torch
    op on the current stream, so ``coefficients`` / ``sample`` make no host synchronisation and may be captured in a graph (a
    replay draws the next field)."""

    def __init__(self, inverse_transform, sigmas, seed=0, phi=0.0, row_scale=None):
        super().__init__()
        tr = inverse_transform
        for name in ("inverse_packed", "lmax", "mmax", "nlat", "nlon"):
            if not hasattr(tr, name):
                raise TypeError(f"SphericalNoise: the inverse transform has no {name!r} (an InverseRealSHT or DistributedInverseRealSHT)")
        self.inverse_transform = tr
        self.distributed = hasattr(tr, "lmax_local")
        self.lmax, self.mmax, self.nlat, self.nlon = tr.lmax, tr.mmax, tr.nlat, tr.nlon
        self.l_off, self.m_off = (tr.l_off, tr.m_off) if self.distributed else (0, 0)
        self.l_loc, self.m_loc = (tr.lmax_local, tr.mmax_local) if self.distributed else (tr.lmax, tr.mmax)
        sig = np.asarray(sigmas.detach().cpu() if torch.is_tensor(sigmas) else sigmas, dtype=np.float64).reshape(-1)
        if sig.size != self.lmax or not np.isfinite(sig).all() or (sig < 0).any():
            raise ValueError(f"SphericalNoise: sigmas must be {self.lmax} finite non-negative values, got {sig.size}")
        self.phi = float(phi)
        if not 0.0 <= self.phi < 1.0:
            raise ValueError(f"SphericalNoise: phi {phi} outside [0, 1)")
        self.seed = self._check_seed(seed)
        self.register_buffer("sigma_l", torch.from_numpy(sig[self.l_off:self.l_off + self.l_loc].astype(np.float32)), persistent=False)
        self.register_buffer("row_scale", None if row_scale is None else torch.as_tensor(row_scale).detach().float().reshape(-1).clone(),
                             persistent=False)
        self.register_buffer("draws", torch.zeros(1, dtype=torch.int32), persistent=False)
        self.state = None
        self._state_key = None

    @staticmethod
    def _check_seed(seed):
        seed = int(seed)
        if not 0 <= seed < 1 << 64:
            raise ValueError(f"SphericalNoise: seed {seed} outside [0, 2^64)")
        return seed

    def reset(self, seed=None):
        """Back to draw 0 (of ``seed``, if given) and without a state: the next call is a fresh draw."""
        if seed is not None:
            self.seed = self._check_seed(seed)
        self.draws.zero_()
        self.state = None
        self._state_key = None

    @torch.no_grad()
    def coefficients(self, rows, row0=0):
        """One step of the process for global rows ``row0 ... row0 + rows - 1`` (``row0`` even): the packed state, complex64
        ``[l_loc, m_loc, rows]``, which the module keeps and the next call overwrites.  ``phi == 0``, and the first call for a
        state (after ``reset`` or with another ``rows`` / ``row0`` / device), draw afresh; otherwise the state takes the AR(1)
        update.  Then the draw counter goes up by one."""
        rows, row0 = int(rows), int(row0)
        if rows < 1:
            raise ValueError(f"SphericalNoise: rows must be at least 1, got {rows}")
        if self.row_scale is not None and self.row_scale.numel() != rows:
            raise ValueError(f"SphericalNoise: row_scale has {self.row_scale.numel()} entries, asked for {rows} rows")
        key = (rows, row0, self.draws.device)
        fresh = self.state is None or self._state_key != key
        if fresh:
            self.state = torch.empty((self.l_loc, self.m_loc, rows), dtype=torch.complex64, device=self.draws.device)
            self._state_key = key
        ops.noise_spectrum(self.state, self.sigma_l, self.seed, t=0, t_dev=self.draws, phi=0.0 if fresh else self.phi,
                           row_scale=self.row_scale, l_off=self.l_off, m_off=self.m_off, row0=row0)
        self.draws.add_(1)
        return self.state

    @torch.no_grad()
    def sample(self, rows, batch=None, row0=0, out_dtype=torch.float32):
        """One field per row: ``[rows, nlat_loc, nlon_loc]`` in ``out_dtype``, ``coefficients`` synthesised by the transform's
        ``inverse_packed``.  ``batch`` (default 1) is the batch extent the sharded transform splits ``rows`` = batch x channels
        by for its channel transposes; the local transform does not need it."""
        c = self.coefficients(rows, row0)
        if self.distributed:
            x = self.inverse_transform.inverse_packed(c, int(batch or 1), out_dtype)
            return x.reshape(rows, x.shape[-2], x.shape[-1])
        return self.inverse_transform.inverse_packed(c, out_dtype)

    def extra_repr(self):
        return f"lmax={self.lmax}, mmax={self.mmax}, seed={self.seed}, phi={self.phi}"
