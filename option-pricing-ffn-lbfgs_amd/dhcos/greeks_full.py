"""The full Greeks and Dupire's local volatility of the COS price (dh_surface_greeks_full,
csrc/dh_greeks_full.h).

``greeks_full`` returns what ``greeks`` returns, bit for bit, and from the same pass the price's
sensitivity to the maturity (``dprice_dT``; ``theta`` is its negative), to the rate (``rho``) and to
the dividend yield (``epsilon``), its second derivative in the strike (``dual_gamma``; times
``e^{rT}`` the risk-neutral ``density``) and Dupire's local variance

    local_var(K, T) = [dC/dT + (r - q) K dC/dK + q C] / [1/2 K^2 d2C/dK2]

(the same for calls and puts).  ``local_vol`` evaluates it on a strike x maturity grid in one
launch: the surface a PDE or local-stochastic-vol pricer takes.  With jumps (``lambda_j > 0``) the
model is no diffusion and the quotient is its Markovian projection: the local volatility whose
diffusion reprices the model's European options, not a volatility of the model's own paths.

Like ``greeks``, everything is a partial derivative of the COS series at a FIXED truncation range
``[a, b]`` and strike.  For ``dprice_dT`` that is not the total derivative in ``T``: the range moves
with ``T`` and is held here.  The difference is of the size of the series' truncation error where
the log-strike clamp is inactive, far below the series' own error at ``local_vol``'s default
``N = 512``; where the clamp is active (far wings, short maturities) it is not small, the dual
gamma there is at rounding level and ``local_var`` is noise or NaN (``valid`` is False where it is
NaN or negative).

Every argument the native library refuses is refused here first, with ``ValueError`` and before
the library is loaded.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _native
from .greeks import _options, _records, check_L, check_N


def _sqrt_where_nonneg(v):
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(v >= 0.0, np.sqrt(np.where(v >= 0.0, v, 0.0)), np.nan)


@dataclass
class FullGreeks:
    """The ten planes of one request, shaped as ``Greeks``' are, and the maturities and rates they
    were computed at (broadcastable to the planes).  Partial derivatives of the COS series at a
    fixed truncation range: dprice_dT = d/dT, rho = d/dr, dual_gamma = d2/dK2; local_var is
    Dupire's quotient, NaN where its denominator is not > 0, not clipped where negative."""
    price: np.ndarray
    delta: np.ndarray
    gamma: np.ndarray
    dual_delta: np.ndarray
    vega1: np.ndarray
    vega2: np.ndarray
    dprice_dT: np.ndarray
    rho: np.ndarray
    dual_gamma: np.ndarray
    local_var: np.ndarray
    maturity: np.ndarray
    risk_free: np.ndarray

    @classmethod
    def from_planes(cls, planes, maturity, risk_free):
        """planes[g] in _native.GREEKS_FULL's order -> FullGreeks."""
        return cls(*(planes[g] for g in range(len(_native.GREEKS_FULL))), maturity, risk_free)

    @property
    def theta(self):
        """The calendar decay per year: -dprice_dT."""
        return -self.dprice_dT

    @property
    def epsilon(self):
        """d price / dq, the dividend-yield sensitivity: -(rho + T price)."""
        return -(self.rho + self.maturity * self.price)

    @property
    def density(self):
        """The risk-neutral density of S_T at the strike: e^{rT} dual_gamma."""
        return np.exp(self.risk_free * self.maturity) * self.dual_gamma

    @property
    def local_vol(self):
        """sqrt(local_var) where local_var >= 0, else NaN."""
        v = _sqrt_where_nonneg(self.local_var)
        return v if v.ndim else np.float64(v)


def greeks_full(parameters, spot, risk_free, options, N=128, q=0.0, L=10.0,
                device=None) -> FullGreeks:
    """``greeks``' arguments -> ``FullGreeks``: its six planes with the same bits, and dprice_dT,
    rho, dual_gamma and local_var, of ``[M]`` arrays for one parameter set, ``[P, M]`` for ``P``, in
    the options' order; one pass on the GPU.  The same call gives the same bits."""
    N, L = check_N(N), check_L(L)
    rec, single = _records(parameters, spot, risk_free, q)
    K, T, call = _options(options)
    ctx = _native.default_context(device)
    surf = _native.Surface(ctx, K, T, call)
    try:
        planes = surf.greeks_full(rec, N, L)
    finally:
        surf.close()
    if single:
        return FullGreeks.from_planes(planes[:, 0], T, rec[0, 14])
    return FullGreeks.from_planes(planes, T[None, :], rec[:, 14][:, None])


@dataclass
class LocalVolSurface:
    """Dupire's local volatility on a grid: ``strikes`` [nK], ``maturities`` [nT], and local_vol,
    local_var, density, price (of the call) and valid of shape [nT, nK], or [P, nT, nK] for ``P``
    parameter sets.  valid: local_var is finite and >= 0; local_vol is NaN elsewhere."""
    strikes: np.ndarray
    maturities: np.ndarray
    local_vol: np.ndarray
    local_var: np.ndarray
    density: np.ndarray
    price: np.ndarray
    valid: np.ndarray


def _grid_axis(name, v):
    v = np.asarray(v, dtype=np.float64)
    if v.ndim != 1 or v.size < 1:
        raise ValueError(f"{name}: a 1-d array of at least one value, got shape {v.shape}")
    if not np.all(np.isfinite(v)) or not np.all(v > 0.0):
        raise ValueError(f"{name}: must be finite and > 0")
    return v


def local_vol(parameters, spot, risk_free, strikes, maturities, N=512, q=0.0, L=10.0,
              device=None) -> LocalVolSurface:
    """Dupire's local volatility of the model on ``strikes`` x ``maturities``: one surface of calls
    over the grid, one launch.  Entry [i, j] (``[p, i, j]``) is ``greeks_full``'s of the call
    (strikes[j], maturities[i]), bit for bit.  See the module docstring for what the quotient means
    with jumps and where it is not to be trusted (``valid``)."""
    N, L = check_N(N), check_L(L)
    rec, single = _records(parameters, spot, risk_free, q)
    K, T = _grid_axis("strikes", strikes), _grid_axis("maturities", maturities)
    nT, nK = T.size, K.size
    Kg, Tg = np.tile(K, nT), np.repeat(T, nK)
    ctx = _native.default_context(device)
    surf = _native.Surface(ctx, Kg, Tg, np.ones(nT * nK, dtype=np.int8))
    try:
        planes = surf.greeks_full(rec, N, L)
    finally:
        surf.close()
    planes = planes.reshape(len(_native.GREEKS_FULL), rec.shape[0], nT, nK)
    g = {name: planes[i] for i, name in enumerate(_native.GREEKS_FULL)}
    density = np.exp(rec[:, 14][:, None, None] * T[None, :, None]) * g["dual_gamma"]
    var = g["local_var"]
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(var) & (var >= 0.0)
    out = [_sqrt_where_nonneg(var), var, density, g["price"], valid]
    if single:
        out = [x[0] for x in out]
    return LocalVolSurface(K, T, *out)


__all__ = ["FullGreeks", "greeks_full", "LocalVolSurface", "local_vol"]
