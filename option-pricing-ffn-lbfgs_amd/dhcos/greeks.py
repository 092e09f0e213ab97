"""Analytic Greeks of the COS price (dh_surface_greeks, csrc/dh_greeks.h).

``greeks`` takes the parameters a calibration returns and a list of the reference's option dicts and
returns, from one pass on the GPU, the price and its sensitivities to the spot (delta, gamma), to
the strike (dual delta) and to the two initial variances (vega1, vega2).

What is differentiated: the reference's COS series (double_heston.py:160-192) at a FIXED truncation
range ``[a, b]`` and a fixed absolute strike.  The Greeks do not differentiate through the cumulant
range or through its ``log(K / S0) -+ 0.1`` clamp; that is the difference from a total derivative (a
bump-and-reprice quotient), of the size of the series' truncation error where the clamp is inactive
and not small where it is active.  ``price == spot * delta + strike * dual_delta`` to rounding.  The
vegas are per unit of variance (``v01``, ``v02``), not per unit of volatility.

Every argument the native library refuses is refused here first, with ``ValueError`` and before
the library is loaded.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _native
from .calibrator import PARAM_NAMES
from .pricer import resolve_call


@dataclass
class Greeks:
    """The six planes of one request: scalars (``DoubleHeston.greeks``), ``[n]`` arrays
    (``greeks_batch``), ``[M]`` for one parameter set or ``[P, M]`` for ``P`` (``dhcos.greeks``).
    Partial derivatives of the COS series at a fixed truncation range (see the module docstring):
    delta = d/dS0, gamma = d2/dS0^2, dual_delta = d/dK, vega_j = d/dv0j (per unit of variance)."""
    price: np.ndarray
    delta: np.ndarray
    gamma: np.ndarray
    dual_delta: np.ndarray
    vega1: np.ndarray
    vega2: np.ndarray

    @classmethod
    def from_planes(cls, planes):
        """planes[g] in _native.GREEKS' order -> Greeks."""
        return cls(*(planes[g] for g in range(len(_native.GREEKS))))


def check_N(N):
    if int(N) != N or not 1 <= N <= _native.MAX_N:
        raise ValueError(f"N: a whole number in [1, {_native.MAX_N}], got {N!r}")
    return int(N)


def check_L(L):
    if not np.isfinite(L) or not L > 0.0:
        raise ValueError(f"L: finite and > 0, got {L!r}")
    return float(L)


def _records(parameters, spot, risk_free, q):
    """-> ([P, 16] records, True if `parameters` was one set)."""
    if isinstance(parameters, dict):
        missing = [n for n in PARAM_NAMES if n not in parameters]
        if missing:
            raise ValueError(f"parameters: missing {missing}")
        parameters = [parameters[n] for n in PARAM_NAMES]
    p = np.asarray(parameters, dtype=np.float64)
    single = p.ndim == 1
    p = np.atleast_2d(p)
    if p.ndim != 2 or p.shape[1] != 13 or p.shape[0] < 1:
        raise ValueError(f"parameters: a dict of the 13 names, [13] or [P, 13], got {p.shape}")
    P = p.shape[0]
    rec = np.zeros((P, _native.PARAM_STRIDE))
    rec[:, :13] = p
    for name, col, v in (("spot", 13, spot), ("risk_free", 14, risk_free), ("q", 15, q)):
        v = np.asarray(v, dtype=np.float64)
        if v.shape not in ((), (P,)):
            raise ValueError(f"{name}: a scalar or [{P}], got shape {v.shape}")
        if not np.all(np.isfinite(v)):
            raise ValueError(f"{name}: must be finite")
        rec[:, col] = v
    if not np.all(rec[:, 13] > 0.0):
        raise ValueError("spot: must be > 0")
    return rec, single


def _options(options):
    """The reference's option dicts (strike, maturity, option_type) -> K, T, is_call arrays."""
    options = list(options)
    if not options:
        raise ValueError("options: at least one")
    K, T, call = np.empty(len(options)), np.empty(len(options)), np.empty(len(options), np.int8)
    for j, o in enumerate(options):
        K[j], T[j] = float(o["strike"]), float(o["maturity"])
        if not np.isfinite(K[j]) or K[j] <= 0.0:
            raise ValueError(f"options[{j}]: strike must be finite and > 0, got {K[j]}")
        if not np.isfinite(T[j]) or T[j] <= 0.0:
            raise ValueError(f"options[{j}]: maturity must be finite and > 0, got {T[j]}")
        call[j] = resolve_call(o["option_type"])
    return K, T, call


def greeks(parameters, spot, risk_free, options, N=128, q=0.0, L=10.0, device=None) -> Greeks:
    """Price and analytic Greeks of ``options`` under every parameter set, on the GPU.

    parameters: a dict of the 13 names, a ``[13]`` array or ``[P, 13]`` (what
    ``CalibrationResult.parameters`` / ``BatchCalibrationResult.parameters`` hold); spot, risk_free,
    q: scalars or ``[P]``; options: the reference's list of dicts (``strike``, ``maturity``,
    ``option_type``).  Returns ``Greeks`` of ``[M]`` arrays for one set, ``[P, M]`` for ``P``, in the
    options' order.

    The Greeks are partial derivatives of the COS series with ``N`` terms at a fixed truncation
    range (width ``L``) and strike: not through the cumulant range or its log-strike clamp (the
    module docstring).  The same call gives the same bits."""
    N, L = check_N(N), check_L(L)
    rec, single = _records(parameters, spot, risk_free, q)
    K, T, call = _options(options)
    ctx = _native.default_context(device)
    surf = _native.Surface(ctx, K, T, call)
    try:
        planes = surf.greeks(rec, N, L)
    finally:
        surf.close()
    return Greeks.from_planes(planes[:, 0] if single else planes)


__all__ = ["Greeks", "greeks"]
