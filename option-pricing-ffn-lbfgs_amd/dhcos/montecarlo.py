"""Monte Carlo path pricing under the Double-Heston + Merton-jump model (dh_mc_price, csrc/dh_mc.h).

``monte_carlo`` takes the parameters a calibration returns (``CalibrationResult.parameters``, a
row or all rows of ``BatchCalibrationResult.parameters``) and prices European, arithmetic Asian and
discretely monitored knock-out options from one set of simulated paths on the GPU; DESIGN.md 3.15
is the scheme.  Every argument the native library refuses is refused here first, with
``ValueError`` and before the library is loaded.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _native
from .calibrator import PARAM_NAMES
from .pricer import resolve_call

KINDS = dict(_native.MC_KINDS)
MAX_OPTIONS = _native.MC_MAX_OPTIONS
MAX_SETS = 65535                 # parameter sets of one call (the launch grid's second axis)
_STEP_TOL = 1e-9                 # a maturity is n steps when |T steps_per_year - n| <= 1e-9 n


@dataclass
class MonteCarloResult:
    """Prices and their standard errors: ``[n_options]`` for one parameter set, ``[P, n_options]``
    for ``P``; the rest echoes the call (the result is a function of these and the inputs alone)."""
    price: np.ndarray
    stderr: np.ndarray
    n_paths: int
    steps_per_year: int
    seed: int

    def confidence(self, z: float = 1.96):
        """(low, high) = price -+ z stderr."""
        return self.price - z * self.stderr, self.price + z * self.stderr


@dataclass
class VarianceReducedResult(MonteCarloResult):
    """``monte_carlo`` with ``antithetic`` and / or ``control_variate`` (dh_mc_price_vr, DESIGN.md
    3.15.2).  ``price`` / ``stderr`` are the reduced estimator's; ``base_price`` / ``base_stderr``
    the plain mean of the same samples (pair averages under ``antithetic``); ``beta`` the fitted
    control coefficient (0 without a control) and ``control_mean`` the control's known mean: spot
    for Europeans and strike-0 options, else the COS price of the option's European twin (NaN
    without a control).  ``n_paths`` counts walks: ``n_paths / 2`` pairs under ``antithetic``.
    beta is fitted on the priced sample, so ``price`` carries the usual O(1 / n) bias."""
    base_price: np.ndarray = None
    base_stderr: np.ndarray = None
    beta: np.ndarray = None
    control_mean: np.ndarray = None
    antithetic: bool = False
    control_variate: bool = False

    @property
    def variance_ratio(self):
        """(base_stderr / stderr)^2: the variance the control removed from the same samples (inf
        where the control is the payoff itself, NaN where both errors are 0)."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return (self.base_stderr / self.stderr) ** 2


def _vr_flags(antithetic, control_variate, n_paths):
    """The DH_MC_VR_* flags of the two keywords, 0 for the plain pricer."""
    flags = (_native.MC_VR_ANTITHETIC if antithetic else 0) \
        | (_native.MC_VR_CONTROL if control_variate else 0)
    if antithetic and (n_paths % 2 or n_paths < 4):
        raise ValueError(f"n_paths: counts walks, so with antithetic=True an even number >= 4, "
                         f"got {n_paths!r}")
    return flags


def _records(parameters, spot, risk_free):
    """-> ([P, 16] records, True if `parameters` was one set)."""
    if isinstance(parameters, dict):
        missing = [n for n in PARAM_NAMES if n not in parameters]
        if missing:
            raise ValueError(f"parameters: missing {missing}")
        parameters = [parameters[n] for n in PARAM_NAMES]
    p = np.asarray(parameters, dtype=np.float64)
    single = p.ndim == 1
    p = np.atleast_2d(p)
    if p.ndim != 2 or p.shape[1] != 13:
        raise ValueError(f"parameters: a dict of the 13 names, [13] or [P, 13], got {p.shape}")
    P = p.shape[0]
    if not 1 <= P <= MAX_SETS:
        raise ValueError(f"parameters: 1 to {MAX_SETS} sets per call, got {P}")
    rec = np.zeros((P, _native.PARAM_STRIDE))
    rec[:, :13] = p
    for name, col, v in (("spot", 13, spot), ("risk_free", 14, risk_free)):
        v = np.asarray(v, dtype=np.float64)
        if v.shape not in ((), (P,)):
            raise ValueError(f"{name}: a scalar or [{P}], got shape {v.shape}")
        rec[:, col] = v
    return rec, single


def _check_records(rec, steps_per_year):
    names = PARAM_NAMES + ["spot", "risk_free"]
    bad = ~np.isfinite(rec[:, :15])
    if bad.any():
        p, k = np.argwhere(bad)[0]
        raise ValueError(f"{names[k]} of set {p} is not finite")

    def need(ok, k, why):
        if not ok.all():
            raise ValueError(f"{names[k]} of set {int(np.argmin(ok))} {why}")

    for f in (0, 5):
        need(rec[:, f] >= 0.0, f, "must be >= 0")
        for k in (f + 1, f + 2, f + 3):
            need(rec[:, k] > 0.0, k, "must be > 0")
        need(np.abs(rec[:, f + 4]) < 1.0, f + 4, "must lie inside (-1, 1)")
    need(rec[:, 10] >= 0.0, 10, "must be >= 0")
    need(rec[:, 10] / float(steps_per_year) <= 1.0, 10,
         "gives lambda dt > 1 (the Poisson walk's cap): raise steps_per_year")
    need(rec[:, 12] >= 0.0, 12, "must be >= 0")
    need(rec[:, 13] > 0.0, 13, "must be > 0")


def _check_steps_per_year(steps_per_year):
    if int(steps_per_year) != steps_per_year or steps_per_year < 1:
        raise ValueError(f"steps_per_year: a whole number >= 1, got {steps_per_year!r}")
    return int(steps_per_year)


def _check_seed(seed):
    if int(seed) != seed or not 0 <= seed < 1 << 64:
        raise ValueError(f"seed: an integer in [0, 2^64), got {seed!r}")
    return int(seed)


def _maturity_step(j, T, steps_per_year):
    """The step of maturity ``T`` of option ``j``: a whole number >= 1 of steps."""
    ns = T * steps_per_year
    n = np.rint(ns)
    if not np.isfinite(ns) or n < 1 or n > 2147483647 or abs(ns - n) > _STEP_TOL * n:
        raise ValueError(f"options[{j}]: maturity {T} is not a whole number (>= 1) of steps "
                         f"of 1/{steps_per_year}")
    return int(n)


def _options(options, steps_per_year):
    """The reference's option dicts (strike, maturity, option_type; optional kind, barrier) ->
    an array of dh_mc_option."""
    options = list(options)
    if not 1 <= len(options) <= MAX_OPTIONS:
        raise ValueError(f"options: 1 to {MAX_OPTIONS} per call, got {len(options)}")
    arr = (_native.McOption * len(options))()
    for j, o in enumerate(options):
        kind = o.get("kind", "european")
        if kind not in KINDS:
            raise ValueError(f"options[{j}]: unknown kind {kind!r} (one of {sorted(KINDS)})")
        strike, T = float(o["strike"]), float(o["maturity"])
        if not np.isfinite(strike) or strike < 0.0:
            raise ValueError(f"options[{j}]: strike must be finite and >= 0, got {strike}")
        _maturity_step(j, T, steps_per_year)
        barrier = 0.0
        if kind in ("up_and_out", "down_and_out"):
            if "barrier" not in o:
                raise ValueError(f"options[{j}]: a {kind} option needs a barrier")
            barrier = float(o["barrier"])
            if not barrier > 0.0:
                raise ValueError(f"options[{j}]: barrier must be > 0, got {barrier}")
        arr[j] = _native.McOption(KINDS[kind], int(resolve_call(o["option_type"])), strike, T,
                                  barrier)
    return arr


def monte_carlo(parameters, spot, risk_free, options, *, n_paths=1 << 20, steps_per_year=64,
                seed=0, device=None, antithetic=False,
                control_variate=False) -> MonteCarloResult:
    """Price ``options`` by simulating the model's SDE on the GPU.

    parameters: a dict of the 13 names, a ``[13]`` array or ``[P, 13]`` (what
    ``CalibrationResult.parameters`` / ``BatchCalibrationResult.parameters`` hold); spot, risk_free:
    scalars or ``[P]``; options: the reference's list of dicts (``strike``, ``maturity``,
    ``option_type``) with optional ``kind`` (``"european"``, ``"asian"``, ``"up_and_out"``,
    ``"down_and_out"``) and ``barrier``.  Every maturity must be a whole number of steps of
    ``1 / steps_per_year``; barriers and averages are monitored at every step date.  All parameter
    sets see the same random numbers, and the same call gives the same bits.

    antithetic: walk every path together with its mirror (the same random words, ``1 - U`` and
    ``-Z``) and average the two payoffs; ``n_paths`` counts walks and must be even and >= 4.
    control_variate: subtract ``beta`` times a control's deviation from its known mean -- the
    discounted terminal spot for Europeans, the COS price of the European twin for Asians and
    barriers.  With either keyword the result is a ``VarianceReducedResult``; with neither the call
    is the plain pricer's, unchanged."""
    steps_per_year = _check_steps_per_year(steps_per_year)
    seed = _check_seed(seed)
    if int(n_paths) != n_paths or n_paths < 2:
        raise ValueError(f"n_paths: a whole number >= 2, got {n_paths!r}")
    flags = _vr_flags(antithetic, control_variate, int(n_paths))
    rec, single = _records(parameters, spot, risk_free)
    _check_records(rec, steps_per_year)
    opts = _options(options, steps_per_year)
    if not flags:
        price, err = _native.default_context(device).mc_price(rec, opts, int(n_paths),
                                                              steps_per_year, seed)
        if single:
            price, err = price[0], err[0]
        return MonteCarloResult(price, err, int(n_paths), steps_per_year, seed)
    out = _native.default_context(device).mc_price_vr(rec, opts, int(n_paths), steps_per_year,
                                                      seed, flags)
    if single:
        out = tuple(a[0] for a in out)
    return VarianceReducedResult(out[0], out[1], int(n_paths), steps_per_year, seed, *out[2:],
                                 bool(antithetic), bool(control_variate))


@dataclass
class MonteCarloGreeks:
    """``monte_carlo_greeks``: the price, delta, gamma and the two v0 vegas (per unit of variance,
    as ``dhcos.greeks``) of every option, each with the standard error of its own paired samples:
    ``[n_options]`` for one parameter set, ``[P, n_options]`` for ``P``.  ``price`` and
    ``price_stderr`` are ``monte_carlo``'s bits.  delta and gamma are central differences in spot
    at the relative step ``spot_bump``, the vegas in ``v0_j`` at the relative step ``v0_bump``: of a
    barrier option they estimate the difference quotient at that step, not the derivative."""
    price: np.ndarray
    price_stderr: np.ndarray
    delta: np.ndarray
    delta_stderr: np.ndarray
    gamma: np.ndarray
    gamma_stderr: np.ndarray
    vega_v01: np.ndarray
    vega_v01_stderr: np.ndarray
    vega_v02: np.ndarray
    vega_v02_stderr: np.ndarray
    n_paths: int
    steps_per_year: int
    seed: int
    spot_bump: float
    v0_bump: float

    def confidence(self, z: float = 1.96):
        """{name: (low, high)} = value -+ z stderr of each of the five."""
        return {n: (getattr(self, n) - z * getattr(self, n + "_stderr"),
                    getattr(self, n) + z * getattr(self, n + "_stderr"))
                for n in _native.MC_GREEKS}


def _check_bump(name, v):
    v = float(v)
    if not 0.0 < v < 1.0:                # NaN and the infinities fail both comparisons' chain
        raise ValueError(f"{name}: a relative step inside (0, 1), got {v!r}")
    return v


def monte_carlo_greeks(parameters, spot, risk_free, options, *, n_paths=1 << 20,
                       steps_per_year=64, seed=0, spot_bump=1e-2, v0_bump=5e-2,
                       device=None) -> MonteCarloGreeks:
    """Price, delta, gamma and the two v0 vegas of ``options`` with their standard errors, from one
    walk of coupled paths on the GPU (dh_mc_greeks).

    parameters, spot, risk_free, options, n_paths, steps_per_year, seed: as ``monte_carlo``, whose
    price and standard error this call reproduces bit for bit.  spot_bump: the relative step
    ``eps`` of the central differences in spot (the paths at ``spot (1 +- eps)`` are the base paths
    scaled, no walk of their own); v0_bump: the relative step ``b`` of those in each ``v0_j`` (the
    paths from ``v0_j (1 +- b)`` share every random number, the other factor and the jumps with the
    base path); both inside (0, 1), and neither ``v0`` may be 0.  Antithetic pairs and the control
    variate of ``monte_carlo`` are not composed with the Greeks."""
    steps_per_year = _check_steps_per_year(steps_per_year)
    seed = _check_seed(seed)
    if int(n_paths) != n_paths or n_paths < 2:
        raise ValueError(f"n_paths: a whole number >= 2, got {n_paths!r}")
    spot_bump = _check_bump("spot_bump", spot_bump)
    v0_bump = _check_bump("v0_bump", v0_bump)
    rec, single = _records(parameters, spot, risk_free)
    _check_records(rec, steps_per_year)
    for k, name in ((0, "v1_0"), (5, "v2_0")):
        if not (rec[:, k] != 0.0).all():
            raise ValueError(f"{name} of set {int(np.argmin(rec[:, k] != 0.0))} is 0: its relative "
                             f"bump v0_bump would be empty")
    opts = _options(options, steps_per_year)
    value, err = _native.default_context(device).mc_greeks(rec, opts, int(n_paths), steps_per_year,
                                                           seed, spot_bump, v0_bump)
    if single:
        value, err = value[0], err[0]
    planes = []
    for g in range(len(_native.MC_GREEKS)):
        planes += [np.ascontiguousarray(value[..., g]), np.ascontiguousarray(err[..., g])]
    return MonteCarloGreeks(*planes, int(n_paths), steps_per_year, seed, spot_bump, v0_bump)


def simulate_paths(parameters, spot, risk_free, obs_steps, *, n_paths, path0=0, steps_per_year=64,
                   seed=0, device=None, mirror=False) -> np.ndarray:
    """dh_mc_paths: ``S, v1, v2, running max, running min, running sum`` of paths ``path0 ..
    path0 + n_paths - 1`` at the listed steps (>= 1, strictly increasing), by the pricing kernel's
    own step function -> ``[n_paths, n_obs, 6]``, or ``[P, n_paths, n_obs, 6]`` for ``[P, 13]``
    parameters.  mirror: the statistics of the paths' antithetic mirrors instead
    (dh_mc_paths_vr)."""
    steps_per_year = _check_steps_per_year(steps_per_year)
    seed = _check_seed(seed)
    if int(n_paths) != n_paths or n_paths < 1:
        raise ValueError(f"n_paths: a whole number >= 1, got {n_paths!r}")
    if int(path0) != path0 or path0 < 0 or path0 + n_paths >= 1 << 63:
        raise ValueError(f"path0: a whole number >= 0 with path0 + n_paths < 2^63, got {path0!r}")
    obs = np.asarray(obs_steps)
    if obs.ndim != 1 or obs.size < 1 or obs.dtype.kind not in "iu":
        raise ValueError("obs_steps: a non-empty 1-d sequence of whole numbers")
    if obs[0] < 1 or np.any(np.diff(obs.astype(np.int64)) <= 0) or obs[-1] > 2147483647:
        raise ValueError("obs_steps: step numbers >= 1, strictly increasing")
    rec, single = _records(parameters, spot, risk_free)
    _check_records(rec, steps_per_year)
    if rec.shape[0] * int(n_paths) * obs.size * 6 > 1 << 31:
        raise ValueError("simulate_paths: more than 2^31 doubles of output; ask for fewer paths "
                         "per call (path0 selects the range)")
    ctx = _native.default_context(device)
    if mirror:
        out = ctx.mc_paths_vr(rec, obs.astype(np.int32), int(path0), int(n_paths), steps_per_year,
                              seed, True)
    else:
        out = ctx.mc_paths(rec, obs.astype(np.int32), int(path0), int(n_paths), steps_per_year,
                           seed)
    return out[0] if single else out


__all__ = ["monte_carlo", "monte_carlo_greeks", "simulate_paths", "MonteCarloResult",
           "VarianceReducedResult", "MonteCarloGreeks", "KINDS", "MAX_OPTIONS"]
