"""American and Bermudan options under the Double-Heston + Merton-jump model by least-squares
Monte Carlo (dh_lsm_price, csrc/dh_lsm.h).

``american_monte_carlo`` takes the parameters ``monte_carlo`` takes and prices vanilla calls and
puts with early exercise at the steps ``exercise_every, 2 exercise_every, ...`` of the path grid
(every step: the discrete stand-in for an American option; fewer: a Bermudan; the start value is not
a date), all from one set of simulated paths on the GPU; DESIGN.md 3.15.1 is the scheme.  The same
paths fit and value the exercise policy, so the price carries LSM's in-sample bias.  Every argument
the native library refuses is refused here first, with ``ValueError`` and before the library is
loaded.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _native
from .montecarlo import (_check_records, _check_seed, _check_steps_per_year, _maturity_step,
                         _records)
from .pricer import resolve_call

MAX_OPTIONS = _native.LSM_MAX_OPTIONS
MAX_BYTES = _native.LSM_MAX_GIB << 30    # cap of the path store


@dataclass
class AmericanMonteCarloResult:
    """Prices with early exercise, the European values of the same paths and their standard errors:
    ``[n_options]`` for one parameter set, ``[P, n_options]`` for ``P``.  With ``policy=True`` also
    ``coefficients`` ``[..., n_options, dates, 10]`` (row ``d - 1``: the regression coefficients
    used at date ``d``; NaN where the date was skipped, at the option's maturity date and past it)
    and ``exercise_date`` ``[..., n_options, n_paths]`` (the date ``1 .. D_j`` of each path's
    cashflow).  The rest echoes the call."""
    price: np.ndarray
    stderr: np.ndarray
    european: np.ndarray
    european_stderr: np.ndarray
    coefficients: np.ndarray | None
    exercise_date: np.ndarray | None
    n_paths: int
    steps_per_year: int
    exercise_every: int
    seed: int

    @property
    def premium(self):
        """The early-exercise premium, price - european (same paths: most of the noise cancels)."""
        return self.price - self.european

    def confidence(self, z: float = 1.96):
        """(low, high) = price -+ z stderr."""
        return self.price - z * self.stderr, self.price + z * self.stderr


def _options(options, steps_per_year, exercise_every):
    """The reference's option dicts (strike, maturity, option_type) -> (an array of
    dh_lsm_option, the largest number of exercise dates)."""
    options = list(options)
    if not 1 <= len(options) <= MAX_OPTIONS:
        raise ValueError(f"options: 1 to {MAX_OPTIONS} per call, got {len(options)}")
    arr = (_native.LsmOption * len(options))()
    dates = 0
    for j, o in enumerate(options):
        strike, T = float(o["strike"]), float(o["maturity"])
        if not np.isfinite(strike) or strike < 0.0:
            raise ValueError(f"options[{j}]: strike must be finite and >= 0, got {strike}")
        n = _maturity_step(j, T, steps_per_year)
        if n % exercise_every:
            raise ValueError(f"options[{j}]: maturity {T} (step {n}) is not a whole multiple "
                             f"of exercise_every = {exercise_every}")
        dates = max(dates, n // exercise_every)
        arr[j] = _native.LsmOption(int(resolve_call(o["option_type"])), 0, strike, T)
    return arr, dates


def american_monte_carlo(parameters, spot, risk_free, options, *, n_paths=1 << 17,
                         steps_per_year=64, exercise_every=1, seed=0, policy=False,
                         device=None) -> AmericanMonteCarloResult:
    """Price ``options`` with early exercise by least-squares Monte Carlo on the GPU.

    parameters, spot, risk_free: as ``monte_carlo``; options: the reference's list of dicts
    (``strike``, ``maturity``, ``option_type``), at most 16.  The exercise dates are the steps
    ``exercise_every, 2 exercise_every, ...`` of the grid of ``1 / steps_per_year`` (time 0 is not
    one); every maturity must be a whole number of steps and a whole multiple of
    ``exercise_every``.  ``policy=True`` also returns the regression coefficients of every date
    and every path's exercise date.  All parameter sets see the same random numbers, and the same
    call gives the same bits."""
    steps_per_year = _check_steps_per_year(steps_per_year)
    seed = _check_seed(seed)
    if int(n_paths) != n_paths or n_paths < 2:
        raise ValueError(f"n_paths: a whole number >= 2, got {n_paths!r}")
    if int(exercise_every) != exercise_every or exercise_every < 1:
        raise ValueError(f"exercise_every: a whole number >= 1, got {exercise_every!r}")
    n_paths, exercise_every = int(n_paths), int(exercise_every)
    rec, single = _records(parameters, spot, risk_free)
    _check_records(rec, steps_per_year)
    opts, dates = _options(options, steps_per_year, exercise_every)
    if rec.shape[0] * n_paths * (24 * dates + 12 * len(opts)) > MAX_BYTES:
        raise ValueError(f"n_paths: the path store of P x n_paths x (24 dates + 12 n_options) "
                         f"bytes exceeds the cap of {_native.LSM_MAX_GIB} GiB: fewer paths or "
                         "parameter sets per call")
    out = _native.default_context(device).lsm_price(rec, opts, dates, n_paths, steps_per_year,
                                                    exercise_every, seed, policy=bool(policy))
    if single:
        out = [None if o is None else o[0] for o in out]
    return AmericanMonteCarloResult(*out, n_paths, steps_per_year, exercise_every, seed)


__all__ = ["american_monte_carlo", "AmericanMonteCarloResult", "MAX_OPTIONS", "MAX_BYTES"]
