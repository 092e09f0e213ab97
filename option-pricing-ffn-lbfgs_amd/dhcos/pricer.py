"""Drop-in ``DoubleHeston`` whose arithmetic runs in the gfx950 kernels of libdhcos.so.

Mirrors the public surface of the reference class (src/models/double_heston.py:8-192):
same constructor signature and attributes, ``pricing(N=128)`` returning an ``np.float64``,
and ``characteristic_function`` / ``truncationRange`` / ``chi_k`` / ``psi_k`` still callable.
Every one of them is evaluated on the GPU through the C-ABI (include/dhcos.h); nothing here
computes a price on the CPU.  ``price_batch`` is the new batched entry point (one launch for any
number of (param set, option) pairs).
"""
from __future__ import annotations

import numpy as np

from . import _native

# constructor order of the 13 model parameters (double_heston.py:26-27)
MODEL_FIELDS = ("v01", "kappa1", "theta1", "sigma1", "rho1", "v02", "kappa2", "theta2",
                "sigma2", "rho2", "lambda_j", "mu_j", "sigma_j")


def resolve_call(option_type) -> bool:
    """Reference rule (double_heston.py:172): call iff option_type.upper()[0] == 'C'.
    Anything else is a put; '' raises IndexError exactly like the reference."""
    return option_type.upper()[0] == "C"


def param_record(model13, S0, r, q=0.0) -> np.ndarray:
    """Pack one DH_PARAM_STRIDE record: 13 model params, S0, r, q."""
    rec = np.empty(_native.PARAM_STRIDE)
    rec[:13] = model13
    rec[13], rec[14], rec[15] = S0, r, q
    return rec


def _is_call_array(option_type) -> np.ndarray:
    """price_batch's option_type rule: a string (reference rule), or a sequence / array of
    strings (reference rule each) or booleans (is_call) -> a bool array (0-d for a string)."""
    if isinstance(option_type, str):
        return np.array(resolve_call(option_type))
    ot = np.asarray(option_type)
    if ot.dtype.kind in "US":
        flat = [resolve_call(str(o)) for o in ot.reshape(-1)]
        return np.array(flat, dtype=bool).reshape(ot.shape)
    if ot.dtype.kind == "O":
        flat = [resolve_call(o) if isinstance(o, str) else bool(o) for o in ot.reshape(-1)]
        return np.array(flat, dtype=bool).reshape(ot.shape)
    return ot.astype(bool)


def _pair_args(params, S0, K, T, r, option_type, q):
    """price_batch's arguments as (records [n, 16], K [n], T [n], is_call [n]) of n pairs."""
    params = np.atleast_2d(np.asarray(params, dtype=np.float64))
    n = max(params.shape[0], np.size(K), np.size(T), np.size(S0))
    P = np.broadcast_to(params, (n, 13))
    rec = np.empty((n, _native.PARAM_STRIDE))
    rec[:, :13] = P
    rec[:, 13] = np.broadcast_to(np.asarray(S0, dtype=np.float64), (n,))
    rec[:, 14] = np.broadcast_to(np.asarray(r, dtype=np.float64), (n,))
    rec[:, 15] = np.broadcast_to(np.asarray(q, dtype=np.float64), (n,))
    if isinstance(option_type, str):
        ic = np.full(n, resolve_call(option_type))
    else:
        ot = list(option_type)
        ic = np.array([resolve_call(o) if isinstance(o, str) else bool(o) for o in ot])
        ic = np.broadcast_to(ic, (n,))
    Kb = np.broadcast_to(np.asarray(K, dtype=np.float64), (n,))
    Tb = np.broadcast_to(np.asarray(T, dtype=np.float64), (n,))
    return rec, Kb, Tb, ic


def implied_vol(price, S0, K, T, r, q=0.0, option_type="C", device=None):
    """Black-Scholes implied volatility on the GPU (dh_implied_vol): the sigma whose price of a
    European option (spot S0, strike K, maturity T, rate r, dividend yield q) is ``price``.

    All arguments broadcast (NumPy rules); option_type as in ``DoubleHeston.price_batch``.
    Returns an array of the broadcast shape, or an ``np.float64`` when every argument is a
    scalar.  0.0 where the price equals its lower bound; NaN where no volatility exists (price
    outside [lower, upper), non-finite or non-positive inputs) -- include/dhcos.h."""
    ic = _is_call_array(option_type)
    cols = [np.asarray(a, dtype=np.float64) for a in (price, S0, K, T, r, q)]
    shape = np.broadcast_shapes(ic.shape, *(c.shape for c in cols))
    flat = [np.ascontiguousarray(np.broadcast_to(c, shape)).reshape(-1) for c in cols]
    icf = np.ascontiguousarray(np.broadcast_to(ic, shape), dtype=np.int8).reshape(-1)
    out = _native.default_context(device).implied_vol(*flat, icf)
    return out.reshape(shape) if shape else np.float64(out[0])


class DoubleHeston:
    """Double Heston + lognormal (Merton) jumps, European call/put by the COS method."""

    def __init__(self, S0, K, T, r, v01, kappa1, theta1, sigma1, rho1,
                 v02, kappa2, theta2, sigma2, rho2, lambda_j, mu_j, sigma_j, option_type="C",
                 q=0.0, *, device=None):
        self.S0, self.K, self.T, self.r, self.q = S0, K, T, r, q
        self.v01, self.kappa1, self.theta1, self.sigma1, self.rho1 = v01, kappa1, theta1, sigma1, rho1
        self.v02, self.kappa2, self.theta2, self.sigma2, self.rho2 = v02, kappa2, theta2, sigma2, rho2
        self.option_type = option_type
        self.lambda_j, self.mu_j, self.sigma_j = lambda_j, mu_j, sigma_j
        self.device = device

    # -- helpers --------------------------------------------------------------------------
    def _ctx(self):
        return _native.default_context(self.device)

    def _record(self) -> np.ndarray:
        return param_record([getattr(self, f) for f in MODEL_FIELDS], self.S0, self.r, self.q)

    # -- reference API --------------------------------------------------------------------
    def characteristic_function(self, phi, tau):
        """phi(u; tau) for real or complex ``phi`` (scalar or array) -- double_heston.py:48-97.
        Real input takes the real-frequency kernel; complex input (any complex dtype, even with
        a zero imaginary part) the complex-frequency one, as the reference's complex arithmetic."""
        u = np.asarray(phi)
        if np.iscomplexobj(u):
            vals = self._ctx().cf_complex(self._record(), u.reshape(-1), tau)
        elif u.dtype.kind in "biuf":
            vals = self._ctx().cf(self._record(), u.astype(np.float64).reshape(-1), tau)
        else:
            raise TypeError(f"phi must be real or complex, got dtype {u.dtype}")
        return vals.reshape(u.shape) if u.ndim else np.complex128(vals[0])

    def truncationRange(self, L=10):
        """(a, b) -- double_heston.py:100-139 (c1 double-counts r*T, log-strike clamp)."""
        a, b = self._ctx().trunc_range(self._record()[None, :], [self.K], [self.T], L)
        return np.float64(a[0]), np.float64(b[0])

    def chi_k(self, k, c, d, a, b):
        """Cosine coefficient of e^y on [c, d] -- double_heston.py:141-151."""
        chi, _ = self._ctx().cos_coeffs([int(k)], c, d, a, b)
        return np.float64(chi[0])

    def psi_k(self, k, c, d, a, b):
        """Cosine coefficient of 1 on [c, d] -- double_heston.py:153-158."""
        _, psi = self._ctx().cos_coeffs([int(k)], c, d, a, b)
        return np.float64(psi[0])

    def pricing(self, N=128):
        """COS price with N terms -- double_heston.py:160-192."""
        is_call = resolve_call(self.option_type)
        return np.float64(self._ctx().price_one(self._record(), float(self.K), float(self.T),
                                                is_call, N))

    def implied_vol(self, N=128):
        """The Black-Scholes implied volatility of ``pricing(N)`` (NaN where the model price has
        none, e.g. below intrinsic)."""
        return implied_vol(self.pricing(N), self.S0, self.K, self.T, self.r, self.q,
                           self.option_type, device=self.device)

    def greeks(self, N=128):
        """``Greeks`` (price, delta, gamma, dual_delta, vega1, vega2) of this instance's option as
        scalars: the analytic partial derivatives of ``pricing(N)``'s COS series at a fixed
        truncation range and strike -- not through the cumulant range or its log-strike clamp
        (``dhcos.greeks``; the vegas are per unit of the variances v01, v02)."""
        from .greeks import Greeks, check_N
        out = self._ctx().greeks_pairs(self._record(), [float(self.K)], [float(self.T)],
                                       [resolve_call(self.option_type)], check_N(N))
        return Greeks.from_planes(out[:, 0])

    def greeks_full(self, N=128):
        """``FullGreeks`` of this instance's option as scalars: ``greeks(N)``'s six planes with the
        same bits, and dprice_dT, rho, dual_gamma and Dupire's local_var (with theta, epsilon,
        density and local_vol derived from them), partial derivatives at a fixed truncation range
        (``dhcos.greeks_full``)."""
        from .greeks import check_N
        from .greeks_full import FullGreeks
        out = self._ctx().greeks_full_pairs(self._record(), [float(self.K)], [float(self.T)],
                                            [resolve_call(self.option_type)], check_N(N))
        return FullGreeks.from_planes(out[:, 0], np.float64(self.T), np.float64(self.r))

    def parameter_sensitivities(self, N=128):
        """``ParameterSensitivities`` (the price and d price / d each of the 13 model parameters) of
        this instance's option as scalars: analytic partial derivatives of ``pricing(N)``'s COS
        series at a fixed truncation range (``dhcos.parameter_sensitivities``; N <= 1024)."""
        from .param_sens import ParameterSensitivities, check_N
        out = self._ctx().param_sens_pairs(self._record(), [float(self.K)], [float(self.T)],
                                           [resolve_call(self.option_type)], check_N(N))
        return ParameterSensitivities.from_planes(out[:, 0])

    def monte_carlo(self, n_paths=1 << 20, steps_per_year=64, seed=0, antithetic=False,
                    control_variate=False):
        """(price, stderr) of this instance's option by simulating the model's SDE
        (``dhcos.monte_carlo``; q must be 0, the simulated dynamics carry no dividend yield).
        antithetic, control_variate: the variance reduction of ``dhcos.monte_carlo`` (the control
        of a European option is its discounted terminal spot)."""
        from .montecarlo import monte_carlo
        if self.q != 0.0:
            raise ValueError("monte_carlo: the simulated dynamics have q = 0")
        res = monte_carlo([getattr(self, f) for f in MODEL_FIELDS], self.S0, self.r,
                          [{"strike": self.K, "maturity": self.T,
                            "option_type": self.option_type}],
                          n_paths=n_paths, steps_per_year=steps_per_year, seed=seed,
                          device=self.device, antithetic=antithetic,
                          control_variate=control_variate)
        return np.float64(res.price[0]), np.float64(res.stderr[0])

    def monte_carlo_greeks(self, n_paths=1 << 20, steps_per_year=64, seed=0, spot_bump=1e-2,
                           v0_bump=5e-2):
        """``MonteCarloGreeks`` (price, delta, gamma and the v0 vegas, each with its standard
        error) of this instance's option as scalars, from one walk of coupled paths
        (``dhcos.monte_carlo_greeks``; q must be 0, the simulated dynamics carry no dividend
        yield)."""
        from .montecarlo import monte_carlo_greeks
        if self.q != 0.0:
            raise ValueError("monte_carlo_greeks: the simulated dynamics have q = 0")
        res = monte_carlo_greeks([getattr(self, f) for f in MODEL_FIELDS], self.S0, self.r,
                                 [{"strike": self.K, "maturity": self.T,
                                   "option_type": self.option_type}],
                                 n_paths=n_paths, steps_per_year=steps_per_year, seed=seed,
                                 spot_bump=spot_bump, v0_bump=v0_bump, device=self.device)
        for name in _native.MC_GREEKS:
            for field in (name, name + "_stderr"):
                setattr(res, field, np.float64(getattr(res, field)[0]))
        return res

    def american_monte_carlo(self, n_paths=1 << 17, steps_per_year=64, exercise_every=1, seed=0):
        """(price, stderr) of this instance's option with early exercise at every
        ``exercise_every``-th step, by least-squares Monte Carlo (``dhcos.american_monte_carlo``;
        q must be 0, the simulated dynamics carry no dividend yield)."""
        from .american import american_monte_carlo
        if self.q != 0.0:
            raise ValueError("american_monte_carlo: the simulated dynamics have q = 0")
        res = american_monte_carlo([getattr(self, f) for f in MODEL_FIELDS], self.S0, self.r,
                                   [{"strike": self.K, "maturity": self.T,
                                     "option_type": self.option_type}],
                                   n_paths=n_paths, steps_per_year=steps_per_year,
                                   exercise_every=exercise_every, seed=seed, device=self.device)
        return np.float64(res.price[0]), np.float64(res.stderr[0])

    # -- batched entry point ----------------------------------------------------------------
    @staticmethod
    def price_batch(params, S0, K, T, r, option_type="C", N=128, q=0.0, L=10.0, device=None):
        """Price option i under param set i, all in one launch.

        params: [n, 13] model parameters (constructor order); S0, K, T, r, q broadcast to n;
        option_type: a string or a sequence of n strings (reference rule) or booleans (is_call).
        """
        rec, Kb, Tb, ic = _pair_args(params, S0, K, T, r, option_type, q)
        return _native.default_context(device).price_pairs(rec, Kb, Tb, ic, N, L)

    @staticmethod
    def greeks_batch(params, S0, K, T, r, option_type="C", N=128, q=0.0, L=10.0, device=None):
        """``price_batch``'s arguments -> ``Greeks`` of ``[n]`` arrays: price, delta, gamma,
        dual_delta, vega1, vega2 of option i under param set i, all in one launch.  Partial
        derivatives of the COS series at a fixed truncation range and strike (``dhcos.greeks``)."""
        from .greeks import Greeks, check_L, check_N
        N, L = check_N(N), check_L(L)
        rec, Kb, Tb, ic = _pair_args(params, S0, K, T, r, option_type, q)
        return Greeks.from_planes(
            _native.default_context(device).greeks_pairs(rec, Kb, Tb, ic, N, L))

    @staticmethod
    def greeks_full_batch(params, S0, K, T, r, option_type="C", N=128, q=0.0, L=10.0,
                          device=None):
        """``price_batch``'s arguments -> ``FullGreeks`` of ``[n]`` arrays: the ten planes of option
        i under param set i, all in one launch (``dhcos.greeks_full``)."""
        from .greeks import check_L, check_N
        from .greeks_full import FullGreeks
        N, L = check_N(N), check_L(L)
        rec, Kb, Tb, ic = _pair_args(params, S0, K, T, r, option_type, q)
        return FullGreeks.from_planes(
            _native.default_context(device).greeks_full_pairs(rec, Kb, Tb, ic, N, L), Tb,
            rec[:, 14].copy())

    @staticmethod
    def implied_vol_batch(params, S0, K, T, r, option_type="C", N=128, q=0.0, L=10.0,
                          device=None):
        """``price_batch``'s arguments -> the Black-Scholes implied vols of its prices (option i
        under param set i; the prices stay price_batch's bits)."""
        prices = DoubleHeston.price_batch(params, S0, K, T, r, option_type, N, q, L, device)
        n = prices.size
        bc = [np.broadcast_to(np.asarray(a, dtype=np.float64), (n,)) for a in (S0, K, T, r, q)]
        ic = _is_call_array(option_type)
        return implied_vol(prices, *bc, option_type=np.broadcast_to(ic, (n,)), device=device)
