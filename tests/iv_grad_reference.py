"""NumPy restatement of the implied-vol objective and its exact gradient (dh_surface_iv_grad_rows_dev,
dh_surface_loss_iv_grad_rows) -- a helper of tests/test_iv_grad.py and
tests/test_gpu_iv_grad.py, not a test.

tests/param_grad_reference.sens_vec's planes, the Black-Scholes vega in the inverter's variables

    A = S0 e^{-qT}, B = K e^{-rT}, s = v sqrt T, h = |log1p((S0 - K) / K) + (r - q) T| / s, t = s / 2
    vega = sqrt A sqrt B sqrt T exp(-(h^2 + t^2) / 2 - ln sqrt(2 pi))

and the reduction's rules and order: a price that is NaN, infinite or <= 0 has no vol and is bad
where its weight is positive; a price below its lower bound is clamped to the vol 0.0; a zero
weight enters nothing; a used option adds w (v - mkt)^2 to sse and, unless its vol is 0.0 or its
vega is not > 0, c = w (v - mkt) / vega times each parameter plane to the gradient sums.  Lane l of
64 takes the options sorted by maturity (stable) l, l + 64, ... from 0.0; then the xor butterfly
1, 2, 4, 8, 16, 32.  f = n_bad ? 1e10 : sse / sum(w) + Feller; g_i = n_bad ? 0 : (2 / sum(w))
sum_i dtheta_i/dx_i + dFeller/dx_i (param_grad_reference's transform and Feller expressions).

The vols are the caller's (the device's own vols as used, in the GPU tests) or SciPy brentq's."""
import numpy as np
from scipy.optimize import brentq
from scipy.special import ndtr

import param_grad_reference as R
from oracle import dh_oracle as O

LN_SQRT_2PI = 0.9189385332046728


def vega(v, S0, K, T, r, q=0.0):
    """Black-Scholes d price / d vol (a call's and a put's) in the inverter's variables."""
    with np.errstate(all="ignore"):
        A, B = S0 * np.exp(-q * T), K * np.exp(-r * T)
        s = v * np.sqrt(T)
        h = np.abs(np.log1p((S0 - K) / K) + (r - q) * T) / s
        t = 0.5 * s
        return np.sqrt(A) * np.sqrt(B) * np.sqrt(T) * np.exp(-0.5 * (h * h + t * t) - LN_SQRT_2PI)


def bs_price(v, S0, K, T, r, is_call, q=0.0):
    A, B = S0 * np.exp(-q * T), K * np.exp(-r * T)
    s = v * np.sqrt(T)
    d1 = np.log(A / B) / s + 0.5 * s
    call = A * ndtr(d1) - B * ndtr(d1 - s)
    return call if is_call else call - A + B


def lower_bound(S0, K, T, r, is_call, q=0.0):
    A, B = S0 * np.exp(-q * T), K * np.exp(-r * T)
    return max(A - B, 0.0) if is_call else max(B - A, 0.0)


def vol_as_used(price, S0, K, T, r, is_call, q=0.0):
    """The vol the reduction uses for one price, by brentq: NaN for a bad price (NaN, infinite,
    <= 0) or one at or above its upper bound, 0.0 at or below its lower bound."""
    if not (np.isfinite(price) and price > 0.0):
        return np.nan
    A, B = S0 * np.exp(-q * T), K * np.exp(-r * T)
    if price <= lower_bound(S0, K, T, r, is_call, q):
        return 0.0
    if price >= (A if is_call else B):
        return np.nan
    return brentq(lambda v: bs_price(v, S0, K, T, r, is_call, q) - price, 1e-8, 20.0,
                  xtol=1e-16, rtol=8.9e-16, maxiter=200)


def vols_as_used(prices, S0, K, T, r, call, q=0.0):
    return np.array([vol_as_used(p, S0, k, t, r, bool(c), q)
                     for p, k, t, c in zip(prices, K, T, call)])


def _wave_sum(terms, order):
    """terms [M, ...] summed in the reduction's order: lane l adds the sorted options l, l + 64,
    ... from 0.0, then the xor butterfly."""
    acc = np.zeros((64,) + terms.shape[1:])
    for i, c in enumerate(order):
        acc[i % 64] = acc[i % 64] + terms[c]
    lane = np.arange(64)
    for off in (1, 2, 4, 8, 16, 32):
        acc = acc + acc[lane ^ off]
    return acc[0]


def reduce_planes(planes, p, iv, mkt_iv, w, S0, K, T, r, q=0.0):
    """The reduction of one set: planes [14, M] (plane 0 the price), p the 13 model parameters, iv
    [M] the vols as used (NaN: none), mkt_iv / w [M], absolute strikes K [M]
    -> (f, g [13], sse, n_bad)."""
    planes = np.asarray(planes, dtype=np.float64)
    M = planes.shape[1]
    order = np.argsort(T, kind="stable")                 # sorted place -> caller's place
    used = w > 0
    bad = used & np.isnan(iv)
    live = used & ~bad
    with np.errstate(all="ignore"):
        d = np.where(live, iv - mkt_iv, 0.0)
        term = np.where(live, w * (d * d), 0.0)
        vg = vega(iv, S0, K, T, r, q)
        moves = live & (iv != 0.0) & (vg > 0.0)
        c = np.where(moves, (w * d) / np.where(moves, vg, 1.0), 0.0)
        contrib = np.where((c != 0.0)[:, None], c[:, None] * planes[1:].T, 0.0)     # [M, 13]
    sse = float(_wave_sum(term, order))
    n_bad = int(bad.sum())
    if n_bad:
        return O.INVALID_LOSS, np.zeros(13), sse, n_bad
    wsum = 0.0
    for m in range(M):                                   # option order, sequential, from 0.0
        wsum += w[m]
    f = sse / wsum + O.feller(p)
    g = (2.0 / wsum) * _wave_sum(contrib, order) * R.dtheta_dx(p) + R.feller_grad_x(p)
    return f, g, sse, n_bad


def planes_of(p, S0, K, T, r, call, N=128):
    """param_grad_reference.sens_vec for every option -> [14, M]."""
    return np.array([R.sens_vec(p, S0, k, t, r, bool(c), N) for k, t, c in zip(K, T, call)]).T


def loss_grad(x, K, T, call, mkt_iv, w, S0, r, N=128, iv=None):
    """(f, g [13], iv [M] as used) of the vol objective at the unconstrained x against one market:
    absolute strikes K [M], maturities T [M], flags, vols and weights.  iv: the vols to use (the
    device's own), default brentq's of the restated prices."""
    p = O.to_params(np.asarray(x, dtype=np.float64))
    planes = planes_of(p, S0, K, T, r, call, N)
    if iv is None:
        iv = vols_as_used(planes[0], S0, K, T, r, call)
    f, g, _, _ = reduce_planes(planes, p, iv, mkt_iv, w, S0, K, T, r)
    return f, g, iv


def loss(x, K, T, call, mkt_iv, w, S0, r, N=128):
    """The vol objective alone (O.price_vec prices, brentq vols): what loss_grad differentiates."""
    p = O.to_params(np.asarray(x, dtype=np.float64))
    prices = np.array([O.price_vec(p, S0, k, t, r, bool(c), N) for k, t, c in zip(K, T, call)])
    iv = vols_as_used(prices, S0, K, T, r, call)
    used = w > 0
    if np.any(used & np.isnan(iv)):
        return O.INVALID_LOSS
    return float(np.sum(w[used] * (iv[used] - mkt_iv[used]) ** 2) / np.sum(w)) + O.feller(p)
