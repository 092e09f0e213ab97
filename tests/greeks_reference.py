"""NumPy restatement of the analytic COS Greeks (include/dhcos.h) -- a helper of
tests/test_greeks*.py and tests/test_gpu_greeks*.py, not a test.

Built on oracle.dh_oracle (cf, _heston_factor, trunc_range) and written in price_vec's operation
order, so that its price plane IS price_vec, bit for bit.  With xK = log(K / S0), [a, b] =
trunc_range, u_k = k pi / (b - a), w_k = phi(u_k) e^{-i u_k a}:

    price      = e^{-rT} sum'_k Re(w_k) V_k,   V_k = +-(2 / (b - a)) (S0 chi_k - K psi_k)
    delta      : V_k -> +-(2 / (b - a)) chi_k
    gamma      : V_k -> (2 / (b - a)) cos(u_k (xK - a)) K / S0^2
    dual_delta : V_k -> -+(2 / (b - a)) psi_k
    vega1, 2   : w_k -> w_k B_j(u_k)

partial derivatives at fixed [a, b] and fixed strike (not through the cumulant range or its clamp).
"""
import numpy as np

from oracle import dh_oracle as O

PLANES = ("price", "delta", "gamma", "dual_delta", "vega1", "vega2")


def clamp_active(prm, S0, K, T, r, L=10.0):
    """True where the log-strike clamp widens the cumulant range (double_heston.py:131-137)."""
    a, b = O.trunc_range(prm, S0, K, T, r, L)          # min(a0, x - 0.1), max(b0, x + 0.1)
    x = np.log(K / S0)
    return bool(a == x - 0.1 or b == x + 0.1)


def unclamped_range(prm, T, r, L=10.0):
    """The cumulant range (a0, b0) before the log-strike clamp, in trunc_range's arithmetic."""
    v01, k1, t1, s1, r1, v02, k2, t2, s2, r2, lam, muj, sj = prm
    c1a, c2a = O._factor_cumulants(T, r, v01, k1, t1, s1, r1)
    c1b, c2b = O._factor_cumulants(T, r, v02, k2, t2, s2, r2)
    c1 = c1a + c1b + lam * T * muj
    c2 = c2a + c2b + lam * T * (sj ** 2 + muj ** 2)
    half = L * np.sqrt(np.abs(c2))
    return c1 - half, c1 + half


def _plane_terms(prm, S0, K, T, r, is_call, N, q, L):
    """(e^{-rT}, {plane: its N terms, halved at k = 0}) in price_vec's operation order."""
    v01, k1, t1, s1, r1, v02, k2, t2, s2, r2, lam, muj, sj = prm
    xK = np.log(K / S0)
    a, b = O.trunc_range(prm, S0, K, T, r, L)
    k = np.arange(N, dtype=np.float64)
    u = k * np.pi / (b - a)
    with np.errstate(all="ignore"):
        phi = O.cf(u, T, prm, r, q)
        B1, _ = O._heston_factor(u, T, k1, t1, s1, r1)
        B2, _ = O._heston_factor(u, T, k2, t2, s2, r2)
        c, d = (xK, b) if is_call else (a, xK)
        ed, ec = np.exp(d), np.exp(c)
        cd, cc = np.cos(u * (d - a)), np.cos(u * (c - a))
        sd, sc = np.sin(u * (d - a)), np.sin(u * (c - a))
        ch = (1.0 / (1 + u ** 2)) * (cd * ed - cc * ec + u * sd * ed - u * sc * ec)
        ps = (1.0 / u) * (sd - sc)
        ch[0] = ed - ec
        ps[0] = d - c
        scale = 2.0 / (b - a)
        if is_call:
            V = scale * (S0 * ch - K * ps)
            Vd, Vk = scale * ch, -(scale * ps)
        else:
            V = scale * (K * ps - S0 * ch)
            Vd, Vk = -(scale * ch), scale * ps
        Vg = scale * np.cos(u * (xK - a)) * K / S0 ** 2
        w = phi * np.exp(-1j * u * a)
        disc = np.exp(-r * T)

        def terms(weights, coef):
            t = np.real(weights) * coef
            t[0] *= 0.5
            return t

        return disc, {"price": terms(w, V), "delta": terms(w, Vd), "gamma": terms(w, Vg),
                      "dual_delta": terms(w, Vk), "vega1": terms(w * B1, V),
                      "vega2": terms(w * B2, V)}


def greeks_vec(prm, S0, K, T, r, is_call, N=128, q=0.0, L=10.0):
    """The six planes of one option as a dict of floats; 'price' equals O.price_vec bit for bit."""
    disc, terms = _plane_terms(prm, S0, K, T, r, is_call, N, q, L)
    with np.errstate(all="ignore"):
        return {name: disc * np.sum(t) for name, t in terms.items()}


def term_sums(prm, S0, K, T, r, is_call, N=128, q=0.0, L=10.0):
    """e^{-rT} sum_k |term_k| per plane, in fp64: the series' absolute term sum, the unit in which
    tests/test_greeks_truth.py and tests/test_gpu_greeks_truth.py state their bars."""
    disc, terms = _plane_terms(prm, S0, K, T, r, is_call, N, q, L)
    return {name: disc * np.sum(np.abs(t)) for name, t in terms.items()}


def greeks_surface(records, K, T, is_call, N=128, L=10.0, pct_spot=False):
    """greeks_vec for every (record [P, 16], option [M]) -> [6, P, M] in PLANES' order.  pct_spot:
    K holds strikes in percent of each record's spot (DH_STRIKE_PCT_SPOT): K_rel * S0 / 100.0."""
    records = np.atleast_2d(np.asarray(records, dtype=np.float64))
    K, T = np.asarray(K, dtype=np.float64), np.asarray(T, dtype=np.float64)
    call = np.broadcast_to(np.asarray(is_call, dtype=bool), K.shape)
    out = np.empty((len(PLANES), records.shape[0], K.size))
    for p, rec in enumerate(records):
        S0, r, q = rec[13], rec[14], rec[15]
        for m in range(K.size):
            strike = K[m] * S0 / 100.0 if pct_spot else K[m]
            g = greeks_vec(rec[:13], S0, strike, T[m], r, bool(call[m]), N, q, L)
            out[:, p, m] = [g[n] for n in PLANES]
    return out
