"""NumPy restatement of the full Greeks' four further planes (include/dhcos.h) -- a
helper of tests/test_greeks_full_truth.py and tests/test_gpu_greeks_full.py, not a test.

Built on greeks_reference (whose six planes it returns unchanged) and oracle.dh_oracle.  With xK =
log(K / S0), [a, b] = trunc_range HELD, u_k = k pi / (b - a), w_k = phi(u_k) e^{-i u_k a} and V_k the
price's payoff coefficient:

    dprice_dT  = -r price + e^{-rT} sum'_k Re(w_k G_k) V_k
    rho        = -T price + e^{-rT} sum'_k Re(w_k i u_k T) V_k
    dual_gamma = e^{-rT} sum'_k Re(w_k) (2 / (b - a)) cos(u_k (xK - a)) / K
    local_var  = [dprice_dT + (r - q) K dual_delta + q price] / [1/2 K^2 dual_gamma]

G = d log phi / d tau = i (r - q - lambda comp) u + lambda (e^{i u mu - sj^2 u^2 / 2} - 1) +
sum_j (kappa_j theta_j B_j + v0_j B_j'), with B_j' = -2 u (u + i) d^2 e / D^2 (e = e^{-d tau},
D = (beta + d) - (beta - d) e): the derivative of the reference's B written without the cancellation
of the Riccati right side 1/2 sigma^2 B^2 - beta B - 1/2 (u^2 + i u), which it equals.
"""
import numpy as np

import greeks_reference as G6
from oracle import dh_oracle as O

NEW_PLANES = ("dprice_dT", "rho", "dual_gamma")          # the planes that are sums of a series
PLANES = G6.PLANES + NEW_PLANES + ("local_var",)
WRONG = ("dT_without_r_price", "rho_without_T_price", "dual_gamma_inverted")


def _b_prime(u, tau, kappa, sigma, rho):
    beta = kappa - rho * sigma * 1j * u
    dsq = beta ** 2 + sigma ** 2 * u * (u + 1j)
    d = np.sqrt(dsq)
    e = np.exp(-d * tau)
    D = (beta + d) - (beta - d) * e
    return -2.0 * (u * (u + 1j)) * dsq * e / (D * D)


def log_cf_dtau(u, tau, prm, r, q):
    """G(u) = d log phi / d tau."""
    v01, k1, t1, s1, r1, v02, k2, t2, s2, r2, lam, muj, sj = prm
    B1, _ = O._heston_factor(u, tau, k1, t1, s1, r1)
    B2, _ = O._heston_factor(u, tau, k2, t2, s2, r2)
    comp = np.exp(muj + 0.5 * sj ** 2) - 1
    g = (r - q - lam * comp) * 1j * u + lam * (np.exp(1j * u * muj - 0.5 * sj ** 2 * u ** 2) - 1)
    g = g + (k1 * t1 * B1 + v01 * _b_prime(u, tau, k1, s1, r1))
    return g + (k2 * t2 * B2 + v02 * _b_prime(u, tau, k2, s2, r2))


def _new_terms(prm, S0, K, T, r, is_call, N, q, L):
    """(e^{-rT}, {plane: its N series terms, halved at k = 0}) at the held range; dprice_dT's and
    rho's without their -r price, -T price."""
    xK = np.log(K / S0)
    a, b = O.trunc_range(prm, S0, K, T, r, L)
    k = np.arange(N, dtype=np.float64)
    u = k * np.pi / (b - a)
    with np.errstate(all="ignore"):
        w = O.cf(u, T, prm, r, q) * np.exp(-1j * u * a)
        c, d = (xK, b) if is_call else (a, xK)
        ed, ec = np.exp(d), np.exp(c)
        cd, cc = np.cos(u * (d - a)), np.cos(u * (c - a))
        sd, sc = np.sin(u * (d - a)), np.sin(u * (c - a))
        ch = (1.0 / (1 + u ** 2)) * (cd * ed - cc * ec + u * sd * ed - u * sc * ec)
        ps = (1.0 / u) * (sd - sc)
        ch[0] = ed - ec
        ps[0] = d - c
        scale = 2.0 / (b - a)
        V = scale * (S0 * ch - K * ps) if is_call else scale * (K * ps - S0 * ch)
        Vkk = scale * np.cos(u * (xK - a))

        def terms(weights, coef):
            t = np.real(weights) * coef
            t[0] *= 0.5
            return t

        return np.exp(-r * T), {
            "dprice_dT": terms(w * log_cf_dtau(u, T, prm, r, q), V),
            "rho": terms(w * (1j * u * T), V),
            "dual_gamma": terms(w, Vkk)}


def local_var_from_planes(dprice_dT, price, dual_delta, dual_gamma, K, r, q):
    """Dupire's quotient in the order csrc/dh_greeks_full.h documents (every operation rounded on its
    own), NaN where one of the four planes is not finite or the denominator is not > 0."""
    dT, price, dual, dgam, K, r, q = np.broadcast_arrays(
        *(np.asarray(x, dtype=np.float64) for x in (dprice_dT, price, dual_delta, dual_gamma, K,
                                                     r, q)))
    with np.errstate(all="ignore"):
        num = (dT + ((r - q) * K) * dual) + q * price
        den = (0.5 * (K * K)) * dgam
        ok = np.isfinite(dT) & np.isfinite(price) & np.isfinite(dual) & np.isfinite(dgam) & \
            (den > 0.0)
        return np.where(ok, num / np.where(ok, den, 1.0), np.nan)


def full_vec(prm, S0, K, T, r, is_call, N=128, q=0.0, L=10.0, wrong=None):
    """The ten planes of one option as a dict of floats.  wrong: one of WRONG, a deliberately wrong
    restatement that tests/test_greeks_full_truth.py must see refused."""
    assert wrong is None or wrong in WRONG
    out = G6.greeks_vec(prm, S0, K, T, r, is_call, N, q, L)
    disc, t = _new_terms(prm, S0, K, T, r, is_call, N, q, L)
    with np.errstate(all="ignore"):
        out["dprice_dT"] = disc * np.sum(t["dprice_dT"]) - \
            (0.0 if wrong == "dT_without_r_price" else r * out["price"])
        out["rho"] = disc * np.sum(t["rho"]) - \
            (0.0 if wrong == "rho_without_T_price" else T * out["price"])
        out["dual_gamma"] = disc * np.sum(t["dual_gamma"]) * (K if wrong == "dual_gamma_inverted"
                                                              else 1.0 / K)
    out["local_var"] = float(local_var_from_planes(out["dprice_dT"], out["price"],
                                                   out["dual_delta"], out["dual_gamma"], K, r, q))
    return out

