"""NumPy restatement of the analytic parameter sensitivities of the COS price and of the loss
gradient built on them (include/dhcos.h) -- a helper of tests/test_param_grad.py
and tests/test_gpu_param_grad.py, not a test.

Built on oracle.dh_oracle (cf, _heston_factor, trunc_range) and written in price_vec's operation
order, so that its price plane IS price_vec and its v0 planes ARE greeks_reference's vegas, bit for
bit.  With xK = log(K / S0), [a, b] = trunc_range, u_k = k pi / (b - a), w_k = phi(u_k) e^{-i u_k a}:

    price        = e^{-rT} sum'_k Re(w_k) V_k
    d price / dp = e^{-rT} sum'_k Re(w_k D_p(u_k)) V_k,   D_p = d log phi / d p

partial derivatives at fixed [a, b] (not through the cumulant range or its clamp).  Per factor, with
beta = kappa - i rho sigma u, uu = u (u + i), d = sqrt(beta^2 + sigma^2 uu), bm = beta - d, bp =
beta + d, e = e^{-d tau}, D = bp - bm e, c = kappa theta / sigma^2:

    d/dv0 = B (the factor's B as _heston_factor forms it)
    d/dtheta = (kappa / sigma^2) (bm tau - 2 log(D / (2 d)))
    p in {kappa, sigma, rho} from (beta', (d^2)', c'): d' = (d^2)' / (2 d), bm' = beta' - d', bp' =
    beta' + d', e' = -tau d' e, D' = bp' - bm' e - bm e', B' = -uu (-e' D - (1 - e) D') / D^2,
    A' = c' (bm tau - 2 log(D / (2 d))) + c (bm' tau - 2 (D' / D - d' / d)), d/dp = A' + B' v0

and for the jumps, J = e^{i u mu_j - sigma_j^2 u^2 / 2}, m = e^{mu_j + sigma_j^2 / 2}:

    d/dlambda = tau (J - 1) - i u tau (m - 1),  d/dmu_j = lambda tau i u J - i u tau lambda m,
    d/dsigma_j = -lambda tau sigma_j u^2 J - i u tau lambda sigma_j m.
"""
import numpy as np

from oracle import dh_oracle as O

PLANES = ("price",) + tuple(O.PARAM_NAMES)


def factor_derivs(u, tau, v0, kappa, theta, sigma, rho):
    """(D_v0, D_kappa, D_theta, D_sigma, D_rho) of one factor at the frequencies u."""
    B, _ = O._heston_factor(u, tau, kappa, theta, sigma, rho)
    beta = kappa - rho * sigma * 1j * u
    uu = u * (u + 1j)
    d = np.sqrt(beta ** 2 + sigma ** 2 * uu)
    bm, bp = beta - d, beta + d
    e = np.exp(-d * tau)
    D = bp - bm * e
    c = kappa * theta / sigma ** 2
    inner = bm * tau - 2 * np.log(D / (2 * d))

    def chain(bq, d2q, cq):
        dq = d2q / (2 * d)
        bmq, bpq = bq - dq, bq + dq
        eq = -tau * dq * e
        Dq = bpq - bmq * e - bm * eq
        Bq = -uu * (-eq * D - (1 - e) * Dq) / D ** 2
        Aq = cq * inner + c * (bmq * tau - 2 * (Dq / D - dq / d))
        return Aq + Bq * v0

    d_kappa = chain(1.0, 2 * beta, theta / sigma ** 2)
    d_sigma = chain(-1j * rho * u, 2 * beta * (-1j * rho * u) + 2 * sigma * uu,
                    -2 * kappa * theta / sigma ** 3)
    d_rho = chain(-1j * sigma * u, 2 * beta * (-1j * sigma * u), 0.0)
    return B, d_kappa, (kappa / sigma ** 2) * inner, d_sigma, d_rho


def log_cf_derivs(u, tau, prm):
    """The thirteen D_p(u) in PARAM_NAMES' order."""
    v01, k1, t1, s1, r1, v02, k2, t2, s2, r2, lam, muj, sj = prm
    J = np.exp(1j * u * muj - 0.5 * sj ** 2 * u ** 2)
    m = np.exp(muj + 0.5 * sj ** 2)
    d_lam = tau * (J - 1) - 1j * u * tau * (m - 1)
    d_mu = lam * tau * 1j * u * J - 1j * u * tau * lam * m
    d_sj = -lam * tau * sj * u ** 2 * J - 1j * u * tau * lam * sj * m
    return (*factor_derivs(u, tau, v01, k1, t1, s1, r1),
            *factor_derivs(u, tau, v02, k2, t2, s2, r2), d_lam, d_mu, d_sj)


PI_EXTENDED = np.longdouble(np.pi) + np.longdouble(1.2246467991473532e-16)   # pi - fp64(pi)


def sens_vec(prm, S0, K, T, r, is_call, N=128, q=0.0, L=10.0, ab=None, extended=False):
    """The fourteen planes of one option as an array [14]; [0] equals O.price_vec bit for bit.
    ab: the range to hold (default O.trunc_range's).  extended: the same expressions on the same
    fp64 inputs and the same fp64 [a, b], evaluated in np.longdouble (x87: 64-bit significand,
    eps 1.1e-19) -- the higher-precision evaluation the clamp test measures fp64 rounding against;
    the result is rounded to fp64 at the end."""
    a, b = O.trunc_range(prm, S0, K, T, r, L) if ab is None else ab
    pi = np.pi
    if extended:
        ld = np.longdouble
        prm, S0, K, T, r, q, a, b = [ld(v) for v in prm], ld(S0), ld(K), ld(T), ld(r), ld(q), \
            ld(a), ld(b)
        pi = PI_EXTENDED
    xK = np.log(K / S0)
    k = np.arange(N, dtype=np.longdouble if extended else np.float64)
    u = k * pi / (b - a)
    with np.errstate(all="ignore"):
        phi = O.cf(u, T, prm, r, q)
        Ds = log_cf_derivs(u, T, prm)
        c, d = (xK, b) if is_call else (a, xK)
        ed, ec = np.exp(d), np.exp(c)
        cd, cc = np.cos(u * (d - a)), np.cos(u * (c - a))
        sd, sc = np.sin(u * (d - a)), np.sin(u * (c - a))
        ch = (1.0 / (1 + u ** 2)) * (cd * ed - cc * ec + u * sd * ed - u * sc * ec)
        ps = (1.0 / u) * (sd - sc)
        ch[0] = ed - ec
        ps[0] = d - c
        if is_call:
            V = (2.0 / (b - a)) * (S0 * ch - K * ps)
        else:
            V = (2.0 / (b - a)) * (K * ps - S0 * ch)
        w = phi * np.exp(-1j * u * a)
        disc = np.exp(-r * T)

        def series(weights):
            terms = np.real(weights) * V
            terms[0] *= 0.5
            return disc * np.sum(terms)

        return np.array([series(w)] + [series(w * D) for D in Ds], dtype=np.float64)


def sens_surface(records, K, T, is_call, N=128, L=10.0, extended=False):
    """sens_vec for every (record [P, 16], option [M]) -> [14, P, M] in PLANES' order."""
    records = np.atleast_2d(np.asarray(records, dtype=np.float64))
    K, T = np.asarray(K, dtype=np.float64), np.asarray(T, dtype=np.float64)
    call = np.broadcast_to(np.asarray(is_call, dtype=bool), K.shape)
    out = np.empty((len(PLANES), records.shape[0], K.size))
    for p, rec in enumerate(records):
        for m in range(K.size):
            out[:, p, m] = sens_vec(rec[:13], rec[13], K[m], T[m], rec[14], bool(call[m]), N,
                                    rec[15], L, extended=extended)
    return out


def dtheta_dx(p):
    """d (model parameter) / d x of O.to_params: theta (exp), 1 - rho^2 (tanh), 1 (mu_j)."""
    p = np.asarray(p, dtype=np.float64)
    d = p.copy()
    d[list(O._TANH_IDX)] = 1.0 - p[list(O._TANH_IDX)] ** 2
    d[11] = 1.0
    return d


def feller_grad_x(p):
    """Gradient in x of O.feller where a factor's slack sigma^2 - 2 kappa theta is strictly
    positive, zero otherwise: +2000 sigma^2 (sigma), -2000 kappa theta (kappa and theta each)."""
    g = np.zeros(13)
    for o in (0, 5):
        kap, th, sig = p[o + 1], p[o + 2], p[o + 3]
        if sig ** 2 - 2 * kap * th > 0:
            g[o + 3] += 2000.0 * sig ** 2
            g[o + 1] -= 2000.0 * kap * th
            g[o + 2] -= 2000.0 * kap * th
    return g


def loss_grad(x, market, spot, r, N=128):
    """(loss, gradient [13] in x) of the price objective (O.loss's value): 1e10 and zeros where a
    price is NaN, infinite or <= 0."""
    p = O.to_params(x)
    mkt = np.array([o["price"] for o in market], dtype=np.float64)
    planes = np.array([sens_vec(p, spot, o["strike"], o["maturity"], r,
                                O.is_call_type(o["option_type"]), N) for o in market])   # [M, 14]
    model = planes[:, 0]
    if not np.all(np.isfinite(model)) or np.any(model <= 0):
        return O.INVALID_LOSS, np.zeros(13)
    rel = (model - mkt) / mkt
    f = np.mean(rel ** 2) + O.feller(p)
    g = (2.0 / len(market)) * ((rel / mkt) @ planes[:, 1:]) * dtheta_dx(p) + feller_grad_x(p)
    return f, g
