"""Writes tests/golden/iv_truth.npz: Black-Scholes quotes with known implied volatility, priced in
60-digit arithmetic (mpmath), and the accuracy of the host route a user has without the library
(SciPy brentq on the textbook formula), which is the bar of tests/test_gpu_iv.py.

CPU only; the GPU tests read the .npz alone (mpmath may be absent there).

    python tests/golden/make_iv_truth.py

Grid: S0 = 100; s = sigma sqrt(T) over geomspace(1e-3, 4, 25); per s, z = x / s over
linspace(-zmax, zmax, 25), zmax = min(12, 3 / s), x = ln(F / K); T, r, q cycle through
{0.1, 1, 2}, {0, 0.03, 0.05}, {0, 0.02}; K = F e^{-x} (rounded to fp64: the truth is computed from
the stored doubles); a call and a put at every point: 1,250 quotes.

Per quote: the inputs, sigma_true, the price rounded to fp64, the true vega, lower (the fp64
bound the library forms: max(S0 e^{-qT} - K e^{-rT}, 0) for a call, the mirror for a put) and
scale = price where lower == 0, else max(price, S0 e^{-qT}, K e^{-rT}).  keep = price - lower >=
1000 eps scale: the rest are in-the-money quotes whose time value the fp64 price no longer holds.

Error unit per quote: u = eps sigma_true + eps scale / vega -- what one ulp of the price or of the
discounted bounds already moves sigma by.  yardstick = the worst |sigma - sigma_true| / u of brentq
(xtol 1e-16, rtol 4 eps) on the textbook formula with scipy.special.ndtr over the kept quotes.
"""
import os

import mpmath as mp
import numpy as np
from scipy.optimize import brentq
from scipy.special import ndtr

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = float(np.finfo(np.float64).eps)
KEEP_ULPS = 1000.0


def grid():
    S0 = 100.0
    Ts, rs, qs = (0.1, 1.0, 2.0), (0.0, 0.03, 0.05), (0.0, 0.02)
    rows = []
    i = 0
    for s in np.geomspace(1e-3, 4.0, 25):
        zmax = min(12.0, 3.0 / s)
        for z in np.linspace(-zmax, zmax, 25):
            T, r, q = Ts[i % 3], rs[(i // 3) % 3], qs[(i // 9) % 2]
            i += 1
            x = z * s
            K = float(S0 * np.exp((r - q) * T) * np.exp(-x))
            sigma = float(s / np.sqrt(T))
            for call in (1, 0):
                rows.append((S0, K, T, r, q, call, sigma))
    return np.array(rows)


def truth(S0, K, T, r, q, call, sigma):
    """(price, vega) in 60 digits from the fp64 inputs."""
    S0, K, T, r, q, sigma = (mp.mpf(float(v)) for v in (S0, K, T, r, q, sigma))
    sq = sigma * mp.sqrt(T)
    d1 = (mp.log(S0 / K) + (r - q) * T) / sq + sq / 2
    d2 = d1 - sq
    A, B = S0 * mp.exp(-q * T), K * mp.exp(-r * T)
    if call:
        price = A * mp.ncdf(d1) - B * mp.ncdf(d2)
    else:
        price = B * mp.ncdf(-d2) - A * mp.ncdf(-d1)
    vega = A * mp.npdf(d1) * mp.sqrt(T)
    return float(price), float(vega)


def bounds(S0, K, T, r, q, call):
    """lower and the two discounted legs, in fp64 as the library forms them."""
    A, B = S0 * np.exp(-q * T), K * np.exp(-r * T)
    lower = np.where(call != 0, np.maximum(A - B, 0.0), np.maximum(B - A, 0.0))
    return lower, A, B


def textbook_price(S0, K, T, r, q, call, sigma):
    sq = sigma * np.sqrt(T)
    d1 = (np.log(S0 / K) + (r - q + 0.5 * sigma * sigma) * T) / sq
    d2 = d1 - sq
    if call:
        return S0 * np.exp(-q * T) * ndtr(d1) - K * np.exp(-r * T) * ndtr(d2)
    return K * np.exp(-r * T) * ndtr(-d2) - S0 * np.exp(-q * T) * ndtr(-d1)


def brentq_iv(price, S0, K, T, r, q, call, lo=1e-9, hi=100.0):
    """What a user has today: a scalar root-finder per option on the textbook formula."""
    def f(sig):
        return textbook_price(S0, K, T, r, q, call, sig) - price
    flo, fhi = f(lo), f(hi)
    if not flo < 0.0:
        return lo
    if not fhi > 0.0:
        return hi
    return brentq(f, lo, hi, xtol=1e-16, rtol=4 * EPS, maxiter=500)


def main():
    mp.mp.dps = 60
    g = grid()
    S0, K, T, r, q, call, sigma = g.T
    n = len(g)
    price, vega = np.empty(n), np.empty(n)
    for i in range(n):
        price[i], vega[i] = truth(*g[i])
    lower, A, B = bounds(S0, K, T, r, q, call)
    scale = np.where(lower == 0.0, price, np.maximum(price, np.maximum(A, B)))
    keep = price - lower >= KEEP_ULPS * EPS * scale
    u = EPS * sigma + EPS * scale / vega
    ratio = np.zeros(n)
    for i in np.flatnonzero(keep):
        got = brentq_iv(price[i], S0[i], K[i], T[i], r[i], q[i], int(call[i]))
        ratio[i] = abs(got - sigma[i]) / u[i]
    yardstick = float(ratio.max())
    worst = int(ratio.argmax())
    print(f"{n} quotes, kept {int(keep.sum())} ({keep.mean():.3f}); out of the money kept: "
          f"{bool(np.all(keep[lower == 0.0]))}")
    print(f"brentq yardstick {yardstick:.4g} u at quote {worst}: s = "
          f"{sigma[worst] * np.sqrt(T[worst]):.4g}, K = {K[worst]:.6g}, call = {int(call[worst])}")
    np.savez(os.path.join(HERE, "iv_truth.npz"), S0=S0, K=K, T=T, r=r, q=q,
             is_call=call.astype(np.int8), sigma_true=sigma, price=price, vega=vega, lower=lower,
             scale=scale, keep=keep, yardstick=np.float64(yardstick))


if __name__ == "__main__":
    main()
