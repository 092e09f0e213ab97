"""Generate tests/golden/param_grad_truth.json: the COS price and its thirteen parameter
sensitivities at a fixed truncation range, in mpmath at 50 digits -- the truth
tests/test_param_grad.py holds the NumPy restatement (tests/param_grad_reference.py) to.

The series is restated here a second time, from the reference's formulas (double_heston.py:48-97,
141-192), in 50-digit arithmetic: the parameters are the doubles the tests pass, the range [a, b]
is oracle.trunc_range's in fp64 (stored, and HELD while a parameter moves), and each sensitivity is
the central difference of the 50-digit price with h = 1e-20 max(|theta|, 1): its truncation error
is ~1e-40 and its rounding error ~1e-30 of the price, far below a double's.  No derivative formula
is used, so the fixture is independent of the closed forms under test.

Cases: 8 parameter sets (the reference demo's, five draws inside the generator's bounds, one with
sigma_j = 1e-3, one with rho1 = -0.9 and rho2 = 0.9) x T in {0.1, 1, 2} x K / S0 in {0.8, 1, 1.2}
x call and put, S0 = 100, r = 0.03, N = 128: 144 cases of 14 values.

Stored: "cases" (prm, S0, K, T, r, is_call, a, b, truth[14] rounded to double), "planes", and
"restatement_worst": the restatement's worst |error| per plane in units of max |plane| over the
fixture, on the generating machine -- tests/test_param_grad.py sets each plane's bar at 10x it.

Usage: python tests/golden/make_param_grad_truth.py   (writes param_grad_truth.json next to itself)
"""
import json
import os
import sys

import mpmath
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import param_grad_reference as R  # noqa: E402
from oracle import dh_oracle as O  # noqa: E402

mpmath.mp.dps = 50
mpf, mpc = mpmath.mpf, mpmath.mpc
S0, RATE, N = 100.0, 0.03, 128
LO = np.array([0.025, 1.5, 0.025, 0.2, -0.85, 0.02, 0.3, 0.025, 0.1, -0.7, 0.05, -0.08, 0.03])
HI = np.array([0.08, 4.5, 0.065, 0.5, -0.4, 0.07, 1.2, 0.07, 0.35, -0.2, 0.25, -0.01, 0.12])
DEMO = [0.04, 2.0, 0.04, 0.3, -0.5, 0.04, 1.5, 0.04, 0.2, -0.3, 0.5, -0.05, 0.10]


def parameter_sets():
    rs = np.random.RandomState(20)
    draws = LO + (HI - LO) * rs.rand(7, 13)
    draws[5, 12] = 1e-3                       # sigma_j small
    draws[6, 4], draws[6, 9] = -0.9, 0.9      # |rho| near 0.9, both signs
    return [list(map(float, DEMO))] + [list(map(float, d)) for d in draws]


def factor_mp(u, tau, kappa, theta, sigma, rho):
    beta = kappa - rho * sigma * mpc(0, 1) * u
    d = mpmath.sqrt(beta ** 2 + sigma ** 2 * u * (u + mpc(0, 1)))
    bm = beta - d
    g = bm / (beta + d)
    e = mpmath.exp(-d * tau)
    B = (bm / sigma ** 2) * ((1 - e) / (1 - g * e))
    A = (kappa * theta / sigma ** 2) * (bm * tau - 2 * mpmath.log((1 - g * e) / (1 - g)))
    return B, A


def cf_mp(u, tau, prm, r):
    v01, k1, t1, s1, r1, v02, k2, t2, s2, r2, lam, muj, sj = prm
    B1, A1 = factor_mp(u, tau, k1, t1, s1, r1)
    B2, A2 = factor_mp(u, tau, k2, t2, s2, r2)
    comp = mpmath.exp(muj + sj ** 2 / 2) - 1
    A = (r - lam * comp) * mpc(0, 1) * u * tau + A1 + A2
    jump = mpmath.exp(lam * tau * (mpmath.exp(mpc(0, 1) * u * muj - sj ** 2 * u ** 2 / 2) - 1))
    return mpmath.exp(A + B1 * v01 + B2 * v02) * jump


def weights_mp(prm, T, r, a, b):
    """Re(phi(u_k) e^{-i u_k a}), k < N, halved at k = 0."""
    out = []
    for k in range(N):
        u = k * mpmath.pi / (b - a)
        w = cf_mp(u, T, prm, r) * mpmath.exp(-mpc(0, 1) * u * a)
        out.append(w.real / 2 if k == 0 else w.real)
    return out


def payoff_mp(K, T, r, is_call, a, b):
    """e^{-rT} V_k, k < N (double_heston.py:141-158, 176-186)."""
    xK = mpmath.log(K / mpf(S0))
    c, d = (xK, b) if is_call else (a, xK)
    out = []
    for k in range(N):
        if k == 0:
            chi, psi = mpmath.exp(d) - mpmath.exp(c), d - c
        else:
            w = k * mpmath.pi / (b - a)
            chi = (mpmath.cos(w * (d - a)) * mpmath.exp(d) - mpmath.cos(w * (c - a)) * mpmath.exp(c)
                   + w * mpmath.sin(w * (d - a)) * mpmath.exp(d)
                   - w * mpmath.sin(w * (c - a)) * mpmath.exp(c)) / (1 + w ** 2)
            psi = (mpmath.sin(w * (d - a)) - mpmath.sin(w * (c - a))) / w
        v = 2 / (b - a) * (S0 * chi - K * psi)
        out.append(mpmath.exp(-r * T) * (v if is_call else -v))
    return out


def main():
    cases, truth = [], []
    for prm in parameter_sets():
        for T in (0.1, 1.0, 2.0):
            cache = {}                        # (a, b) -> the 27 weight vectors: they ignore K, type
            for ratio in (0.8, 1.0, 1.2):
                K = S0 * ratio
                a, b = (float(v) for v in O.trunc_range(prm, S0, K, T, RATE))
                if (a, b) not in cache:
                    P = [mpf(v) for v in prm]
                    ws = [weights_mp(P, mpf(T), mpf(RATE), mpf(a), mpf(b))]
                    for i in range(13):
                        h = mpf(10) ** -20 * max(abs(P[i]), 1)
                        up, dn = list(P), list(P)
                        up[i], dn[i] = P[i] + h, P[i] - h
                        wu = weights_mp(up, mpf(T), mpf(RATE), mpf(a), mpf(b))
                        wd = weights_mp(dn, mpf(T), mpf(RATE), mpf(a), mpf(b))
                        ws.append([(x - y) / (2 * h) for x, y in zip(wu, wd)])
                    cache[(a, b)] = ws
                for is_call in (True, False):
                    V = payoff_mp(mpf(K), mpf(T), mpf(RATE), is_call, mpf(a), mpf(b))
                    vals = [float(mpmath.fsum(x * v for x, v in zip(w, V))) for w in cache[(a, b)]]
                    cases.append({"prm": prm, "S0": S0, "K": K, "T": T, "r": RATE,
                                  "is_call": is_call, "a": a, "b": b, "truth": vals})
                    truth.append(vals)
            print(f"set {prm[:2]} T={T}: {len(cases)} cases", flush=True)
    truth = np.array(truth)
    got = np.array([R.sens_vec(c["prm"], c["S0"], c["K"], c["T"], c["r"], c["is_call"], N,
                               ab=(c["a"], c["b"])) for c in cases])
    scale = np.max(np.abs(truth), axis=0)
    worst = np.max(np.abs(got - truth), axis=0) / scale
    for name, w, s in zip(R.PLANES, worst, scale):
        print(f"{name:9s} worst {w:.3e} of max |plane| {s:.3e}")
    with open(os.path.join(HERE, "param_grad_truth.json"), "w") as fh:
        json.dump({"about": "tests/golden/make_param_grad_truth.py: 50-digit central differences "
                            "of the COS series at fixed [a, b]; restatement_worst in units of "
                            "max |plane| over the fixture",
                   "N": N, "planes": list(R.PLANES), "plane_scale": scale.tolist(),
                   "restatement_worst": worst.tolist(), "cases": cases}, fh, indent=0)


if __name__ == "__main__":
    main()
