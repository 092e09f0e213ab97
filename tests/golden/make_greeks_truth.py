"""Generate tests/golden/greeks_truth.json: the COS price and its five analytic Greeks (delta, gamma,
dual delta, vega1, vega2) at a fixed truncation range, in mpmath at 80 digits -- the
truth tests/test_greeks_truth.py holds the NumPy restatement (tests/greeks_reference.py) to, and
tests/test_gpu_greeks_truth.py the device.

The series is restated here from the reference's formulas (double_heston.py:48-97, 141-192): the
CF's drift is (r - q), q appears nowhere else, the discount is e^{-rT}; the parameters, S0, K, T, r
and q are the doubles the tests pass; [a, b] is oracle.trunc_range's in fp64, stored, and HELD while
anything moves.  Term k of the price is

    t_k(S0, K, v01, v02) = e^{-rT} wt_k W_k(v01, v02) V_k(S0, K),     wt_0 = 1/2, else 1,
    W_k = Re(phi(u_k) e^{-i u_k a}),   V_k = +-(2 / (b - a)) (S0 chi_k - K psi_k),  xK = log(K / S0)

and NO derivative formula appears below: every Greek's term is a central difference of t_k,

    delta, dual delta   (t_k(x + h x) - t_k(x - h x)) / (2 h x),   x = S0 or K,        h = 1e-25
    vega1, vega2        the same in v01 or v02 with the step h max(|v0|, 1),          h = 1e-25
    gamma               (t_k(S0 + h S0) - 2 t_k + t_k(S0 - h S0)) / (h S0)^2,          h = 1e-20

(W_k does not depend on S0 or K, nor V_k on v0, so the quotient of t_k is the quotient of the one
factor times the other; that is an identity of the differences, not a derivative.)

The arithmetic of the steps, at 80 digits (eps = 1e-80).  t_k depends on S0 and K through xK with
the frequency u_k <= N pi / (b - a) < 2048 pi / 0.2 = 3.3e4 (the clamp keeps b - a >= 0.2), so each
derivative in log S0 or log K costs at most a factor u = 3.3e4; in v0 the exponent is linear with
|B_j| <= ~u / sigma_j < 2e5.
  first difference:   truncation (h x)^2 f''' / 6  <= h^2 u^2 / 6 = 2e-42 of f' (v0: 1e-50 B^2 / 6
                      = 7e-41); rounding 2 eps |f| / (2 h x) against f' >= ~|f| / x: 1e-55.
  second difference:  truncation (h x)^2 f'''' / 12 <= h^2 u^2 / 12 = 1e-32 of f''; rounding
                      4 eps |f| / (h x)^2 against f'' >= ~|f| / x^2: 4e-40.
All are below 1e-25 of the term's size (its amplitude: where a term's derivative vanishes by the
phase of its cosine, the errors stay relative to the amplitude, which is what the unit below sums).

Per case and plane two doubles are stored: truth = fsum of the differenced terms, and unit = fsum of
their absolute values, the series' absolute term sum for that plane.  Every bar of the two tests is
in this unit, which keeps a bar meaningful where the value is at rounding level (the clamped put
K = 40 has delta -9.08e-10 with unit 0.17).

Parameter sets: 0 the reference demo's, 1 and 2 drawn (RandomState(20)) inside the generator's
bounds (LO, HI of tests/test_gpu_greeks.py), 3 a further draw with rho1 = -0.9, rho2 = 0.9.
  A  grid            N = 128: sets 0-3 x T in {0.1, 1, 2} x K / S0 in {0.8, 1, 1.2} x call, put;
                     S0 = 100, r = 0.03, q = 0                                          72 cases
  B  market data     N = 128: set 1 under (S0, r, q) = (80, 0.01, 0.02), set 2 under (125, 0.05, 0)
                     x T in {0.25, 1.75} x K / S0 in {0.9, 1.1} x call, put             16 cases
  C  clamp           N = 256: sets 0, 1, 2, T = 0.1, K in {5, 40, 60, 250, 500, 3000} x call, put,
                     S0 = 100; clamp-active and -inactive options both occur (asserted), the flag
                     is stored                                                          36 cases
  D  series length   N in {1, 2, 65, 1080, 1081, 2048}: set 0, T = 0.7, K / S0 in {0.9, 1.1}, call,
                     put, S0 = 100, r = 0.03, q = 0                                     24 cases

"restatement_worst"[plane][N] = max |greeks_reference.greeks_vec - truth| / unit over the cases of
that N, on the generating machine; the fixture is REFUSED if any entry exceeds 64 * 2^-52 -- a
condition, not a measurement: a correct fp64 restatement stays far inside it, a wrong factor gives
an error of order 1 in this unit.

Usage: python tests/golden/make_greeks_truth.py   (writes greeks_truth.json next to itself; a few
minutes on 16 cores)
"""
import json
import multiprocessing
import os
import sys

import mpmath
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import greeks_reference as G  # noqa: E402
from oracle import dh_oracle as O  # noqa: E402

mpmath.mp.dps = 80
mpf, mpc = mpmath.mpf, mpmath.mpc
I = mpc(0, 1)
H1, H2 = mpf(10) ** -25, mpf(10) ** -20
CAP = 64 * 2.0 ** -52
CHUNK = 64
LO = np.array([0.025, 1.5, 0.025, 0.2, -0.85, 0.02, 0.3, 0.025, 0.1, -0.7, 0.05, -0.08, 0.03])
HI = np.array([0.08, 4.5, 0.065, 0.5, -0.4, 0.07, 1.2, 0.07, 0.35, -0.2, 0.25, -0.01, 0.12])
DEMO = [0.04, 2.0, 0.04, 0.3, -0.5, 0.04, 1.5, 0.04, 0.2, -0.3, 0.5, -0.05, 0.10]
NS_D = (1, 2, 65, 1080, 1081, 2048)


def parameter_sets():
    rs = np.random.RandomState(20)
    draws = LO + (HI - LO) * rs.rand(3, 13)
    draws[2, 4], draws[2, 9] = -0.9, 0.9
    return [list(map(float, DEMO))] + [list(map(float, d)) for d in draws]


def case_list(sets):
    """The cases without their truth: dicts of doubles, in the order of the fixture."""
    out = []

    def add(group, s, S0, r, q, K, T, is_call, N):
        a, b = (float(v) for v in O.trunc_range(sets[s], S0, K, T, r))
        out.append({"group": group, "set": s, "S0": S0, "r": r, "q": q, "K": float(K), "T": T,
                    "is_call": is_call, "N": N, "a": a, "b": b,
                    "clamp": G.clamp_active(sets[s], S0, K, T, r)})

    for s in range(4):
        for T in (0.1, 1.0, 2.0):
            for ratio in (0.8, 1.0, 1.2):
                for is_call in (True, False):
                    add("A", s, 100.0, 0.03, 0.0, 100.0 * ratio, T, is_call, 128)
    for s, (S0, r, q) in ((1, (80.0, 0.01, 0.02)), (2, (125.0, 0.05, 0.0))):
        for T in (0.25, 1.75):
            for ratio in (0.9, 1.1):
                for is_call in (True, False):
                    add("B", s, S0, r, q, S0 * ratio, T, is_call, 128)
    for s in range(3):
        for K in (5.0, 40.0, 60.0, 250.0, 500.0, 3000.0):
            for is_call in (True, False):
                add("C", s, 100.0, 0.03, 0.0, K, 0.1, is_call, 256)
    for N in NS_D:
        for ratio in (0.9, 1.1):
            for is_call in (True, False):
                add("D", 0, 100.0, 0.03, 0.0, 100.0 * ratio, 0.7, is_call, N)
    return out


# ---- the series in mpmath (double_heston.py:48-97, 141-192) ------------------------------------
def factor_mp(u, tau, kappa, theta, sigma, rho):
    beta = kappa - rho * sigma * I * u
    d = mpmath.sqrt(beta ** 2 + sigma ** 2 * u * (u + I))
    bm = beta - d
    g = bm / (beta + d)
    e = mpmath.exp(-d * tau)
    B = (bm / sigma ** 2) * ((1 - e) / (1 - g * e))
    A = (kappa * theta / sigma ** 2) * (bm * tau - 2 * mpmath.log((1 - g * e) / (1 - g)))
    return B, A


def weight_chunk(task):
    """W_k = Re(phi(u_k) e^{-i u_k a}) for k0 <= k < k1 at (v01, v02) and at each v0 moved by +-its
    step: rows of (W, W(v01 + h1), W(v01 - h1), W(v02 + h2), W(v02 - h2)).  phi is evaluated as the
    function of (v01, v02) it is: exp(A + B1 v01 + B2 v02) * jump."""
    prm, T, r, q, a, b, k0, k1 = task
    v01, kp1, t1, s1, r1, v02, kp2, t2, s2, r2, lam, muj, sj = (mpf(v) for v in prm)
    T, r, q, a, b = mpf(T), mpf(r), mpf(q), mpf(a), mpf(b)
    h1, h2 = H1 * max(abs(v01), 1), H1 * max(abs(v02), 1)
    rows = []
    for k in range(k0, k1):
        u = k * mpmath.pi / (b - a)
        B1, A1 = factor_mp(u, T, kp1, t1, s1, r1)
        B2, A2 = factor_mp(u, T, kp2, t2, s2, r2)
        comp = mpmath.exp(muj + sj ** 2 / 2) - 1
        A = (r - q - lam * comp) * I * u * T + A1 + A2
        jump = mpmath.exp(lam * T * (mpmath.exp(I * u * muj - sj ** 2 * u ** 2 / 2) - 1))
        shift = mpmath.exp(-I * u * a)
        rows.append(tuple((mpmath.exp(A + B1 * x + B2 * y) * jump * shift).real
                          for x, y in ((v01, v02), (v01 + h1, v02), (v01 - h1, v02),
                                       (v01, v02 + h2), (v01, v02 - h2))))
    return rows


def payoff(S0, K, is_call, a, b, k):
    """V_k (double_heston.py:141-158, 176-186), without the discount."""
    xK = mpmath.log(K / S0)
    c, d = (xK, b) if is_call else (a, xK)
    if k == 0:
        chi, psi = mpmath.exp(d) - mpmath.exp(c), d - c
    else:
        w = k * mpmath.pi / (b - a)
        chi = (mpmath.cos(w * (d - a)) * mpmath.exp(d) - mpmath.cos(w * (c - a)) * mpmath.exp(c)
               + w * mpmath.sin(w * (d - a)) * mpmath.exp(d)
               - w * mpmath.sin(w * (c - a)) * mpmath.exp(c)) / (1 + w ** 2)
        psi = (mpmath.sin(w * (d - a)) - mpmath.sin(w * (c - a))) / w
    v = 2 / (b - a) * (S0 * chi - K * psi)
    return v if is_call else -v


def payoff_chunk(task):
    """Rows of (V_k, its central difference in S0, its second central difference in S0, its central
    difference in K) for k0 <= k < k1, at fixed [a, b]."""
    S0, K, is_call, a, b, k0, k1 = task
    S0, K, a, b = mpf(S0), mpf(K), mpf(a), mpf(b)
    rows = []
    for k in range(k0, k1):
        def V(s, x):
            return payoff(s, x, is_call, a, b, k)
        mid = V(S0, K)
        hs, hk, hg = H1 * S0, H1 * K, H2 * S0
        rows.append((mid,
                     (V(S0 + hs, K) - V(S0 - hs, K)) / (2 * hs),
                     (V(S0 + hg, K) - 2 * mid + V(S0 - hg, K)) / hg ** 2,
                     (V(S0, K + hk) - V(S0, K - hk)) / (2 * hk)))
    return rows


def chunks(n):
    return [(k0, min(k0 + CHUNK, n)) for k0 in range(0, n, CHUNK)]


def main():
    sets = parameter_sets()
    cases = case_list(sets)
    c_flags = [c["clamp"] for c in cases if c["group"] == "C"]
    assert any(c_flags) and not all(c_flags), "group C must hold clamped and unclamped options"
    for s in range(3):                                     # and so must each set's tile of group C
        f = [c["clamp"] for c in cases if c["group"] == "C" and c["set"] == s]
        assert any(f) and not all(f), (s, f)

    # the weights depend on (set, market, T, [a, b]) and the payoffs on (S0, K, type, [a, b]); both
    # are computed once up to the longest series that needs them
    wkey = lambda c: (c["set"], c["T"], c["r"], c["q"], c["a"], c["b"])            # noqa: E731
    vkey = lambda c: (c["S0"], c["K"], c["is_call"], c["a"], c["b"])               # noqa: E731
    wn, vn = {}, {}
    for c in cases:
        wn[wkey(c)] = max(wn.get(wkey(c), 0), c["N"])
        vn[vkey(c)] = max(vn.get(vkey(c), 0), c["N"])
    wtasks = [(key, (sets[key[0]],) + key[1:] + ch) for key, n in wn.items() for ch in chunks(n)]
    vtasks = [(key, key + ch) for key, n in vn.items() for ch in chunks(n)]
    print(f"{len(cases)} cases: {sum(wn.values())} CF terms, {sum(vn.values())} payoff terms",
          flush=True)
    with multiprocessing.Pool(min(16, os.cpu_count() or 1)) as pool:
        wrows = pool.map(weight_chunk, [t for _, t in wtasks], chunksize=1)
        print("weights done", flush=True)
        vrows = pool.map(payoff_chunk, [t for _, t in vtasks], chunksize=1)
    W, V = {}, {}
    for (key, _), rows in zip(wtasks, wrows):              # the tasks of a key are in k's order
        W.setdefault(key, []).extend(rows)
    for (key, _), rows in zip(vtasks, vrows):
        V.setdefault(key, []).extend(rows)

    worst = {name: {} for name in G.PLANES}
    for c in cases:
        prm, N = sets[c["set"]], c["N"]
        w, v = W[wkey(c)][:N], V[vkey(c)][:N]
        disc = mpmath.exp(-mpf(c["r"]) * mpf(c["T"]))
        h1, h2 = H1 * max(abs(mpf(prm[0])), 1), H1 * max(abs(mpf(prm[5])), 1)
        terms = {name: [] for name in G.PLANES}
        for k in range(N):
            f = disc / 2 if k == 0 else disc
            w0, w1p, w1m, w2p, w2m = w[k]
            v0, vs, vss, vk = v[k]
            terms["price"].append(f * w0 * v0)
            terms["delta"].append(f * w0 * vs)
            terms["gamma"].append(f * w0 * vss)
            terms["dual_delta"].append(f * w0 * vk)
            terms["vega1"].append(f * (w1p - w1m) / (2 * h1) * v0)
            terms["vega2"].append(f * (w2p - w2m) / (2 * h2) * v0)
        c["truth"] = [float(mpmath.fsum(terms[name])) for name in G.PLANES]
        c["unit"] = [float(mpmath.fsum(abs(t) for t in terms[name])) for name in G.PLANES]
        got = G.greeks_vec(prm, c["S0"], c["K"], c["T"], c["r"], c["is_call"], N, c["q"])
        for i, name in enumerate(G.PLANES):
            e = abs(got[name] - c["truth"][i])             # unit 0 (the vegas at N = 1: B(0) = 0)
            e = e / c["unit"][i] if c["unit"][i] > 0 else (0.0 if e == 0 else np.inf)
            worst[name][str(N)] = max(worst[name].get(str(N), 0.0), e)
    for name in G.PLANES:
        print(f"{name:10s} restatement worst / unit: " +
              "  ".join(f"N={n}: {e:.2e}" for n, e in worst[name].items()))
    over = {(name, n): e for name in G.PLANES for n, e in worst[name].items() if not e <= CAP}
    if over:
        raise SystemExit(f"restatement further than 64 * 2^-52 of the unit from the truth: {over}")

    lines = ",\n".join(json.dumps(c) for c in cases)
    about = ("tests/golden/make_greeks_truth.py: 80-digit term-by-term central differences of the "
             "COS series at fixed [a, b]; truth = fsum(terms), unit = fsum(|terms|) per plane; "
             "restatement_worst[plane][N] = max |greeks_reference.greeks_vec - truth| / unit")
    with open(os.path.join(HERE, "greeks_truth.json"), "w") as fh:
        fh.write("{" + f'"about": {json.dumps(about)},\n"planes": {json.dumps(list(G.PLANES))},\n'
                 f'"sets": {json.dumps(sets)},\n"restatement_worst": {json.dumps(worst)},\n'
                 f'"cases": [\n{lines}\n]' + "}\n")


if __name__ == "__main__":
    main()
