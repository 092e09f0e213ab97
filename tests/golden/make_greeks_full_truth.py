"""Generate tests/golden/greeks_full_truth.json: the maturity and rate sensitivities and the dual
gamma of the COS price at a fixed truncation range, in mpmath at 80 digits -- the
truth tests/test_greeks_full_truth.py holds the NumPy restatement (tests/greeks_full_reference.py)
to, and tests/test_gpu_greeks_full.py the device.  The method is make_greeks_truth.py's.

The series is restated here from the reference's formulas (double_heston.py:48-97, 141-192): the
CF's drift is (r - q), q appears nowhere else, the discount is e^{-rT}; the parameters, S0, K, T, r
and q are the doubles the tests pass; [a, b] is oracle.trunc_range's in fp64, stored, and HELD while
anything moves (so u_k = k pi / (b - a) is held too).  Term k of the price is

    t_k(T, r, q, S0, K) = wt_k F_k(T, r, q) V_k(S0, K),     wt_0 = 1/2, else 1,
    F_k = e^{-rT} Re(phi(u_k; T, r, q) e^{-i u_k a}),   V_k = +-(2 / (b - a)) (S0 chi_k - K psi_k)

and NO derivative formula appears below: every plane's term is a central difference of t_k,

    dprice_dT, rho, (d/dq)   (t_k(x + h') - t_k(x - h')) / (2 h'),  x = T, r or q,
                             h' = h max(|x|, 1),                                      h = 1e-25
    dual_gamma, (gamma)      (t_k(x + h x) - 2 t_k + t_k(x - h x)) / (h x)^2, x = K or S0,
                                                                                     h = 1e-20

(F_k does not depend on S0 or K, nor V_k on T, r or q, so the quotient of t_k is the quotient of the
one factor times the other; that is an identity of the differences, not a derivative.)  The two
planes in brackets, with the price and the dual delta (a first difference in K, h = 1e-25), are
stored as `extra`: the CPU tests hold K^2 dual_gamma = S0^2 gamma and d/dq = -(rho + T price) on
them.

The arithmetic of the steps, at 80 digits (eps = 1e-80).  u_k <= N pi / (b - a) < 2048 pi / 0.2 =
3.3e4 (the clamp keeps b - a >= 0.2).  In T, log F_k has the derivative -r + G(u_k) with |G| <=
v0 |B'| + kappa theta |B| + |drift| u + 2 lambda <= ~0.1 u^2 = 1e8 at the largest u (B' = -(u^2 +
i u) / 2 at tau = 0); in r it is -T + i u T, at most 7e4; in q, i u T.
  first difference:   truncation h'^2 f''' / 6 <= h'^2 |G|^2 / 6 = 4e-50 * 1e16 / 6 < 1e-34 of f'
                      (T <= 2: h' <= 2e-25); rounding 2 eps |f| / (2 h') = 1e-55 |f|, against
                      f' of the size of |f| or more wherever the plane's term matters.
  second difference:  as make_greeks_truth.py's gamma: truncation (h x)^2 u^2 / 12 = 1e-32 of f'',
                      rounding 4 eps |f| / (h x)^2 = 4e-40 |f| / x^2.
All are below 1e-25 of the term's amplitude, which is what the unit below sums.

Per case and plane two doubles are stored: truth = fsum of the differenced terms, and unit = fsum of
their absolute values, the plane's absolute term sum (for dprice_dT the terms are those of the whole
derivative, -r t_k included, and likewise for rho).  Every bar of the two tests is in this unit.

Parameter sets and market data: make_greeks_truth.py's four sets (0 the reference demo's).
  A  grid            N = 128: sets 0-3 x T in {0.1, 1, 2} x K / S0 in {0.8, 1.2} x call, put;
                     S0 = 100, r = 0.03, q = 0                                          48 cases
  B  market data     N = 128: set 1 under (S0, r, q) = (80, 0.01, 0.02), set 2 under (125, 0.05, 0)
                     x T in {0.25, 1.75} x K / S0 in {0.9, 1.1} x call, put             16 cases
  C  clamp           N = 256: set 0, T = 0.1, K in {5, 40, 60, 250, 500, 3000} x call, put,
                     S0 = 100; clamp-active and -inactive options both occur (asserted), the flag
                     is stored                                                          12 cases
  D  series length   N in {1, 2, 17, 772, 773, 2048}: set 0, T = 0.7, K / S0 in {0.9, 1.1}, call,
                     put, S0 = 100, r = 0.03, q = 0                                     24 cases

"restatement_worst"[plane][N] = max |greeks_full_reference.full_vec - truth| / unit over the cases
of that N, on the generating machine; the fixture is REFUSED if any entry exceeds 64 * 2^-52 -- the
condition of make_greeks_truth.py, not a measurement.

Usage: python tests/golden/make_greeks_full_truth.py   (writes greeks_full_truth.json next to
itself; a few minutes on 8 cores)
"""
import json
import multiprocessing
import os
import sys

import mpmath
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import greeks_full_reference as GF  # noqa: E402
import greeks_reference as G  # noqa: E402
import make_greeks_truth as M6  # noqa: E402  (the series in mpmath: factor_mp, payoff)
from oracle import dh_oracle as O  # noqa: E402

mpmath.mp.dps = 80
mpf, mpc = mpmath.mpf, mpmath.mpc
I = mpc(0, 1)
H1, H2 = mpf(10) ** -25, mpf(10) ** -20
CAP = 64 * 2.0 ** -52
CHUNK = 32
NS_D = (1, 2, 17, 772, 773, 2048)
EXTRA = ("price", "dual_delta", "gamma", "dprice_dq")


def case_list(sets):
    out = []

    def add(group, s, S0, r, q, K, T, is_call, N):
        a, b = (float(v) for v in O.trunc_range(sets[s], S0, K, T, r))
        out.append({"group": group, "set": s, "S0": S0, "r": r, "q": q, "K": float(K), "T": T,
                    "is_call": is_call, "N": N, "a": a, "b": b,
                    "clamp": G.clamp_active(sets[s], S0, K, T, r)})

    for s in range(4):
        for T in (0.1, 1.0, 2.0):
            for ratio in (0.8, 1.2):
                for is_call in (True, False):
                    add("A", s, 100.0, 0.03, 0.0, 100.0 * ratio, T, is_call, 128)
    for s, (S0, r, q) in ((1, (80.0, 0.01, 0.02)), (2, (125.0, 0.05, 0.0))):
        for T in (0.25, 1.75):
            for ratio in (0.9, 1.1):
                for is_call in (True, False):
                    add("B", s, S0, r, q, S0 * ratio, T, is_call, 128)
    for K in (5.0, 40.0, 60.0, 250.0, 500.0, 3000.0):
        for is_call in (True, False):
            add("C", 0, 100.0, 0.03, 0.0, K, 0.1, is_call, 256)
    for N in NS_D:
        for ratio in (0.9, 1.1):
            for is_call in (True, False):
                add("D", 0, 100.0, 0.03, 0.0, 100.0 * ratio, 0.7, is_call, N)
    return out


def steps(T, r, q):
    return tuple(H1 * max(abs(mpf(x)), 1) for x in (T, r, q))


def weight_chunk(task):
    """F_k = e^{-rT} Re(phi(u_k; T, r, q) e^{-i u_k a}) for k0 <= k < k1 at (T, r, q) and at each of
    the three moved by +-its step, u_k and a held: rows of seven."""
    prm, T, r, q, a, b, k0, k1 = task
    v01, kp1, t1, s1, r1, v02, kp2, t2, s2, r2, lam, muj, sj = (mpf(v) for v in prm)
    hT, hr, hq = steps(T, r, q)
    T, r, q, a, b = mpf(T), mpf(r), mpf(q), mpf(a), mpf(b)
    comp = mpmath.exp(muj + sj ** 2 / 2) - 1

    def F(u, T, r, q):
        B1, A1 = M6.factor_mp(u, T, kp1, t1, s1, r1)
        B2, A2 = M6.factor_mp(u, T, kp2, t2, s2, r2)
        A = (r - q - lam * comp) * I * u * T + A1 + A2
        jump = mpmath.exp(lam * T * (mpmath.exp(I * u * muj - sj ** 2 * u ** 2 / 2) - 1))
        phi = mpmath.exp(A + B1 * v01 + B2 * v02) * jump
        return mpmath.exp(-r * T) * (phi * mpmath.exp(-I * u * a)).real

    rows = []
    for k in range(k0, k1):
        u = k * mpmath.pi / (b - a)
        rows.append((F(u, T, r, q), F(u, T + hT, r, q), F(u, T - hT, r, q), F(u, T, r + hr, q),
                     F(u, T, r - hr, q), F(u, T, r, q + hq), F(u, T, r, q - hq)))
    return rows


def payoff_chunk(task):
    """Rows of (V_k, its central difference in K, its second central differences in K and in S0)
    for k0 <= k < k1, at fixed [a, b]."""
    S0, K, is_call, a, b, k0, k1 = task
    S0, K, a, b = mpf(S0), mpf(K), mpf(a), mpf(b)
    rows = []
    for k in range(k0, k1):
        def V(s, x):
            return M6.payoff(s, x, is_call, a, b, k)
        mid = V(S0, K)
        hk, hkk, hss = H1 * K, H2 * K, H2 * S0
        rows.append((mid,
                     (V(S0, K + hk) - V(S0, K - hk)) / (2 * hk),
                     (V(S0, K + hkk) - 2 * mid + V(S0, K - hkk)) / hkk ** 2,
                     (V(S0 + hss, K) - 2 * mid + V(S0 - hss, K)) / hss ** 2))
    return rows


def chunks(n):
    return [(k0, min(k0 + CHUNK, n)) for k0 in range(0, n, CHUNK)]


def main():
    sets = M6.parameter_sets()
    cases = case_list(sets)
    c_flags = [c["clamp"] for c in cases if c["group"] == "C"]
    assert any(c_flags) and not all(c_flags), "group C must hold clamped and unclamped options"
    assert not any(c["clamp"] for c in cases if c["group"] != "C")

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

    worst = {name: {} for name in GF.NEW_PLANES}
    for c in cases:
        prm, N = sets[c["set"]], c["N"]
        w, v = W[wkey(c)][:N], V[vkey(c)][:N]
        hT, hr, hq = steps(c["T"], c["r"], c["q"])
        terms = {name: [] for name in GF.NEW_PLANES + EXTRA}
        for k in range(N):
            wt = mpf(1) / 2 if k == 0 else mpf(1)
            f0, fTp, fTm, frp, frm, fqp, fqm = w[k]
            v0, vk, vkk, vss = v[k]
            terms["dprice_dT"].append(wt * (fTp - fTm) / (2 * hT) * v0)
            terms["rho"].append(wt * (frp - frm) / (2 * hr) * v0)
            terms["dual_gamma"].append(wt * f0 * vkk)
            terms["price"].append(wt * f0 * v0)
            terms["dual_delta"].append(wt * f0 * vk)
            terms["gamma"].append(wt * f0 * vss)
            terms["dprice_dq"].append(wt * (fqp - fqm) / (2 * hq) * v0)
        c["truth"] = [float(mpmath.fsum(terms[name])) for name in GF.NEW_PLANES]
        c["unit"] = [float(mpmath.fsum(abs(t) for t in terms[name])) for name in GF.NEW_PLANES]
        c["extra"] = [float(mpmath.fsum(terms[name])) for name in EXTRA]
        got = GF.full_vec(prm, c["S0"], c["K"], c["T"], c["r"], c["is_call"], N, c["q"])
        for i, name in enumerate(GF.NEW_PLANES):
            e = abs(got[name] - c["truth"][i])
            e = e / c["unit"][i] if c["unit"][i] > 0 else (0.0 if e == 0 else np.inf)
            worst[name][str(N)] = max(worst[name].get(str(N), 0.0), e)
    for name in GF.NEW_PLANES:
        print(f"{name:10s} restatement worst / unit: " +
              "  ".join(f"N={n}: {e:.2e}" for n, e in worst[name].items()))
    over = {(name, n): e for name in GF.NEW_PLANES for n, e in worst[name].items()
            if not e <= CAP}
    if over:
        raise SystemExit(f"restatement further than 64 * 2^-52 of the unit from the truth: {over}")

    lines = ",\n".join(json.dumps(c) for c in cases)
    about = ("tests/golden/make_greeks_full_truth.py: 80-digit term-by-term central differences "
             "(in T, r, and twice in K) of the COS series at fixed [a, b]; truth = fsum(terms), "
             "unit = fsum(|terms|) per plane; extra = the truth of price, dual_delta, gamma and "
             "d price / dq; restatement_worst[plane][N] = max |greeks_full_reference.full_vec - "
             "truth| / unit")
    with open(os.path.join(HERE, "greeks_full_truth.json"), "w") as fh:
        fh.write("{" + f'"about": {json.dumps(about)},\n'
                 f'"planes": {json.dumps(list(GF.NEW_PLANES))},\n'
                 f'"extra": {json.dumps(list(EXTRA))},\n'
                 f'"sets": {json.dumps(sets)},\n"restatement_worst": {json.dumps(worst)},\n'
                 f'"cases": [\n{lines}\n]' + "}\n")


if __name__ == "__main__":
    main()
