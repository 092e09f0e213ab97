"""Generate tests/golden/param_sens_truth.json: the COS price and its thirteen parameter
sensitivities at a fixed truncation range, in mpmath at 50 digits, term by term --
the truth tests/test_param_sens_truth.py holds the NumPy restatement (tests/param_grad_reference.py)
to, and tests/test_gpu_param_sens_truth.py the device (param_grad_kernel and the two reductions on
its planes).  tests/golden/param_grad_truth.json and its generator are left as they are.

The series is restated here from the reference's formulas (double_heston.py:48-97, 141-192): the
CF's drift is (r - q), q appears nowhere else, the discount is e^{-rT}; the parameters, S0, K, T, r
and q are the doubles the tests pass; [a, b] is oracle.trunc_range's in fp64, stored, and HELD while
a parameter moves.  Term k of the price is

    t_k(theta) = e^{-rT} wt_k W_k(theta) V_k,     wt_0 = 1/2, else 1,
    W_k = Re(phi(u_k; theta) e^{-i u_k a}),   V_k = +-(2 / (b - a)) (S0 chi_k - K psi_k)

and NO derivative formula appears below: plane i's term k is the central difference of t_k in
parameter i,

    (t_k(theta_i + h_i) - t_k(theta_i - h_i)) / (2 h_i),     h_i = 1e-20 max(|theta_i|, 1)

(make_param_grad_truth.py's step).  V_k does not depend on a model parameter at fixed [a, b], so the
quotient of t_k is the quotient of W_k times e^{-rT} wt_k V_k: an identity of the differences.  log
phi is a sum of three parts -- factor 1's A + B v0, factor 2's, and the jumps' with their
compensator -- and a parameter moves one of them, so only that part is evaluated again; the sum
goes through one exp either way.  phi(0) = 1 whatever the parameters (a CF's normalisation), and is
evaluated as such: W_0 = 1 and every difference of term 0 is exactly 0, which is what makes the
thirteen parameter planes at N = 1 exactly 0 with unit 0 (asserted).

The arithmetic of the step, at 50 digits (eps = 1e-50).  W_k = Re e^{X(theta)}; a derivative in
theta_i costs at most a factor M = max |dX / dtheta_i| (and its own derivatives no more than M per
order).  u_k <= N pi / (b - a) <= 1024 pi / 0.2 = 1.6e4 whatever the case (the clamp keeps b - a
>= 0.2), and with lambda, tau, sigma_j <= 2 and sigma >= 0.1 no dX / dtheta_i exceeds lambda tau
sigma_j u^2 or u tau / sigma by much: M <= 1e8 with room (the cases' largest is about 1e5, group
C's sigma_j at u = 4e3).
  truncation   h^2 W''' / 6 <= h^2 M^2 / 6 = 1e-40 * 1e16 / 6 = 2e-25 of the term's derivative;
  rounding     2 eps |W| / (2 h) = 1e-30 |W|: against a derivative of size M |W| that is 1e-30 / M
               of it, and where the derivative vanishes (by the phase of the cosine, or because M
               is small) it stays 1e-30 of the PRICE's term -- below 2^-52 of a plane's unit as
               long as the plane is more than 1e-14 of the price's size; the smallest plane_ratio
               stored is 2e-4 (kappa1).
Both are below 1e-24 of the term's amplitude, which is what the unit below sums.

Per case and plane two doubles are stored: truth = fsum of the terms, and unit = fsum of their
absolute values, the series' absolute term sum for that plane.  Every bar of the two tests is in
this unit.  The fp64 restatement's own error in it is NOT a few 2^-52 as for the Greeks: the
kappa/sigma/rho chain cancels inside each term (d' against beta', D'/D against d'/d), so kappa2
comes out at about 37,000 * 2^-52, kappa1 at 19,000 (clamp strikes), sigma2 at 6,000 and the price
at 5.  The bars are therefore per plane and group, from "restatement_worst".

Parameter sets: make_param_grad_truth.parameter_sets()'s eight (0 the reference demo's, 1-5 drawn
inside the generator's bounds, 6 with sigma_j = 1e-3, 7 with rho1 = -0.9 and rho2 = 0.9), then 8 and
9: the two sets whose optimiser x is zero wherever the transform is exp or tanh (v0 = kappa = theta
= sigma = lambda = sigma_j = 1, rho = 0) with mu_j = -0.05 and -0.02.
  A  grid            N = 128: sets 0, 5, 6, 7 x T in {0.1, 1, 2} x K / S0 in {0.8, 1, 1.2} x call,
                     put; S0 = 100, r = 0.03, q = 0                                     72 cases
  B  market data     N = 128: set 1 under (S0, r, q) = (80, 0.01, 0.02), set 2 under (125, 0.05, 0)
                     x T in {0.25, 1.75} x K / S0 in {0.9, 1.1} x call, put             16 cases
  C  clamp           N = 256: sets 0, 1, 2, T = 0.1, K in {5, 40, 60, 250, 500, 3000} x call, put,
                     S0 = 100; clamp-active and -inactive options both occur (asserted), the flag
                     is stored                                                          36 cases
  D  series length   N in {1, 2, 17, 65, 336, 337, 1024}: sets 0 and 6, T = 0.7, K / S0 in
                     {0.9, 1.1}, call, put, S0 = 100, r = 0.03, q = 0; the weights of a range are
                     computed once and reused across N by prefix                        56 cases
  E  exact records   N = 128: set 8 under (S0, r) = (97, 0.02), set 9 under (103.5, 0.04), q = 0,
                     x T in {0.2, 1, 2} x K in {85, 100, 115} x call, put; each with "mkt" =
                     truth price * (1 + 0.02 z), z = RandomState(77).randn(36) in case order
                                                                                        36 cases

"restatement_worst"[plane][key] = max |param_grad_reference.sens_vec - truth| / unit over the cases
of key with unit > 0, on the generating machine; key is the group for A, B, C, E and N for D.  The
fixture is REFUSED if any entry exceeds 1e-9 -- a condition, not a measurement: the correct
restatement stays below 8.3e-12 (37,000 * 2^-52), a wrong factor or sign gives 1e-3 to 1.
"plane_ratio"[i] = the median over group D's N = 2 cases of unit_i / unit_price: the natural size
of plane i beside the price, from truth alone (the bound of the N = 1 planes, whose own unit is 0).

Usage: python tests/golden/make_param_sens_truth.py   (writes param_sens_truth.json next to itself;
minutes on 16 cores)
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
import greeks_reference as G  # noqa: E402
import param_grad_reference as R  # noqa: E402
from make_param_grad_truth import parameter_sets as grad_parameter_sets  # noqa: E402
from oracle import dh_oracle as O  # noqa: E402

mpmath.mp.dps = 50
mpf, mpc = mpmath.mpf, mpmath.mpc
I = mpc(0, 1)
H = mpf(10) ** -20
CAP = 1e-9
CHUNK = 32
NS_D = (1, 2, 17, 65, 336, 337, 1024)
NP = len(R.PLANES)


def parameter_sets():
    exact = [[1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, muj, 1.0]
             for muj in (-0.05, -0.02)]
    return grad_parameter_sets() + exact


def case_list(sets):
    """The cases without their truth: dicts of doubles, in the order of the fixture."""
    out = []

    def add(group, s, S0, r, q, K, T, is_call, N):
        a, b = (float(v) for v in O.trunc_range(sets[s], S0, K, T, r))
        out.append({"group": group, "set": s, "S0": S0, "r": r, "q": q, "K": float(K), "T": T,
                    "is_call": is_call, "N": N, "a": a, "b": b,
                    "clamp": G.clamp_active(sets[s], S0, K, T, r)})

    for s in (0, 5, 6, 7):
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
        for s in (0, 6):
            for ratio in (0.9, 1.1):
                for is_call in (True, False):
                    add("D", s, 100.0, 0.03, 0.0, 100.0 * ratio, 0.7, is_call, N)
    for s, (S0, r) in ((8, (97.0, 0.02)), (9, (103.5, 0.04))):
        for T in (0.2, 1.0, 2.0):
            for K in (85.0, 100.0, 115.0):
                for is_call in (True, False):
                    add("E", s, S0, r, 0.0, K, T, is_call, 128)
    return out


# ---- the series in mpmath (double_heston.py:48-97, 141-192) ------------------------------------
def factor_part(u, tau, v0, kappa, theta, sigma, rho):
    """One Heston factor's share of log phi: A + B v0."""
    beta = kappa - rho * sigma * I * u
    d = mpmath.sqrt(beta ** 2 + sigma ** 2 * u * (u + I))
    bm = beta - d
    g = bm / (beta + d)
    e = mpmath.exp(-d * tau)
    B = (bm / sigma ** 2) * ((1 - e) / (1 - g * e))
    A = (kappa * theta / sigma ** 2) * (bm * tau - 2 * mpmath.log((1 - g * e) / (1 - g)))
    return A + B * v0


def jump_part(u, tau, lam, muj, sj):
    """The jumps' share of log phi, compensator included."""
    comp = mpmath.exp(muj + sj ** 2 / 2) - 1
    return -lam * comp * I * u * tau + \
        lam * tau * (mpmath.exp(I * u * muj - sj ** 2 * u ** 2 / 2) - 1)


PARTS = ((factor_part, 0, 5), (factor_part, 5, 10), (jump_part, 10, 13))


def weight_chunk(task):
    """Rows of (W_k, then the central difference of W_k in each of the thirteen parameters) for
    k0 <= k < k1, W_k = Re(phi(u_k) e^{-i u_k a})."""
    prm, T, r, q, a, b, k0, k1 = task
    prm = [mpf(v) for v in prm]
    T, r, q, a, b = mpf(T), mpf(r), mpf(q), mpf(a), mpf(b)
    rows = []
    for k in range(k0, k1):
        if k == 0:                                         # phi(0) = 1 for every parameter value
            rows.append((mpf(1),) + (mpf(0),) * 13)
            continue
        u = k * mpmath.pi / (b - a)
        parts = [fn(u, T, *prm[lo:hi]) for fn, lo, hi in PARTS]
        fixed = (r - q) * I * u * T - I * u * a
        row = [mpmath.exp(fixed + mpmath.fsum(parts)).real]
        for j, (fn, lo, hi) in enumerate(PARTS):
            rest = fixed + mpmath.fsum(parts[:j] + parts[j + 1:])
            for i in range(lo, hi):
                h = H * max(abs(prm[i]), 1)
                up, dn = list(prm[lo:hi]), list(prm[lo:hi])
                up[i - lo], dn[i - lo] = prm[i] + h, prm[i] - h
                row.append((mpmath.exp(rest + fn(u, T, *up)).real
                            - mpmath.exp(rest + fn(u, T, *dn)).real) / (2 * h))
        rows.append(tuple(row))
    return rows


def payoff_chunk(task):
    """V_k (double_heston.py:141-158, 176-186), without the discount, for k0 <= k < k1."""
    S0, K, is_call, a, b, k0, k1 = task
    S0, K, a, b = mpf(S0), mpf(K), mpf(a), mpf(b)
    xK = mpmath.log(K / S0)
    c, d = (xK, b) if is_call else (a, xK)
    rows = []
    for k in range(k0, k1):
        if k == 0:
            chi, psi = mpmath.exp(d) - mpmath.exp(c), d - c
        else:
            w = k * mpmath.pi / (b - a)
            chi = (mpmath.cos(w * (d - a)) * mpmath.exp(d) - mpmath.cos(w * (c - a)) * mpmath.exp(c)
                   + w * mpmath.sin(w * (d - a)) * mpmath.exp(d)
                   - w * mpmath.sin(w * (c - a)) * mpmath.exp(c)) / (1 + w ** 2)
            psi = (mpmath.sin(w * (d - a)) - mpmath.sin(w * (c - a))) / w
        v = 2 / (b - a) * (S0 * chi - K * psi)
        rows.append(v if is_call else -v)
    return rows


def chunks(n):
    return [(k0, min(k0 + CHUNK, n)) for k0 in range(0, n, CHUNK)]


def main():
    sets = parameter_sets()
    assert len(sets) == 10 and abs(sets[6][12] - 1e-3) < 1e-15
    assert sets[7][4] == -0.9 and sets[7][9] == 0.9
    cases = case_list(sets)
    c_flags = [c["clamp"] for c in cases if c["group"] == "C"]
    assert any(c_flags) and not all(c_flags), "group C must hold clamped and unclamped options"
    for s in range(3):                                     # and so must each set's tile of group C
        f = [c["clamp"] for c in cases if c["group"] == "C" and c["set"] == s]
        assert any(f) and not all(f), (s, f)

    # the weights depend on (set, market, T, [a, b]) and the payoffs on (S0, K, type, [a, b]); both
    # are computed once up to the longest series that needs them and reused across N by prefix
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

    worst = {name: {} for name in R.PLANES}
    for c in cases:
        prm, N = sets[c["set"]], c["N"]
        w, v = W[wkey(c)][:N], V[vkey(c)][:N]
        disc = mpmath.exp(-mpf(c["r"]) * mpf(c["T"]))
        terms = [[(disc / 2 if k == 0 else disc) * w[k][i] * v[k] for k in range(N)]
                 for i in range(NP)]
        c["truth"] = [float(mpmath.fsum(t)) for t in terms]
        c["unit"] = [float(mpmath.fsum(abs(x) for x in t)) for t in terms]
        if N == 1:                                         # term 0 alone: no parameter moves it
            assert not any(c["truth"][1:]) and not any(c["unit"][1:]), c
        got = R.sens_vec(prm, c["S0"], c["K"], c["T"], c["r"], c["is_call"], N, c["q"],
                         ab=(c["a"], c["b"]))
        key = str(N) if c["group"] == "D" else c["group"]
        for i, name in enumerate(R.PLANES):
            if c["unit"][i] > 0:
                e = abs(got[i] - c["truth"][i]) / c["unit"][i]
                worst[name][key] = max(worst[name].get(key, 0.0), e if e == e else np.inf)
    for name in R.PLANES:
        print(f"{name:9s} restatement worst / unit: " +
              "  ".join(f"{n}: {e:.2e}" for n, e in worst[name].items()))
    over = {(name, n): e for name in R.PLANES for n, e in worst[name].items() if not e <= CAP}
    if over:
        raise SystemExit(f"restatement further than 1e-9 of the unit from the truth: {over}")

    z = np.random.RandomState(77).randn(36)
    group_e = [c for c in cases if c["group"] == "E"]
    assert len(group_e) == 36
    for c, zi in zip(group_e, z):
        c["mkt"] = float(c["truth"][0] * (1 + 0.02 * zi))
    two = [c for c in cases if c["group"] == "D" and c["N"] == 2]
    ratio = [float(np.median([c["unit"][i] / c["unit"][0] for c in two])) for i in range(NP)]

    lines = ",\n".join(json.dumps(c) for c in cases)
    about = ("tests/golden/make_param_sens_truth.py: 50-digit term-by-term central differences of "
             "the COS series at fixed [a, b]; truth = fsum(terms), unit = fsum(|terms|) per plane; "
             "restatement_worst[plane][group, or N in group D] = max |param_grad_reference.sens_vec "
             "- truth| / unit; plane_ratio = median unit_i / unit_price over group D's N = 2 cases")
    with open(os.path.join(HERE, "param_sens_truth.json"), "w") as fh:
        fh.write("{" + f'"about": {json.dumps(about)},\n"planes": {json.dumps(list(R.PLANES))},\n'
                 f'"sets": {json.dumps(sets)},\n"restatement_worst": {json.dumps(worst)},\n'
                 f'"plane_ratio": {json.dumps(ratio)},\n"cases": [\n{lines}\n]' + "}\n")


if __name__ == "__main__":
    main()
