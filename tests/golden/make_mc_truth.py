"""Generate tests/golden/mc_truth.npz: the Monte Carlo step of DESIGN.md 3.15 walked in mpmath at
50 digits, the truth the path tests hold the NumPy restatement (tests/test_mc.py) and the kernel
(tests/test_gpu_mc.py) to.

The walk below restates the step a second time, from the document, in exact-for-our-purposes
arithmetic: the parameters are the doubles the tests pass, every expression is the document's, and
nothing is rounded until the end.  Philox and the 53-bit uniforms are integers and dyadic
rationals, so they are taken from tests/mc_reference.py (philox4x32_10, uniform; held to known
answers by tests/test_mc.py); the angle uses the scheme's own double 6.283185307179586, not pi;
the three decisions of a step (psi <= 1.5, U_v <= p, U_N > cdf_k) are taken in mpmath.

Configuration (mc_reference.TRUTH_*): 8 steps per year, observations at steps 2, 4, 8, spot 100,
rate 0.03, seed 0x9E3779B900000005 (high key word live), 32 path indices whose high counter word
is 0, 1 and 5, four parameter sets (the README's, the stressed one, v0 = 0 without jumps at |rho|
= 0.999, lambda dt = 1 with sigma_j = 0).

Stored:
  truth, truth_lo   [4, n_paths, 3, 6] the truth rounded to double, and the rounded remainder
                    (so an error resolves below an ulp in plain float64: |(got - truth) - lo|)
  restatement       [4, n_paths, 3, 6] mc_reference.simulate's output on the generating machine
  rel_err [6]       the restatement's worst relative error per statistic against the truth
  abs_err [2]       its worst absolute error on v1, v2       (both by mc_reference.truth_errors)
  paths, seed, sets, steps_per_year, obs_steps, spot, rate    the configuration
  count_names, counts   quadratic / exponential / v' = 0 steps, steps with one and with more jumps
  psi_gap, u_gap    the smallest distance of any decision from its switch (mpmath)

The file is written only if over the fixture both QE branches, an exact zero variance, one jump
and two or more jumps occur, no decision lies within 1e-9 of its switch (in mpmath and in float64)
and the mpmath decisions equal the float64 restatement's at every (set, path, step).

Usage: python tests/golden/make_mc_truth.py   (writes mc_truth.npz next to itself)
"""
import os
import sys

import mpmath
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mc_reference as R  # noqa: E402

mpmath.mp.dps = 50
mpf = mpmath.mpf
MIN_GAP = 1e-9
COUNTS = ("quad", "expo", "zero", "n1", "n2")


class FactorMP:
    def __init__(self, kappa, theta, sigma, rho, dt):
        self.kappa, self.theta, self.dt = kappa, theta, dt
        self.e = mpmath.exp(-kappa * dt)
        ome = 1 - self.e
        self.k1 = sigma * sigma * self.e * ome / kappa
        self.k2 = theta * sigma * sigma * ome * ome / (2 * kappa)
        self.rs = rho / sigma
        self.ktdt = kappa * theta * dt
        self.omr2 = 1 - rho * rho

    def step(self, v, u_v, z_v, z_s, st):
        """-> (v', the log-spot increment, quadratic?, v' = 0?)."""
        m = self.theta + (v - self.theta) * self.e
        s2 = v * self.k1 + self.k2
        psi = s2 / (m * m)
        st["psi_gap"] = min(st["psi_gap"], abs(psi - mpf(R.PSI_C)))
        quad, zero = psi <= mpf(R.PSI_C), False
        if quad:
            t = 2 / psi
            b2 = t - 1 + mpmath.sqrt(t) * mpmath.sqrt(t - 1)
            a = m / (1 + b2)
            bz = mpmath.sqrt(b2) + z_v
            vn = a * (bz * bz)
        else:
            p = (psi - 1) / (psi + 1)
            beta = (1 - p) / m
            st["u_gap"] = min(st["u_gap"], abs(u_v - p))
            zero = u_v <= p
            vn = mpf(0) if zero else mpmath.log((1 - p) / (1 - u_v)) / beta
        st["quad"] += quad
        st["expo"] += not quad
        st["zero"] += zero
        i_v = (v + vn) * self.dt / 2
        dx = (-i_v / 2 + self.rs * (vn - v - self.ktdt + self.kappa * i_v)
              + mpmath.sqrt(self.omr2 * i_v) * z_s)
        return vn, dx, quad, zero


def box_muller(u1, u2):
    rad = mpmath.sqrt(-2 * mpmath.log(u1))
    ang = mpf(R.TWO_PI) * u2
    return rad * mpmath.cos(ang), rad * mpmath.sin(ang)


def uniforms(seed, paths, step):
    """The ten uniforms of (seed, path, step) for every path, as float64 (exact): per block of the
    document's table, (words 0, 1) and (words 2, 3)."""
    lo, hi = paths & R.MASK, paths >> np.uint64(32)
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    out = []
    for b in range(5):
        w = R.philox4x32_10(lo, hi, np.uint64(step), np.uint64(b), k0, k1)
        out += [R.uniform(w[0], w[1]), R.uniform(w[2], w[3])]
    return out


def walk(params, st):
    """-> (truth [n_paths][3][6] of mpf, decisions [n_paths, n_steps, 5]: quadratic 1, zero 1,
    quadratic 2, zero 2, N)."""
    p = [mpf(float(v)) for v in params]
    dt = mpf(1) / R.TRUTH_SPY
    f1, f2 = FactorMP(p[1], p[2], p[3], p[4], dt), FactorMP(p[6], p[7], p[8], p[9], dt)
    lam, mu_j, sig_j = p[10], p[11], p[12]
    drift = (mpf(R.TRUTH_RATE) - lam * (mpmath.exp(mu_j + sig_j * sig_j / 2) - 1)) * dt
    cdf, pk = [mpmath.exp(-lam * dt)], mpmath.exp(-lam * dt)
    for k in range(1, R.POISSON_CAP):
        pk = pk * (lam * dt) / k
        cdf.append(cdf[-1] + pk)
    n, n_steps = R.TRUTH_PATHS.size, R.TRUTH_OBS[-1]
    us = [uniforms(R.TRUTH_SEED, R.TRUTH_PATHS, s) for s in range(1, n_steps + 1)]
    truth, dec = [], np.zeros((n, n_steps, 5), dtype=np.int64)
    for i in range(n):
        x, v1, v2, sm = mpf(0), p[0], p[5], mpf(0)
        mx = mn = None
        rows = []
        for step in range(1, n_steps + 1):
            u = [mpf(float(a[i])) for a in us[step - 1]]
            z_v, z_s = box_muller(u[2], u[3])
            v1, dx, dec[i, step - 1, 0], dec[i, step - 1, 1] = f1.step(v1, u[0], z_v, z_s, st)
            x += dx
            z_v, z_s = box_muller(u[4], u[5])
            v2, dx, dec[i, step - 1, 2], dec[i, step - 1, 3] = f2.step(v2, u[1], z_v, z_s, st)
            x += dx
            nj = sum(u[6] > c for c in cdf)
            st["u_gap"] = min(st["u_gap"], min(abs(u[6] - c) for c in cdf))
            st["n1"] += nj == 1
            st["n2"] += nj >= 2
            dec[i, step - 1, 4] = nj
            z_j, _ = box_muller(u[8], u[9])
            x += (drift + nj * mu_j) + (mpmath.sqrt(nj) * sig_j) * z_j
            s = mpf(R.TRUTH_SPOT) * mpmath.exp(x)
            mx = s if mx is None else max(mx, s)
            mn = s if mn is None else min(mn, s)
            sm += s
            if step in R.TRUTH_OBS:
                rows.append([s, v1, v2, mx, mn, sm])
        truth.append(rows)
    return truth, dec


def float64_decisions(params):
    """The same decisions as the float64 restatement takes them, and its gaps."""
    st = R.new_stats()
    st["trace"] = []
    R.simulate(params, R.TRUTH_SPOT, R.TRUTH_RATE, R.TRUTH_PATHS, R.TRUTH_OBS[-1], R.TRUTH_SPY,
               R.TRUTH_SEED, R.TRUTH_OBS, st)
    tr = np.stack([np.asarray(a, dtype=np.int64) for a in st.pop("trace")], axis=1)
    return tr.reshape(R.TRUTH_PATHS.size, R.TRUTH_OBS[-1], 5), st


def main():
    st = dict.fromkeys(COUNTS, 0)
    st["psi_gap"] = st["u_gap"] = mpf("inf")
    hi = np.empty((len(R.TRUTH_SETS), R.TRUTH_PATHS.size, len(R.TRUTH_OBS), 6))
    lo = np.empty_like(hi)
    for k, params in enumerate(R.TRUTH_SETS):
        truth, dec = walk(params, st)
        dec64, st64 = float64_decisions(params)
        if not np.array_equal(dec, dec64):
            sys.exit(f"set {k}: the mpmath and float64 decisions differ at (path, step, which) "
                     f"{np.argwhere(dec != dec64)[:5].tolist()}: pick other paths")
        if not (st64["psi_gap"] > MIN_GAP and st64["u_gap"] > MIN_GAP):
            sys.exit(f"set {k}: a float64 decision within {MIN_GAP} of its switch: {st64}")
        for i, rows in enumerate(truth):
            for j, row in enumerate(rows):
                for c, t in enumerate(row):
                    hi[k, i, j, c] = float(t)
                    lo[k, i, j, c] = float(t - mpf(float(t)))
        print(f"set {k}: walked; counts so far { {c: int(st[c]) for c in COUNTS} }")
    if not all(st[c] > 0 for c in COUNTS):
        sys.exit(f"a branch never occurs: { {c: int(st[c]) for c in COUNTS} }")
    if not (st["psi_gap"] > MIN_GAP and st["u_gap"] > MIN_GAP):
        sys.exit(f"a decision within {MIN_GAP} of its switch: psi {st['psi_gap']}, u {st['u_gap']}")
    rest = R.truth_restatement()
    rel, ab = R.truth_errors(rest, hi, lo)
    print("restatement against truth: worst relative error per statistic (S, v1, v2, max, min, "
          f"sum) {rel}, worst absolute error on v1, v2 {ab}")
    path = os.path.join(HERE, R.TRUTH_FILE)
    np.savez_compressed(
        path, truth=hi, truth_lo=lo, restatement=rest, rel_err=rel, abs_err=ab,
        paths=R.TRUTH_PATHS, seed=np.uint64(R.TRUTH_SEED), sets=R.TRUTH_SETS,
        steps_per_year=np.int64(R.TRUTH_SPY), obs_steps=np.array(R.TRUTH_OBS, dtype=np.int64),
        spot=np.float64(R.TRUTH_SPOT), rate=np.float64(R.TRUTH_RATE),
        count_names=np.array(COUNTS), counts=np.array([int(st[c]) for c in COUNTS]),
        psi_gap=np.float64(float(st["psi_gap"])), u_gap=np.float64(float(st["u_gap"])))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
