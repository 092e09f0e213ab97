"""NumPy restatement of the Monte Carlo scheme of DESIGN.md 3.15 (test infrastructure only).

Written from the document, not from the kernel: vectorised Philox4x32-10, the uniform and
Box-Muller maps, Andersen's QE variance step, the central-weight log-spot step, Poisson jumps by
inversion and the running statistics, each expression in the document's order.  Nothing in dhcos/
imports this module; the GPU tests compare the library's paths against it.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57         # Philox4x32 multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85         # Weyl key increments
MASK = np.uint64(0xFFFFFFFF)
POISSON_CAP = 16                        # CDF terms walked: N <= 16
PSI_C = 1.5                             # QE branch switch
TWO_PI = 6.283185307179586
KINDS = {"european": 0, "asian": 1, "up_and_out": 2, "down_and_out": 3}

README_PARAMS = np.array([0.04, 2.5, 0.04, 0.3, -0.7, 0.04, 0.8, 0.04, 0.2, -0.5, 0.15, -0.04,
                          0.08])
# the stressed set of the path-parity test: factor 1 far past the Feller bound, frequent jumps
STRESSED_PARAMS = np.array([0.01, 0.5, 0.02, 1.0, -0.7, 0.04, 0.8, 0.04, 0.2, -0.5, 2.0, -0.04,
                            0.08])
GRID_K = np.tile(np.array([90.0, 95.0, 100.0, 105.0, 110.0]), 3)
GRID_T = np.repeat(np.array([0.25, 0.5, 1.0]), 5)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds of Philox4x32 over arrays of 32-bit words (held in uint64) -> four words."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0 = np.uint64(k0) & MASK
    k1 = np.uint64(k1) & MASK
    for rnd in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1,
             p0 & MASK]
        if rnd < 9:
            k0 = (k0 + np.uint64(W0)) & MASK
            k1 = (k1 + np.uint64(W1)) & MASK
    return c


def uniform(w_hi, w_lo):
    """Two words -> a double strictly inside (0, 1): the odd 53-bit integer 2 k + 1, k the 52-bit
    number (w_hi >> 6) 2^26 + (w_lo >> 6), times 2^-53 (exact)."""
    k = ((w_hi >> np.uint64(6)) << np.uint64(26)) | (w_lo >> np.uint64(6))
    return (2.0 * k.astype(np.float64) + 1.0) * 2.0 ** -53


def box_muller(u1, u2):
    rad = np.sqrt(-2.0 * np.log(u1))
    ang = TWO_PI * u2
    return rad * np.cos(ang), rad * np.sin(ang)


def draws(seed, path, step):
    """The eight variates of (seed, path, step): U_v1, Z_v1, Z_s1, U_v2, Z_v2, Z_s2, U_N, Z_J."""
    path = np.asarray(path, dtype=np.uint64)
    lo, hi = path & MASK, path >> np.uint64(32)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    blk = [philox4x32_10(lo, hi, np.uint64(step), np.uint64(b), k0, k1) for b in range(5)]
    u_v1, u_v2 = uniform(blk[0][0], blk[0][1]), uniform(blk[0][2], blk[0][3])
    z_v1, z_s1 = box_muller(uniform(blk[1][0], blk[1][1]), uniform(blk[1][2], blk[1][3]))
    z_v2, z_s2 = box_muller(uniform(blk[2][0], blk[2][1]), uniform(blk[2][2], blk[2][3]))
    u_n = uniform(blk[3][0], blk[3][1])
    z_j, _ = box_muller(uniform(blk[4][0], blk[4][1]), uniform(blk[4][2], blk[4][3]))
    return u_v1, z_v1, z_s1, u_v2, z_v2, z_s2, u_n, z_j


class Factor:
    """One variance factor's constants at a time step dt."""

    def __init__(self, kappa, theta, sigma, rho, dt):
        self.kappa, self.theta = kappa, theta
        self.e = np.exp(-kappa * dt)
        ome = 1.0 - self.e
        self.k1 = sigma * sigma * self.e * ome / kappa
        self.k2 = theta * sigma * sigma * ome * ome / (2.0 * kappa)
        self.rs = rho / sigma
        self.ktdt = kappa * theta * dt
        self.omr2 = 1.0 - rho * rho
        self.dt = dt

    def step(self, v, u_v, z_v, z_s, stats=None):
        """-> (v', the log-spot increment)."""
        m = self.theta + (v - self.theta) * self.e
        s2 = v * self.k1 + self.k2
        psi = s2 / (m * m)
        quad = psi <= PSI_C
        with np.errstate(all="ignore"):
            t = 2.0 / psi
            b2 = t - 1.0 + np.sqrt(t) * np.sqrt(t - 1.0)
            a = m / (1.0 + b2)
            bz = np.sqrt(b2) + z_v
            vq = a * (bz * bz)
            p = (psi - 1.0) / (psi + 1.0)
            beta = (1.0 - p) / m
            ve = np.where(u_v <= p, 0.0, np.log((1.0 - p) / (1.0 - u_v)) / beta)
        vn = np.where(quad, vq, ve)
        if stats is not None:
            stats["quad"] += int(np.sum(quad))
            stats["expo"] += int(np.sum(~quad))
            stats["zero"] += int(np.sum(~quad & (u_v <= p)))
            stats["psi_gap"] = min(stats["psi_gap"], float(np.min(np.abs(psi - PSI_C))))
            if np.any(~quad):
                stats["u_gap"] = min(stats["u_gap"], float(np.min(np.abs(u_v - p)[~quad])))
            if "trace" in stats:
                stats["trace"] += [quad, ~quad & (u_v <= p)]
        i_v = 0.5 * (v + vn) * self.dt
        dx = (-0.5 * i_v + self.rs * (vn - v - self.ktdt + self.kappa * i_v)
              + np.sqrt(self.omr2 * i_v) * z_s)
        return vn, dx


def poisson_cdf(lam_dt):
    """cdf[k] = P(N <= k), k = 0 .. POISSON_CAP - 1, by the recurrence p_k = p_{k-1} lam_dt / k."""
    cdf = np.empty(POISSON_CAP)
    pk = np.exp(-lam_dt)
    acc = pk
    cdf[0] = acc
    for k in range(1, POISSON_CAP):
        pk = pk * lam_dt / k
        acc = acc + pk
        cdf[k] = acc
    return cdf


def new_stats():
    return {"quad": 0, "expo": 0, "zero": 0, "n1": 0, "n2": 0, "psi_gap": np.inf,
            "u_gap": np.inf}


def simulate(params, spot, rate, paths, n_steps, steps_per_year, seed, obs_steps=(), stats=None):
    """Walk the given path indices n_steps steps under one parameter set.

    -> (state, obs): state the six statistics [n, 6] (S, v1, v2, max, min, sum) after the last
    step, obs [n, len(obs_steps), 6] the same at the listed steps."""
    p = np.asarray(params, dtype=np.float64)
    paths = np.asarray(paths, dtype=np.uint64)
    dt = 1.0 / steps_per_year
    f1 = Factor(p[1], p[2], p[3], p[4], dt)
    f2 = Factor(p[6], p[7], p[8], p[9], dt)
    lam, mu_j, sig_j = p[10], p[11], p[12]
    lam_dt = lam * dt
    if lam_dt > 1.0:
        raise ValueError("lambda dt > 1")
    kbar = np.exp(mu_j + 0.5 * sig_j * sig_j) - 1.0
    drift = (rate - lam * kbar) * dt
    cdf = poisson_cdf(lam_dt)
    n = paths.size
    x = np.zeros(n)
    v1, v2 = np.full(n, p[0]), np.full(n, p[5])
    mx, mn, sm = np.full(n, -np.inf), np.full(n, np.inf), np.zeros(n)
    obs = np.empty((n, len(obs_steps), 6))
    s = np.full(n, float(spot))
    for step in range(1, n_steps + 1):
        u_v1, z_v1, z_s1, u_v2, z_v2, z_s2, u_n, z_j = draws(seed, paths, step)
        v1n, dx = f1.step(v1, u_v1, z_v1, z_s1, stats)
        x = x + dx
        v1 = v1n
        v2n, dx = f2.step(v2, u_v2, z_v2, z_s2, stats)
        x = x + dx
        v2 = v2n
        nj = np.sum(u_n[:, None] > cdf[None, :], axis=1).astype(np.float64)
        if stats is not None:
            stats["n1"] += int(np.sum(nj == 1))
            stats["n2"] += int(np.sum(nj >= 2))
            stats["u_gap"] = min(stats["u_gap"], float(np.min(np.abs(u_n[:, None] - cdf[None, :]))))
            if "trace" in stats:
                stats["trace"].append(nj)
        x = x + ((drift + nj * mu_j) + (np.sqrt(nj) * sig_j) * z_j)
        s = spot * np.exp(x)
        mx, mn, sm = np.maximum(mx, s), np.minimum(mn, s), sm + s
        for j, o in enumerate(obs_steps):
            if o == step:
                obs[:, j] = np.stack([s, v1, v2, mx, mn, sm], axis=1)
    return np.stack([s, v1, v2, mx, mn, sm], axis=1), obs


def payoff(kind, is_call, strike, barrier, n_steps, state):
    """Undiscounted payoff of one option from the statistics at its maturity step [n, 6]."""
    s, mx, mn, sm = state[:, 0], state[:, 3], state[:, 4], state[:, 5]
    under = sm / float(n_steps) if kind == "asian" else s
    pay = np.maximum(under - strike, 0.0) if is_call else np.maximum(strike - under, 0.0)
    if kind == "up_and_out":
        pay = np.where(mx < barrier, pay, 0.0)
    elif kind == "down_and_out":
        pay = np.where(mn > barrier, pay, 0.0)
    return pay


def price(params, spot, rate, options, n_paths, steps_per_year, seed, block=1 << 15):
    """Prices and standard errors of `options` (dicts: strike, maturity, option_type, optional
    kind / barrier) over paths 0 .. n_paths - 1, plus the discounted mean of S_T and its standard
    error per option maturity -> (price, stderr, forward, forward_stderr)."""
    steps = [int(round(o["maturity"] * steps_per_year)) for o in options]
    order = sorted(set(steps))
    sums = np.zeros((len(options), 2))
    fsum = {s: np.zeros(2) for s in order}
    for lo in range(0, n_paths, block):
        idx = np.arange(lo, min(n_paths, lo + block), dtype=np.uint64)
        _, obs = simulate(params, spot, rate, idx, order[-1], steps_per_year, seed, order)
        for j, (o, st) in enumerate(zip(options, steps)):
            pay = payoff(o.get("kind", "european"), o["option_type"].upper()[0] == "C",
                         o["strike"], o.get("barrier", 0.0), st, obs[:, order.index(st)])
            sums[j] += (pay.sum(), (pay * pay).sum())
        for st in order:
            sT = obs[:, order.index(st), 0]
            fsum[st] += (sT.sum(), (sT * sT).sum())
    n = float(n_paths)

    def finish(s1, s2, st):
        disc = np.exp(-rate * st / steps_per_year)
        return disc * s1 / n, disc * np.sqrt(max(s2 - s1 * s1 / n, 0.0) / (n * (n - 1.0)))

    pr = np.array([finish(sums[j, 0], sums[j, 1], steps[j]) for j in range(len(options))])
    fw = np.array([finish(fsum[st][0], fsum[st][1], st) for st in steps])
    return pr[:, 0], pr[:, 1], fw[:, 0], fw[:, 1]


# ---- the 50-digit truth fixture (tests/golden/make_mc_truth.py writes it) -------------------------
def _with(base, **kw):
    names = ["v01", "kappa1", "theta1", "sigma1", "rho1", "v02", "kappa2", "theta2", "sigma2",
             "rho2", "lambda_j", "mu_j", "sigma_j"]
    p = np.array(base, dtype=np.float64)
    for k, v in kw.items():
        p[names.index(k)] = v
    return p


# legal edges of the validation: both variances start at 0, no jumps, |rho| next to 1
ZERO_V0_PARAMS = _with(README_PARAMS, v01=0.0, v02=0.0, lambda_j=0.0, rho1=0.999, rho2=-0.999)
# lambda dt = 1 exactly at 8 steps per year (the Poisson walk's cap), jumps of one fixed size
CAP_JUMP_PARAMS = _with(README_PARAMS, lambda_j=8.0, mu_j=-0.04, sigma_j=0.0)
TRUTH_SETS = np.stack([README_PARAMS, STRESSED_PARAMS, ZERO_V0_PARAMS, CAP_JUMP_PARAMS])
TRUTH_SEED = 0x9E3779B900000005         # the key's high word is live
TRUTH_PATHS = np.array(list(range(24)) + list(range(1000, 1004))
                       + [(1 << 32) - 1, 1 << 32, (1 << 32) + 1, 5 * (1 << 32) + 77],
                       dtype=np.uint64)  # the counter's high word is 0, 1 and 5
TRUTH_SPY, TRUTH_OBS, TRUTH_SPOT, TRUTH_RATE = 8, (2, 4, 8), 100.0, 0.03
TRUTH_FILE = "mc_truth.npz"


def truth_restatement(stats=None):
    """This module's walk of the fixture's configuration -> [4, n_paths, 3, 6]."""
    return np.stack([simulate(p, TRUTH_SPOT, TRUTH_RATE, TRUTH_PATHS, TRUTH_OBS[-1], TRUTH_SPY,
                              TRUTH_SEED, TRUTH_OBS, stats)[1] for p in TRUTH_SETS])


def truth_errors(got, hi, lo):
    """got [..., 6] against the truth hi + lo (hi the truth rounded to double, lo the rounded
    remainder) -> (worst relative error per statistic [6], worst absolute error on v1, v2 [2]).
    got - hi is exact for neighbours, so the figures resolve far below an ulp without mpmath.
    Where the truth is an exact 0 the error counts as 0 if got is 0 too, as infinite if not."""
    d = np.abs((got - hi) - lo)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(hi == 0.0, np.where(got == 0.0, 0.0, np.inf), d / np.abs(hi))
    flat = (-1, 6)
    return rel.reshape(flat).max(axis=0), d.reshape(flat)[:, 1:3].max(axis=0)


# ---- the moments of the variance factors ---------------------------------------------------------
def cir_moments(v0, kappa, theta, sigma, T):
    """Mean and variance of a CIR process at T from v0 (see moment_z_scores)."""
    e = np.exp(-kappa * T)
    return (theta + (v0 - theta) * e,
            v0 * sigma * sigma / kappa * (e - e * e)
            + theta * sigma * sigma / (2.0 * kappa) * (1.0 - e) ** 2)


def moment_z_scores(params, state, spot, rate, T):
    """state [n, 6]: the statistics of n paths at time T -> {name: |sample - exact| / its
    standard error} for the mean and the variance of v1 and v2 and for the discounted mean of S.

    Why the exact figures are the CIR closed forms although the scheme is discrete: one QE step
    from v draws v' with E[v' | v] = m = theta + (v - theta) E and Var[v' | v] = s^2 = v K1 + K2
    in either branch (quadratic: a (1 + b^2) = m and 2 a^2 (1 + 2 b^2) = s^2 by the choice of b^2;
    exponential: (1 - p) / beta = m and (1 - p^2) / beta^2 = s^2), and those are the exact
    conditional moments of the CIR process over dt, E = e^{-kappa dt}.  Both are linear in v, so
    the towers E[v'] = theta + (E[v] - theta) E and Var[v'] = K1 E[v] + K2 + E^2 Var[v] close on
    the first two moments, the exact process obeys the same recursion, and after n steps both give
        E = theta + (v0 - theta) e^{-kappa T},
        Var = v0 sigma^2 / kappa (e^{-kappa T} - e^{-2 kappa T})
              + theta sigma^2 / (2 kappa) (1 - e^{-kappa T})^2,   T = n dt.
    The standard error of the sample variance s^2 is sqrt((m4 - s^4) / n), m4 the sample's own
    fourth central moment.  None of this passes through the restatement of the step."""
    p = np.asarray(params, dtype=np.float64)
    n = state.shape[0]
    z = {}
    for i, col in ((0, 1), (1, 2)):
        v = state[:, col]
        mean, var = cir_moments(p[5 * i], p[5 * i + 1], p[5 * i + 2], p[5 * i + 3], T)
        c = v - v.mean()
        s2 = np.sum(c * c) / (n - 1.0)
        m4 = np.mean(c ** 4)
        z[f"mean v{i + 1}"] = abs(v.mean() - mean) / np.sqrt(s2 / n)
        z[f"var v{i + 1}"] = abs(s2 - var) / np.sqrt((m4 - s2 * s2) / n)
    d = np.exp(-rate * T) * state[:, 0]
    z["forward"] = abs(d.mean() - spot) / (d.std(ddof=1) / np.sqrt(n))
    return z
