"""NumPy restatement of the variance reduction of DESIGN.md 3.15.2 (test infrastructure only).

The draws, the factor step, the Poisson table and the payoffs are mc_reference's; this module
mirrors the draws, walks a path or its mirror, forms the samples and their controls, and states
the estimator.  Nothing in dhcos/ imports it.
"""
import math
from fractions import Fraction

import numpy as np

import mc_reference as R

ANTITHETIC, CONTROL = 1, 2
COS_N, COS_L = 256, 10.0


def mirror_uniform(u):
    """1 - U: exact, and again an odd multiple of 2^-53 inside (0, 1)."""
    return 1.0 - u


def draws(seed, path, step, mirror=False):
    """mc_reference.draws, or their mirror: the uniforms 1 - U, the normals -Z."""
    u_v1, z_v1, z_s1, u_v2, z_v2, z_s2, u_n, z_j = R.draws(seed, path, step)
    if not mirror:
        return u_v1, z_v1, z_s1, u_v2, z_v2, z_s2, u_n, z_j
    return (mirror_uniform(u_v1), -z_v1, -z_s1, mirror_uniform(u_v2), -z_v2, -z_s2,
            mirror_uniform(u_n), -z_j)


def simulate(params, spot, rate, paths, n_steps, steps_per_year, seed, obs_steps=(), mirror=False,
             stats=None):
    """mc_reference.simulate with a mirror switch -> (state [n, 6], obs [n, len(obs_steps), 6])."""
    p = np.asarray(params, dtype=np.float64)
    paths = np.asarray(paths, dtype=np.uint64)
    dt = 1.0 / steps_per_year
    f1 = R.Factor(p[1], p[2], p[3], p[4], dt)
    f2 = R.Factor(p[6], p[7], p[8], p[9], dt)
    lam, mu_j, sig_j = p[10], p[11], p[12]
    kbar = np.exp(mu_j + 0.5 * sig_j * sig_j) - 1.0
    drift = (rate - lam * kbar) * dt
    cdf = R.poisson_cdf(lam * dt)
    n = paths.size
    x = np.zeros(n)
    v1, v2 = np.full(n, p[0]), np.full(n, p[5])
    mx, mn, sm = np.full(n, -np.inf), np.full(n, np.inf), np.zeros(n)
    s = np.full(n, float(spot))
    obs = np.empty((n, len(obs_steps), 6))
    for step in range(1, n_steps + 1):
        u_v1, z_v1, z_s1, u_v2, z_v2, z_s2, u_n, z_j = draws(seed, paths, step, mirror)
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
        x = x + ((drift + nj * mu_j) + (np.sqrt(nj) * sig_j) * z_j)
        s = spot * np.exp(x)
        mx, mn, sm = np.maximum(mx, s), np.minimum(mn, s), sm + s
        for j, o in enumerate(obs_steps):
            if o == step:
                obs[:, j] = np.stack([s, v1, v2, mx, mn, sm], axis=1)
    return np.stack([s, v1, v2, mx, mn, sm], axis=1), obs


def has_twin(option):
    """True where the control is the European twin (mean: its COS price), False where it is S at
    the maturity step (mean: spot)."""
    return option.get("kind", "european") != "european" and option["strike"] != 0.0


def is_call(option):
    return option["option_type"].upper()[0] == "C"


def sample_and_control(option, n_steps, state, mirror_state=None):
    """(y, c) of one option from the statistics [n, 6] of the paths at its maturity step and, for
    antithetic pairs, of their mirrors: the payoff and the control, averaged over the pair."""
    def one(st):
        y = R.payoff(option.get("kind", "european"), is_call(option), option["strike"],
                     option.get("barrier", 0.0), n_steps, st)
        c = (R.payoff("european", is_call(option), option["strike"], 0.0, n_steps, st)
             if has_twin(option) else st[:, 0])
        return y, c
    y, c = one(state)
    if mirror_state is not None:
        ym, cm = one(mirror_state)
        y, c = 0.5 * (y + ym), 0.5 * (c + cm)
    return y, c


def five_sums(y, c):
    """sum y, y^2, c, c^2, y c, each correctly rounded (the products are rounded doubles)."""
    return tuple(math.fsum(v) for v in (y, y * y, c, c * c, y * c))


def estimator(sums, n, disc, mean, control=True, exact=False):
    """The finish of 3.15.2 on the five sums of n samples -> dict(price, stderr, base_price,
    base_stderr, beta).  exact: the arithmetic in rationals, rounded once at the end (and once
    inside each square root); else in doubles, in the document's order."""
    num = Fraction if exact else float
    sy, syy, sc, scc, syc = (num(v) for v in sums)
    n, disc = num(n), num(disc)
    cyy = syy - sy * sy / n
    base_price = disc * sy / n
    root = lambda v: math.sqrt(max(v, num(0)) / (n * (n - 1)))    # noqa: E731
    base_stderr = float(disc) * root(cyy)
    beta, price, stderr = num(0), base_price, base_stderr
    if control:
        ccc = scc - sc * sc / n
        cyc = syc - sy * sc / n
        beta = cyc / ccc if ccc > 0 else num(0)
        price = base_price - beta * (disc * sc / n - num(mean))
        stderr = float(disc) * root(cyy - beta * cyc)
    return {"price": float(price), "stderr": float(stderr), "base_price": float(base_price),
            "base_stderr": float(base_stderr), "beta": float(beta)}


def price(params, spot, rate, options, n_paths, steps_per_year, seed, flags, means,
          block=1 << 14):
    """The whole estimator on the restatement's own paths: n_paths walks (n_paths / 2 pairs under
    ANTITHETIC), means[j] the known mean of option j's control -> a list of estimator() dicts."""
    anti, ctrl = bool(flags & ANTITHETIC), bool(flags & CONTROL)
    n = n_paths // 2 if anti else n_paths
    steps = [int(round(o["maturity"] * steps_per_year)) for o in options]
    order = sorted(set(steps))
    sums = np.zeros((len(options), 5))
    for lo in range(0, n, block):
        idx = np.arange(lo, min(n, lo + block), dtype=np.uint64)
        _, obs = simulate(params, spot, rate, idx, order[-1], steps_per_year, seed, order)
        mobs = simulate(params, spot, rate, idx, order[-1], steps_per_year, seed, order,
                        mirror=True)[1] if anti else None
        for j, (o, st) in enumerate(zip(options, steps)):
            k = order.index(st)
            y, c = sample_and_control(o, st, obs[:, k], None if mobs is None else mobs[:, k])
            sums[j] += five_sums(y, c)
    return [estimator(sums[j], n, math.exp(-rate * o["maturity"]), means[j], ctrl)
            for j, o in enumerate(options)]
