"""NumPy restatement of the coupled-path Greeks of DESIGN.md 3.15.3 (test infrastructure only).

Written from the document on top of tests/mc_reference.py, which it imports and does not change:
``simulate`` walks the base record and the four records with a bumped ``v0`` (the same seed and path
indices, hence the same draws; the other factor and the jumps come out as the base path's because
they do not read the bumped ``v0``), the statistics of the spot bumps are the base path's times
``1 +- eps``, and the samples, sums, values and standard errors follow the document's formulas.
Nothing in dhcos/ imports this module.
"""
import numpy as np

import mc_reference as R

NAMES = ("price", "delta", "gamma", "vega_v01", "vega_v02")     # the DH_MC_GREEK_* planes


def bumped_sets(params, v0_bump):
    """[5, 13]: the base set, then v0_1 + d_1, v0_1 - d_1, v0_2 + d_2, v0_2 - d_2 (d_j = b v0_j)."""
    p = np.asarray(params, dtype=np.float64)
    sets = np.tile(p, (5, 1))
    for k, (col, sign) in enumerate(((0, 1.0), (0, -1.0), (5, 1.0), (5, -1.0)), start=1):
        d = v0_bump * p[col]
        sets[k, col] = p[col] + d if sign > 0 else p[col] - d
    return sets


def scaled(state, u):
    """The statistics [n, 6] of the path at spot S0 u: S, max, min and sum each times u."""
    out = np.array(state, dtype=np.float64)
    for col in (0, 3, 4, 5):
        out[:, col] = u * state[:, col]
    return out


def samples(states, params, spot, option, step, spot_bump, v0_bump):
    """states [5, n, 6]: the statistics at the option's maturity step of the base path and of the
    four bumped-v0 paths (the order of bumped_sets) -> the five samples [5, n] of every path."""
    p = np.asarray(params, dtype=np.float64)
    h = spot_bump * spot
    up, um = 1.0 + spot_bump, 1.0 - spot_bump
    d1, d2 = v0_bump * p[0], v0_bump * p[5]

    def pay(state):
        return R.payoff(option.get("kind", "european"), option["option_type"].upper()[0] == "C",
                        option["strike"], option.get("barrier", 0.0), step, state)

    y, ysp, ysm = pay(states[0]), pay(scaled(states[0], up)), pay(scaled(states[0], um))
    return np.stack([y,
                     (ysp - ysm) / (2.0 * h),
                     ((ysp - y) + (ysm - y)) / (h * h),
                     (pay(states[1]) - pay(states[2])) / (2.0 * d1),
                     (pay(states[3]) - pay(states[4])) / (2.0 * d2)])


def finish(s1, s2, n, disc):
    """value and stderr of sums s1 = sum g, s2 = sum g^2 over n paths."""
    n = float(n)
    return disc * s1 / n, disc * np.sqrt(np.maximum(s2 - s1 * s1 / n, 0.0) / (n * (n - 1.0)))


def from_states(states, obs_steps, params, spot, rate, options, steps_per_year, spot_bump, v0_bump):
    """states [5, n, n_obs, 6] at obs_steps -> (value [n_options, 5], stderr [n_options, 5], the
    mean absolute sample [n_options, 5])."""
    n = states.shape[1]
    obs_steps = list(obs_steps)
    value, err, mean_abs = (np.empty((len(options), 5)) for _ in range(3))
    for j, o in enumerate(options):
        st = int(round(o["maturity"] * steps_per_year))
        g = samples(states[:, :, obs_steps.index(st)], params, spot, o, st, spot_bump, v0_bump)
        disc = np.exp(-rate * o["maturity"])
        value[j], err[j] = finish(g.sum(axis=1), (g * g).sum(axis=1), n, disc)
        mean_abs[j] = disc * np.abs(g).mean(axis=1)
    return value, err, mean_abs


def greeks(params, spot, rate, options, n_paths, steps_per_year, seed, spot_bump, v0_bump,
           block=1 << 15):
    """value, stderr [n_options, 5] (the planes of NAMES) of `options` (dicts as
    mc_reference.price) over paths 0 .. n_paths - 1."""
    steps = [int(round(o["maturity"] * steps_per_year)) for o in options]
    order = sorted(set(steps))
    sets = bumped_sets(params, v0_bump)
    s1, s2 = np.zeros((len(options), 5)), np.zeros((len(options), 5))
    for lo in range(0, n_paths, block):
        idx = np.arange(lo, min(n_paths, lo + block), dtype=np.uint64)
        states = np.stack([R.simulate(p, spot, rate, idx, order[-1], steps_per_year, seed, order)[1]
                           for p in sets])
        for j, (o, st) in enumerate(zip(options, steps)):
            g = samples(states[:, :, order.index(st)], params, spot, o, st, spot_bump, v0_bump)
            s1[j] += g.sum(axis=1)
            s2[j] += (g * g).sum(axis=1)
    disc = np.exp(-rate * np.array([o["maturity"] for o in options]))[:, None]
    return finish(s1, s2, n_paths, disc)


def cos_differences(price_fn, params, spot, spot_bump, v0_bump):
    """Central differences, at the estimator's own steps, of a pricing function price_fn(params,
    spot) -> [n_options]: (delta, gamma, vega_v01, vega_v02), each [n_options]."""
    p = np.asarray(params, dtype=np.float64)
    h = spot_bump * spot
    base = price_fn(p, spot)
    up, dn = price_fn(p, spot * (1.0 + spot_bump)), price_fn(p, spot * (1.0 - spot_bump))
    sets = bumped_sets(p, v0_bump)
    d1, d2 = v0_bump * p[0], v0_bump * p[5]
    return ((up - dn) / (2.0 * h), ((up - base) + (dn - base)) / (h * h),
            (price_fn(sets[1], spot) - price_fn(sets[2], spot)) / (2.0 * d1),
            (price_fn(sets[3], spot) - price_fn(sets[4], spot)) / (2.0 * d2))


# ---- the statistical case (tests/test_mc_greeks.py vets it on the CPU; the GPU test runs it too) --
STAT_PARAMS = R.README_PARAMS
STAT_SPOT, STAT_RATE = 100.0, 0.03
STAT_SPY, STAT_PATHS, STAT_SEED = 32, 1 << 16, 2024
STAT_SPOT_BUMP, STAT_V0_BUMP = 1e-2, 5e-2
STAT_OPTIONS = [{"strike": float(k), "maturity": float(t), "option_type": ty}
                for t in (0.125, 0.25, 0.5) for k, ty in ((95.0, "put"), (100.0, "call"),
                                                          (105.0, "call"))]
