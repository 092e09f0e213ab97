"""Times the least-squares Monte Carlo pricer on the generator's 15 strikes and maturities.

    python tools/lsm_time.py [--paths 131072] [--steps-per-year 64] [--out profiles/lsm_time.json]

dhcos.american_monte_carlo (host arrays in and out: copies, the path launch, one backward launch
per exercise date, the finishing launch, one synchronisation) on the 15 options as American puts
(exercise at every step), and dhcos.monte_carlo on the same options as European puts with the same
paths and steps, at P = 1 and P = 64 parameter sets: wall clock, each quantity the median of 7
calls after 2 warm-up calls, and the ratio of the two medians.  Needs a gfx950 device.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  before the first libdhcos call: one HIP runtime (dhcos/_native.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "option-pricing-ffn-lbfgs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

README = np.array([0.04, 2.5, 0.04, 0.3, -0.7, 0.04, 0.8, 0.04, 0.2, -0.5, 0.15, -0.04, 0.08])
LO = np.array([0.025, 1.5, 0.025, 0.2, -0.85, 0.02, 0.3, 0.025, 0.1, -0.7, 0.05, -0.08, 0.03])
HI = np.array([0.08, 4.5, 0.065, 0.5, -0.4, 0.07, 1.2, 0.07, 0.35, -0.2, 0.25, -0.01, 0.12])


def _median_ms(fn, reps):
    times = []
    for i in range(reps + 2):
        t0 = time.perf_counter()
        out = fn(i)
        times.append(time.perf_counter() - t0)
    t = np.array(times[2:]) * 1e3
    return out, {"wall_ms_median": float(np.median(t)), "wall_ms_min": float(t.min()),
                 "wall_ms_max": float(t.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=1 << 17)
    ap.add_argument("--steps-per-year", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import dhcos
    from dhcos import _native
    if _native.device_count() == 0:
        raise SystemExit("lsm_time: no gfx950 device (nothing is timed on the CPU)")
    options = [{"strike": float(k), "maturity": t, "option_type": "put"}
               for t in (0.25, 0.5, 1.0) for k in (90, 95, 100, 105, 110)]
    res = {"paths": a.paths, "steps_per_year": a.steps_per_year, "exercise_every": 1,
           "options": len(options), "reps": a.reps}
    for P in (1, 64):
        sets = README if P == 1 else LO + (HI - LO) * np.random.RandomState(0).rand(P, 13)
        kw = dict(n_paths=a.paths, steps_per_year=a.steps_per_year)
        am, t_am = _median_ms(lambda i: dhcos.american_monte_carlo(sets, 100.0, 0.03, options,
                                                                   seed=i, **kw), a.reps)
        eu, t_eu = _median_ms(lambda i: dhcos.monte_carlo(sets, 100.0, 0.03, options, seed=i,
                                                          **kw), a.reps)
        assert np.all(np.isfinite(am.price)) and np.all(am.stderr > 0)
        # the same seed, paths and steps: the European values of the two pricers agree
        assert np.allclose(am.european, eu.price, rtol=a.paths * 2.3e-16, atol=0)
        assert np.all(am.premium > -4 * am.stderr)
        res[f"P{P}"] = {"lsm": t_am, "european_mc": t_eu,
                        "ratio": t_am["wall_ms_median"] / t_eu["wall_ms_median"],
                        "path_steps": P * a.paths * a.steps_per_year,
                        "mean_premium": float(np.mean(am.premium))}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
