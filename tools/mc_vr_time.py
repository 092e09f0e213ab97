"""Times the path pricer's variance reduction against the plain pricer, at equal walks.

    python tools/mc_vr_time.py [--paths 1048576] [--steps-per-year 64] [--out profiles/mc_vr_time.json]

The workload of tools/mc_time.py (the generator's 15 calls, P = 1 and P = 64 parameter sets, host
arrays in and out, wall clock, median of 7 calls after 2 warm-up calls) for dhcos.monte_carlo plain
and with antithetic, control_variate and both, the four taken in turn inside every repetition so
that drift of the machine falls on all alike.  ``paths`` counts walks: the antithetic runs walk
paths / 2 pairs.  Per combination: the time, the time relative to plain, each option's
variance_ratio (what the control removed from the same samples), and time x stderr^2 relative to
plain -- the cost of equal accuracy, below 1 where the method pays.  Then each option's
variance_ratio for a table of all four kinds at 2^17 walks.  Needs a gfx950 device.
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
COMBOS = {"plain": {}, "antithetic": {"antithetic": True}, "control": {"control_variate": True},
          "both": {"antithetic": True, "control_variate": True}}


def mixed_table():
    """Asian, up-and-out (H = 125) and down-and-out (H = 85) calls and puts at three strikes, and
    three European calls, T = 0.5."""
    table = [dict({"strike": k, "maturity": 0.5, "option_type": ot, "kind": kind},
                  **({"barrier": h} if h else {}))
             for kind, h in (("asian", None), ("up_and_out", 125.0), ("down_and_out", 85.0))
             for ot in ("call", "put") for k in (90.0, 100.0, 110.0)]
    return table + [{"strike": k, "maturity": 0.5, "option_type": "call"}
                    for k in (90.0, 100.0, 110.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=1 << 20)
    ap.add_argument("--steps-per-year", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import dhcos
    from dhcos import _native
    if _native.device_count() == 0:
        raise SystemExit("mc_vr_time: no gfx950 device (nothing is timed on the CPU)")
    options = [{"strike": float(k), "maturity": t, "option_type": "call"}
               for t in (0.25, 0.5, 1.0) for k in (90, 95, 100, 105, 110)]
    res = {"paths": a.paths, "steps_per_year": a.steps_per_year, "options": len(options),
           "reps": a.reps}
    for P in (1, 64):
        sets = README if P == 1 else LO + (HI - LO) * np.random.RandomState(0).rand(P, 13)
        times = {name: [] for name in COMBOS}
        last = {}
        for i in range(a.reps + 2):
            for name, kw in COMBOS.items():
                t0 = time.perf_counter()
                last[name] = dhcos.monte_carlo(sets, 100.0, 0.03, options, n_paths=a.paths,
                                               steps_per_year=a.steps_per_year, seed=i, **kw)
                times[name].append(time.perf_counter() - t0)
        med = {name: float(np.median(t[2:])) for name, t in times.items()}
        row = {}
        for name in COMBOS:
            out = last[name]
            assert np.all(np.isfinite(out.price)) and np.all(out.stderr > 0)
            t = np.array(times[name][2:])
            cost = med[name] * out.stderr ** 2 / (med["plain"] * last["plain"].stderr ** 2)
            row[name] = {"wall_ms_median": med[name] * 1e3, "wall_ms_min": t.min() * 1e3,
                         "wall_ms_max": t.max() * 1e3, "time_vs_plain": med[name] / med["plain"],
                         "cost_of_equal_accuracy_vs_plain": np.atleast_2d(cost).mean(0).tolist()}
            if name != "plain":
                row[name]["variance_ratio"] = np.atleast_2d(out.variance_ratio).mean(0).tolist()
        res[f"P{P}"] = row
    table = mixed_table()
    mixed = {"walks": 1 << 17, "steps_per_year": a.steps_per_year,
             "options": [f"{o.get('kind', 'european')} {o['option_type']} K={o['strike']:g}"
                         for o in table]}
    plain = dhcos.monte_carlo(README, 100.0, 0.03, table, n_paths=1 << 17,
                              steps_per_year=a.steps_per_year, seed=1)
    for name, kw in COMBOS.items():
        if name == "plain":
            continue
        out = dhcos.monte_carlo(README, 100.0, 0.03, table, n_paths=1 << 17,
                                steps_per_year=a.steps_per_year, seed=1, **kw)
        mixed[name] = {"variance_ratio": out.variance_ratio.tolist(),
                       "stderr2_vs_plain_at_equal_walks": ((out.stderr / plain.stderr) ** 2).tolist()}
    res["mixed"] = mixed
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
