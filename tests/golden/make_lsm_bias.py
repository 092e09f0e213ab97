"""Writes tests/golden/lsm_bias.json: the in-sample bias of the least-squares Monte Carlo method in
the Black-Scholes limit, as the NumPy restatement (tests/lsm_reference.py) shows it.

    python tests/golden/make_lsm_bias.py

Puts at lsm_reference.BS_STRIKES on mc_reference's paths of the model with v0 = theta and
sigma = 1e-3 in both factors and no jumps (total variance 0.04), 8 exercise dates in one year,
2^15 paths, over the 8 seeds BS_FIT_SEEDS.  Per strike: the Cox-Ross-Rubinstein Bermudan and
European values, the mean of LSM - tree over the seeds, and the largest |LSM - tree| / stderr.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import lsm_reference as L  # noqa: E402


def main():
    tree = L.bs_tree()
    runs = [L.bs_restatement(seed) for seed in L.BS_FIT_SEEDS]
    price = np.array([r["price"] for r in runs])           # [seeds, strikes]
    err = np.array([r["stderr"] for r in runs])
    berm = np.array([t[0] for t in tree])
    out = {"spot": L.BS_SPOT, "rate": L.BS_RATE, "sigma": L.BS_SIGMA, "maturity": L.BS_T,
           "dates": L.BS_DATES, "steps_per_year": L.BS_SPY, "n_paths": L.BS_PATHS,
           "seeds": list(L.BS_FIT_SEEDS), "tree_steps_per_date": L.BS_TREE_STEPS,
           "strikes": list(L.BS_STRIKES), "tree": berm.tolist(),
           "tree_european": [t[1] for t in tree],
           "mean_bias": (price - berm).mean(axis=0).tolist(),
           "max_z": (np.abs(price - berm) / err).max(axis=0).tolist()}
    with open(os.path.join(HERE, L.BIAS_FILE), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
