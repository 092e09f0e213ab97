"""Times calibrate_batch(objective="iv") against the price objective on the same markets and against
the host-driven loop that was the only vol-space route before it.

    python tools/batch_iv_calibrate_time.py [--sizes 1,256,4096] [--reps 7]
                                            [--out profiles/batch_iv_calibrate_time.json]

Markets: generate_synthetic_calibrations(max B, as_arrays=True, implied_vols=True) under
np.random.seed(0) -- the generator's 15-option grid, N = 128, a spot per market; the vols fitted are
its ``market_iv`` column, with weight 0 where a noisy market price has no vol and 1 elsewhere.
Every market gets one warm start: its true parameters x (1 + 5% noise), maxiter = 300.
Per B, wall times (median of `reps` runs after one warm-up run):
  * dhcos.calibrate_batch(..., objective="iv", market_ivs=, iv_weights=) over the first B markets;
  * dhcos.calibrate_batch(...) -- the price objective -- over the same markets and starts;
  * the loop
        DoubleHestonJumpCalibrator(spot_b, r, options_b, objective="iv", market_ivs=, iv_weights=)
            .calibrate(300, x0s=[x0_b], driver="scipy")
    over min(B, 32) markets, scaled linearly to B.
Needs a gfx950 device.
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

LOOP_MAX = 32


def timed(run, reps):
    run()                                              # warm-up: allocations, first launches
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        run()
        ts.append(time.perf_counter() - t0)
    return {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,256,4096")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--maxiter", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import dhcos
    from dhcos import _native
    from dhcos.generator import MATURITIES, STRIKES_PCT
    if _native.device_count() == 0:
        raise SystemExit("batch_iv_calibrate_time: no gfx950 device (nothing is timed on the CPU)")
    sizes = [int(s) for s in a.sizes.split(",")]
    nmax = max(sizes)
    np.random.seed(0)
    g = dhcos.generate_synthetic_calibrations(nmax, None, as_arrays=True, verbose=False,
                                              implied_vols=True)
    mkt, spots, r = g["market_prices"], g["spot"], float(g["risk_free"])
    ivs = np.ascontiguousarray(g["market_iv"], dtype=np.float64)
    wts = (np.isfinite(ivs) & (ivs >= 0)).astype(np.float64)
    cal0 = dhcos.DoubleHestonJumpCalibrator(100.0, r, [])
    rs = np.random.RandomState(1)
    X = np.empty((nmax, 1, 13))
    for b in range(nmax):
        true = dict(zip(cal0.param_names, g["params"][b] * (1 + 0.05 * rs.randn(13))))
        X[b, 0] = cal0.inverse_transform_params(true)
    krel = np.tile(STRIKES_PCT, len(MATURITIES)).astype(float)
    T = np.repeat(MATURITIES, len(STRIKES_PCT)).astype(float)

    def options(b):
        return [{"strike": float(k * spots[b] / 100.0), "maturity": float(t), "price": float(p),
                 "option_type": "call"} for k, t, p in zip(krel, T, mkt[b])]

    rows = []
    for B in sizes:
        out = {}

        def batch_iv():
            out["iv"] = dhcos.calibrate_batch(mkt[:B], spots[:B], r, x0s=X[:B],
                                              maxiter=a.maxiter, objective="iv",
                                              market_ivs=ivs[:B], iv_weights=wts[:B])

        def batch_price():
            out["price"] = dhcos.calibrate_batch(mkt[:B], spots[:B], r, x0s=X[:B],
                                                 maxiter=a.maxiter)

        nl = min(B, LOOP_MAX)
        opts = [options(b) for b in range(nl)]

        def loop():
            out["loop"] = [dhcos.DoubleHestonJumpCalibrator(float(spots[b]), r, opts[b],
                                                            objective="iv", market_ivs=ivs[b],
                                                            iv_weights=wts[b])
                           .calibrate(a.maxiter, x0s=[X[b, 0]], driver="scipy")
                           for b in range(nl)]

        t_iv = timed(batch_iv, a.reps)
        t_price = timed(batch_price, a.reps)
        t_loop = timed(loop, a.reps)
        iv, price = out["iv"], out["price"]
        scaled = t_loop["median"] * B / nl
        row = {"markets": B, "starts_per_market": 1, "maxiter": a.maxiter, "reps": a.reps,
               "zero_weight_options": int((wts[:B] == 0).sum()),
               "batch_iv_seconds": t_iv,
               "batch_price_seconds": t_price,
               "iv_over_price": t_iv["median"] / t_price["median"],
               "loop_markets_timed": nl,
               "scipy_iv_loop_seconds": t_loop,
               "scipy_iv_loop_seconds_scaled_to_markets": scaled,
               "loop_over_batch_iv": scaled / t_iv["median"],
               "batch_iv_iterations_enqueued": int(iv.iterations_enqueued),
               "batch_iv_requests": int(iv.nfev.sum()),
               "batch_iv_converged": int(iv.success.sum()),
               "batch_iv_median_final_loss": float(np.median(iv.final_loss)),
               "batch_price_iterations_enqueued": int(price.iterations_enqueued),
               "batch_price_requests": int(price.nfev.sum()),
               "loop_converged": int(sum(q.success for q in out["loop"])),
               "loop_median_final_loss": float(np.median([q.final_loss for q in out["loop"]]))}
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
