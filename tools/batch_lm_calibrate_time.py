"""Times calibrate_batch(method="lm") against the analytic-gradient L-BFGS-B on the same markets, and
that L-BFGS-B of this build against a parent build's.

    python tools/batch_lm_calibrate_time.py [--sizes 1,256,4096] [--reps 7]
                                            [--parent-root DIR]
                                            [--out profiles/batch_lm_calibrate_time.json]

Markets: generate_synthetic_calibrations(max B, as_arrays=True) under np.random.seed(0) -- the
generator's 15-option grid, N = 128, a spot per market.  Every market gets one warm start: its true
parameters x (1 + 5% noise), maxiter = 300.

Every figure comes from fresh processes, alternating between the sides: per B and repetition one
process runs method="lm", the next gradient="analytic" on this build and, with --parent-root DIR (a
built checkout of the parent commit), the next gradient="analytic" from DIR.  A process draws the
markets, runs the call once to warm up and then times it `--inner` times; its figure is the median
of those.  The recorded time is the median over the `--reps` processes, with their minimum and
maximum.  Per side also: iterations enqueued, requests per start, the share of starts that stop on
a tolerance, the median final loss.  With the parent, each row records the parent's own run-to-run
spread (max - min over its processes) and whether this build's L-BFGS-B median lies within it.
Needs a gfx950 device.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(a):
    """One process: markets, warm-up, `inner` timed calls -> one JSON line."""
    import time

    import numpy as np
    import torch  # noqa: F401  before the first libdhcos call: one HIP runtime (dhcos/_native.py)
    for p in (a.root, os.path.join(a.root, "option-pricing-ffn-lbfgs_amd")):
        sys.path.insert(0, p)
    import dhcos
    from dhcos import _native
    if _native.device_count() == 0:
        raise SystemExit("batch_lm_calibrate_time: no gfx950 device (nothing is timed on the CPU)")
    np.random.seed(0)
    g = dhcos.generate_synthetic_calibrations(a.nmax, None, as_arrays=True, verbose=False)
    mkt, spots, r = g["market_prices"], g["spot"], float(g["risk_free"])
    cal0 = dhcos.DoubleHestonJumpCalibrator(100.0, r, [])
    rs = np.random.RandomState(1)
    X = np.empty((a.nmax, 1, 13))
    for b in range(a.nmax):
        true = dict(zip(cal0.param_names, g["params"][b] * (1 + 0.05 * rs.randn(13))))
        X[b, 0] = cal0.inverse_transform_params(true)
    B = a.child
    kw = {"method": "lm"} if a.side == "lm" else {"gradient": "analytic"}

    def run():
        return dhcos.calibrate_batch(mkt[:B], spots[:B], r, x0s=X[:B], maxiter=a.maxiter, **kw)

    run()
    ts = []
    for _ in range(a.inner):
        t0 = time.perf_counter()
        res = run()
        ts.append(time.perf_counter() - t0)
    print(json.dumps({"seconds": float(np.median(ts)),
                      "iterations_enqueued": int(res.iterations_enqueued),
                      "requests_per_start": float(np.mean(res.nfev)),
                      "median_requests": float(np.median(res.nfev)),
                      "tolerance_stop_share": float(np.mean(res.status == 0)),
                      "median_final_loss": float(np.median(res.final_loss))}), flush=True)


def spawn(a, root, B, side):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(B), "--side", side, "--root",
           root, "--nmax", str(a.nmax), "--maxiter", str(a.maxiter), "--inner", str(a.inner)]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout
    return json.loads(out.strip().splitlines()[-1])


def summary(runs):
    import numpy as np
    ts = [q["seconds"] for q in runs]
    last = runs[-1]
    return {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts)),
            **{k: last[k] for k in last if k != "seconds"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,256,4096")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--maxiter", type=int, default=300)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", type=int, default=0)
    ap.add_argument("--side", default="lm")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--nmax", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        return child(a)
    sizes = [int(s) for s in a.sizes.split(",")]
    a.nmax = max(sizes)
    parent_root = os.path.abspath(a.parent_root) if a.parent_root else None
    rows = []
    for B in sizes:
        runs = {"lm": [], "lbfgs_analytic": [], "parent_lbfgs_analytic": []}
        for _ in range(a.reps):
            runs["lm"].append(spawn(a, ROOT, B, "lm"))
            runs["lbfgs_analytic"].append(spawn(a, ROOT, B, "lbfgs"))
            if parent_root:
                runs["parent_lbfgs_analytic"].append(spawn(a, parent_root, B, "lbfgs"))
        lm, lb = summary(runs["lm"]), summary(runs["lbfgs_analytic"])
        row = {"markets": B, "starts_per_market": 1, "maxiter": a.maxiter, "processes": a.reps,
               "timed_calls_per_process": a.inner, "lm": lm, "lbfgs_analytic": lb,
               "lm_over_lbfgs": lm["median"] / lb["median"]}
        if parent_root:
            parent = summary(runs["parent_lbfgs_analytic"])
            spread = parent["max"] - parent["min"]
            row.update({"parent_lbfgs_analytic": parent, "parent_spread_seconds": spread,
                        "lbfgs_this_over_parent": lb["median"] / parent["median"],
                        "lbfgs_within_parent_spread":
                            abs(lb["median"] - parent["median"]) <= spread})
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
