"""Times calibrate_batch(objective="iv", gradient="vega") against gradient="fd" on the same markets,
and the three older device paths of this build against a parent build's.

    python tools/batch_iv_grad_calibrate_time.py [--sizes 1,256,4096] [--reps 7]
                                                 [--parent-root DIR]
                                                 [--out profiles/batch_iv_grad_calibrate_time.json]

Markets and starts: tools/batch_iv_calibrate_time.py's --
generate_synthetic_calibrations(max B, as_arrays=True, implied_vols=True) under np.random.seed(0),
the generator's 15-option grid, N = 128, a spot per market; the vols fitted are its ``market_iv``
column, weight 0 where a noisy market price has no vol and 1 elsewhere.  Every market gets one warm
start: its true parameters x (1 + 5% noise), maxiter = 300.

Every figure comes from fresh processes, alternating between the two sides: per B and repetition
one process runs "fd" and the next "vega" (the same build, the same markets and starts).  A process
draws the markets, runs the call once to warm up (allocations, first launches) and then times it
`--inner` times; its figure is the median of those.  The recorded time is the median over the
`--reps` processes, with their minimum and maximum.  Per side also: iterations enqueued, total
requests and loss evaluations, the share of starts that report convergence, the median final loss.

--parent-root DIR: a built checkout of the parent commit.  objective="price" under "fd" and
"analytic" and objective="iv" under "fd", at B = 256, are then timed from DIR and from this tree,
processes alternating, and the record holds both medians, the parent's own run-to-run spread (max -
min over its processes) and whether the two medians agree within it.
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
        raise SystemExit("batch_iv_grad_calibrate_time: no gfx950 device (nothing is timed on the "
                         "CPU)")
    np.random.seed(0)
    g = dhcos.generate_synthetic_calibrations(a.nmax, None, as_arrays=True, verbose=False,
                                              implied_vols=True)
    mkt, spots, r = g["market_prices"], g["spot"], float(g["risk_free"])
    ivs = np.ascontiguousarray(g["market_iv"], dtype=np.float64)
    wts = (np.isfinite(ivs) & (ivs >= 0)).astype(np.float64)
    cal0 = dhcos.DoubleHestonJumpCalibrator(100.0, r, [])
    rs = np.random.RandomState(1)
    X = np.empty((a.nmax, 1, 13))
    for b in range(a.nmax):
        true = dict(zip(cal0.param_names, g["params"][b] * (1 + 0.05 * rs.randn(13))))
        X[b, 0] = cal0.inverse_transform_params(true)
    B = a.child
    kw = {} if a.gradient == "fd" else {"gradient": a.gradient}
    if a.objective == "iv":
        kw.update(objective="iv", market_ivs=ivs[:B], iv_weights=wts[:B])

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
                      "requests": int(res.nfev.sum()),
                      "loss_evaluations": int(res.n_calls.sum()),
                      "converged_share": float(np.mean(res.status == 0)),
                      "median_final_loss": float(np.median(res.final_loss))}), flush=True)


def spawn(a, root, B, objective, gradient):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(B), "--objective", objective,
           "--gradient", gradient, "--root", root, "--nmax", str(a.nmax), "--maxiter",
           str(a.maxiter), "--inner", str(a.inner)]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900).stdout
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
    ap.add_argument("--objective", default="iv")
    ap.add_argument("--gradient", default="fd")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--nmax", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        return child(a)
    sizes = [int(s) for s in a.sizes.split(",") if s]
    a.nmax = max(sizes + [256])
    rows = []
    for B in sizes:
        runs = {"fd": [], "vega": []}
        for _ in range(a.reps):
            for gradient in ("fd", "vega"):
                runs[gradient].append(spawn(a, ROOT, B, "iv", gradient))
        fd, vg = summary(runs["fd"]), summary(runs["vega"])
        row = {"markets": B, "starts_per_market": 1, "maxiter": a.maxiter, "processes": a.reps,
               "timed_calls_per_process": a.inner, "objective": "iv", "fd": fd, "vega": vg,
               "vega_over_fd": vg["median"] / fd["median"]}
        print(json.dumps(row), flush=True)
        rows.append(row)
    record = {"rows": rows}
    if a.parent_root:
        record["regression"] = []
        for objective, gradient in (("price", "fd"), ("price", "analytic"), ("iv", "fd")):
            runs = {"parent": [], "this": []}
            for _ in range(a.reps):
                runs["parent"].append(spawn(a, os.path.abspath(a.parent_root), 256, objective,
                                            gradient))
                runs["this"].append(spawn(a, ROOT, 256, objective, gradient))
            parent, this = summary(runs["parent"]), summary(runs["this"])
            spread = parent["max"] - parent["min"]
            rec = {"objective": objective, "gradient": gradient, "markets": 256,
                   "processes": a.reps, "parent_seconds": parent, "this_seconds": this,
                   "parent_spread_seconds": spread,
                   "this_over_parent": this["median"] / parent["median"],
                   "within_parent_spread": abs(this["median"] - parent["median"]) <= spread}
            print(json.dumps(rec), flush=True)
            record["regression"].append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(record, fh, indent=1)


if __name__ == "__main__":
    main()
