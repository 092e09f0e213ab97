"""Times the analytic Greeks against the pricing request of another build of the library.

    python tools/greeks_time.py --parent-lib PATH/libdhcos_parent.so [--rounds 7] [--reps 50]
                                [--out profiles/greeks_time.json]

What is timed: dh_surface_greeks_dev of this tree's library, and dh_surface_price_dev of the library
at --parent-lib (a build of the parent commit), on the same records: one FD request (P = 14 param
sets) on the C2 surface (32 x 32 = 1,024 options, 32 maturities, N = 256) and on the C3 surface
(100 x 100 = 10,000 options, N = 512) of bench.py.  The feature replaces bump-and-reprice, nine
pricing requests for its five sensitivities by central differences, so the bar for the ratio
greeks / price is 9.

How: this process never opens the GPU.  It starts one fresh child process per (library, case)
measurement and alternates the two libraries, `rounds` times; a child loads one library, warms up
with 5 requests, then takes HIP events around each of `reps` requests on one non-default stream and
reports their median.  The figure of a (library, case) is the median over the rounds' medians.
Needs a gfx950 device.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"c2": dict(nK=32, nT=32, N=256, put_itm=False),
         "c3": dict(nK=100, nT=100, N=512, put_itm=True)}
LO = np.array([0.025, 1.5, 0.025, 0.2, -0.85, 0.02, 0.3, 0.025, 0.1, -0.7, 0.05, -0.08, 0.03])
HI = np.array([0.08, 4.5, 0.065, 0.5, -0.4, 0.07, 1.2, 0.07, 0.35, -0.2, 0.25, -0.01, 0.12])
GREEK_EXPORTS = ("dh_surface_greeks", "dh_surface_greeks_dev", "dh_greeks_pairs")


def case_inputs(name, S0=100.0, r=0.03):
    """bench.py's surface of the case and one FD request: the seed-1 draw and its 13 bumps."""
    cfg = CASES[name]
    kk, tt = np.meshgrid(np.linspace(0.8, 1.2, cfg["nK"]) * S0, np.linspace(0.1, 2.0, cfg["nT"]))
    K, T = kk.ravel(), tt.ravel()
    call = np.ones(K.size, dtype=bool) if not cfg["put_itm"] else (K >= S0)
    true = LO + (HI - LO) * np.random.RandomState(1).rand(13)
    rec = np.zeros((14, 16))
    rec[:, :13], rec[:, 13], rec[:, 14] = true, S0, r
    for i in range(13):
        rec[1 + i, i] *= 1.0 + 1e-8
    return rec, K, T, call, cfg["N"]


def worker(a):
    """One measurement in this (fresh) process: prints {"ms": [...], "median_ms": x}."""
    import torch  # before the first libdhcos call: one HIP runtime (dhcos/_native.py)
    sys.path[:0] = [ROOT, os.path.join(ROOT, "option-pricing-ffn-lbfgs_amd")]
    from dhcos import _native
    if a.what == "price":          # a library of before the Greeks has no such exports to bind
        for name in GREEK_EXPORTS:
            _native.SIGNATURES.pop(name, None)
    if _native.device_count() == 0:
        raise SystemExit("greeks_time: no gfx950 device (nothing is timed on the CPU)")
    rec, K, T, call, N = case_inputs(a.case)
    ctx = _native.default_context()
    dev = torch.device("cuda", ctx.device)
    surf = _native.Surface(ctx, K, T, call)
    P, M = rec.shape[0], K.size
    d_rec = torch.from_numpy(rec).to(dev)
    planes = 6 if a.what == "greeks" else 1
    d_out = torch.empty((planes, P, M), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.Stream(device=dev)
    request = surf.greeks_dev if a.what == "greeks" else surf.price_dev

    def one():
        request(d_rec.data_ptr(), P, d_out.data_ptr(), N=N, stream=stream.cuda_stream)

    for _ in range(5):
        one()
    stream.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.reps + 1)]
    ev[0].record(stream)
    for i in range(a.reps):
        one()
        ev[i + 1].record(stream)
    stream.synchronize()
    ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(a.reps)]
    out = d_out.cpu().numpy()
    surf.close()
    print(json.dumps({"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)),
                      "max_ms": float(np.max(ms)), "finite": bool(np.isfinite(out).all()),
                      "price_sum": float(out[0].sum())}))


def measure(lib, what, case, reps):
    env = dict(os.environ, DHCOS_LIB=os.path.abspath(lib))
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--what", what, "--case", case,
           "--reps", str(reps)]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    if res.returncode != 0:
        raise SystemExit(f"greeks_time: worker {what} {case} failed ({res.returncode}):\n"
                         f"{res.stdout}\n{res.stderr}")
    return json.loads(res.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--what", choices=("price", "greeks"))
    ap.add_argument("--case", choices=sorted(CASES))
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("greeks_time: --parent-lib must name a build of the parent commit")
    this_lib = os.path.join(ROOT, "option-pricing-ffn-lbfgs_amd", "dhcos", "libdhcos.so")
    res = {"P": 14, "rounds": a.rounds, "reps": a.reps, "bar": 9.0, "cases": {}}
    for case, cfg in CASES.items():
        runs = {"price_parent": [], "greeks": []}
        for _ in range(a.rounds):                       # alternate the two libraries
            runs["price_parent"].append(measure(a.parent_lib, "price", case, a.reps))
            runs["greeks"].append(measure(this_lib, "greeks", case, a.reps))
        price = float(np.median([x["median_ms"] for x in runs["price_parent"]]))
        greeks = float(np.median([x["median_ms"] for x in runs["greeks"]]))
        # the two builds price the same records: the price planes' sums agree
        sums = [runs[k][0]["price_sum"] for k in runs]
        res["cases"][case] = {
            "options": cfg["nK"] * cfg["nT"], "maturities": cfg["nT"], "N": cfg["N"],
            "price_parent_ms": price, "greeks_ms": greeks, "ratio": greeks / price,
            "below_bar": greeks / price < 9.0,
            "price_parent_ms_rounds": [x["median_ms"] for x in runs["price_parent"]],
            "greeks_ms_rounds": [x["median_ms"] for x in runs["greeks"]],
            "price_sum_parent": sums[0], "price_sum_greeks": sums[1],
            "all_finite": all(x["finite"] for k in runs for x in runs[k])}
        print(case, json.dumps(res["cases"][case]), flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
