"""Times the full Greeks (dh_surface_greeks_full_dev, ten planes) against the Greeks
(dh_surface_greeks_dev, six planes) of the same build.

    python tools/greeks_full_time.py [--rounds 7] [--reps 50] [--out profiles/greeks_full_time.json]

What is timed: one request of P = 14 param sets on the C2 surface (32 x 32 = 1,024 options, 32
maturities, N = 256) and on the C3 surface (100 x 100 = 10,000 options, N = 512) of bench.py --
tools/greeks_time.py's cases and records.  No ratio is required; eight sums against six and seven
table arrays against five suggest something under 1.5.

How: tools/greeks_time.py's way.  This process never opens the GPU.  It starts one fresh child
process per (request, case) measurement and alternates the two requests, `rounds` times; a child
warms up with 5 requests, then takes HIP events around each of `reps` requests on one non-default
stream and reports their median.  The figure of a (request, case) is the median over the rounds'
medians.  Needs a gfx950 device.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from greeks_time import CASES, case_inputs  # noqa: E402


def worker(a):
    """One measurement in this (fresh) process: prints {"median_ms": x, ...}."""
    import torch  # before the first libdhcos call: one HIP runtime (dhcos/_native.py)
    sys.path[:0] = [ROOT, os.path.join(ROOT, "option-pricing-ffn-lbfgs_amd")]
    from dhcos import _native
    if _native.device_count() == 0:
        raise SystemExit("greeks_full_time: no gfx950 device (nothing is timed on the CPU)")
    rec, K, T, call, N = case_inputs(a.case)
    ctx = _native.default_context()
    dev = torch.device("cuda", ctx.device)
    surf = _native.Surface(ctx, K, T, call)
    P, M = rec.shape[0], K.size
    d_rec = torch.from_numpy(rec).to(dev)
    planes = len(_native.GREEKS_FULL if a.what == "full" else _native.GREEKS)
    d_out = torch.empty((planes, P, M), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.Stream(device=dev)
    request = surf.greeks_full_dev if a.what == "full" else surf.greeks_dev

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
                      "max_ms": float(np.max(ms)), "finite_six": bool(np.isfinite(out[:6]).all()),
                      "price_sum": float(out[0].sum())}))


def measure(what, case, reps):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--what", what, "--case", case,
           "--reps", str(reps)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if res.returncode != 0:
        raise SystemExit(f"greeks_full_time: worker {what} {case} failed ({res.returncode}):\n"
                         f"{res.stdout}\n{res.stderr}")
    return json.loads(res.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--what", choices=("greeks", "full"))
    ap.add_argument("--case", choices=sorted(CASES))
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    res = {"P": 14, "rounds": a.rounds, "reps": a.reps, "cases": {}}
    for case, cfg in CASES.items():
        runs = {"greeks": [], "full": []}
        for _ in range(a.rounds):                       # alternate the two requests
            for what in runs:
                runs[what].append(measure(what, case, a.reps))
        six = float(np.median([x["median_ms"] for x in runs["greeks"]]))
        ten = float(np.median([x["median_ms"] for x in runs["full"]]))
        res["cases"][case] = {
            "options": cfg["nK"] * cfg["nT"], "maturities": cfg["nT"], "N": cfg["N"],
            "greeks_ms": six, "greeks_full_ms": ten, "ratio": ten / six,
            "greeks_ms_rounds": [x["median_ms"] for x in runs["greeks"]],
            "greeks_full_ms_rounds": [x["median_ms"] for x in runs["full"]],
            # the two requests price the same records: the price planes' sums are equal
            "price_sum_equal": runs["greeks"][0]["price_sum"] == runs["full"][0]["price_sum"],
            "six_planes_finite": all(x["finite_six"] for k in runs for x in runs[k])}
        print(case, json.dumps(res["cases"][case]), flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
