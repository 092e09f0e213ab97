"""Times the implied-vol kernel on the generator's output and the host route it replaces.

    python tools/iv_time.py [--samples 1000000] [--reps 20] [--out profiles/iv_time.json]

Device: dh_implied_vol_dev on the `market_prices` of generate_synthetic_calibrations(samples,
as_arrays=True) (samples x 15 quotes, already resident as torch tensors), HIP events around `reps`
launches on one non-default stream after 3 warm-up launches.  Host: SciPy brentq on the textbook
formula (the yardstick of tests/golden/make_iv_truth.py) over a 2,000-quote slice, wall clock.
Needs a gfx950 device.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # before the first libdhcos call: one HIP runtime (dhcos/_native.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "option-pricing-ffn-lbfgs_amd"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--slice", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dhcos import _native, generate_synthetic_calibrations
    if _native.device_count() == 0:
        raise SystemExit("iv_time: no gfx950 device (nothing is timed on the CPU)")
    np.random.seed(0)
    g = generate_synthetic_calibrations(a.samples, None, as_arrays=True, verbose=False)
    shape = g["market_prices"].shape
    n = int(np.prod(shape))
    cols_h = [np.ascontiguousarray(np.broadcast_to(c, shape)).reshape(-1) for c in
              (g["market_prices"], g["spot"][:, None], g["strikes"], g["maturities"],
               np.float64(g["risk_free"]), np.float64(0.0))]
    ctx = _native.default_context()
    dev = torch.device("cuda", ctx.device)
    cols = [torch.from_numpy(c.copy()).to(dev) for c in cols_h]
    ic = torch.ones(n, dtype=torch.int8, device=dev)
    out = torch.empty(n, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.Stream(device=dev)     # the launches and their events on one stream
    for _ in range(3):
        ctx.implied_vol_dev(*cols, ic, out=out, stream=stream)
    stream.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.reps + 1)]
    ev[0].record(stream)
    for i in range(a.reps):
        ctx.implied_vol_dev(*cols, ic, out=out, stream=stream)
        ev[i + 1].record(stream)
    stream.synchronize()
    ms = np.array([ev[i].elapsed_time(ev[i + 1]) for i in range(a.reps)])
    sig = out.cpu().numpy()
    # the host route on a slice, and the device's agreement with it there
    from make_iv_truth import brentq_iv
    m = min(a.slice, n)
    t0 = time.perf_counter()
    host = np.array([brentq_iv(cols_h[0][i], cols_h[1][i], cols_h[2][i], cols_h[3][i],
                               cols_h[4][i], cols_h[5][i], 1) for i in range(m)])
    host_s = time.perf_counter() - t0
    ok = np.isfinite(sig[:m])
    res = {"quotes": n, "reps": a.reps, "kernel_ms_median": float(np.median(ms)),
           "kernel_ms_min": float(ms.min()), "kernel_ms_max": float(ms.max()),
           "quotes_per_s": n / (float(np.median(ms)) * 1e-3),
           "nan_share": float(np.mean(np.isnan(sig))),
           "brentq_slice": m, "brentq_s": host_s, "brentq_us_per_quote": host_s / m * 1e6,
           "brentq_extrapolated_s": host_s / m * n,
           "max_abs_diff_vs_brentq": float(np.max(np.abs(sig[:m] - host)[ok])) if ok.any() else None}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
