"""Times one calibration request under the two objectives on the bench surfaces.

    python tools/iv_objective_time.py [--reps 200] [--out profiles/iv_objective_time.json]

Per shape -- C2 (1,024 options, N = 256, 14 param sets) and C3 (10,000 options, N = 512, 42 param
sets), the markets and FD param sets of bench.py -- the per-request time of
    dh_surface_loss_dev      the price objective (pricing and its loss sums in the request kernels)
    dh_surface_loss_iv_dev   the vol objective (dh_surface_price_dev, then the inversion + reduction)
and, to say where the difference goes, of the vol objective's two halves alone: dh_surface_price_dev
and dh_surface_iv_sse_dev over resident prices.  Every array is resident (torch tensors); HIP events
around each request on one non-default stream, median of `reps` after `warmup` untimed requests,
the requests cycling through 16 distinct FD requests.  Needs a gfx950 device.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch  # before the first libdhcos call: one HIP runtime (dhcos/_native.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "option-pricing-ffn-lbfgs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import bench  # noqa: E402


def event_us(run, stream, reps, warmup):
    """(median, min) HIP-event time in us of run(j), one event pair per request."""
    for j in range(warmup):
        run(j)
    stream.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
           for _ in range(reps)]
    for j, (e0, e1) in enumerate(evs):
        e0.record(stream)
        run(j)
        e1.record(stream)
    stream.synchronize()
    ms = np.array([e0.elapsed_time(e1) for e0, e1 in evs])
    return float(np.median(ms)) * 1e3, float(ms.min()) * 1e3


def shape(name, reps, warmup):
    import dhcos
    cfg = bench.CONFIGS[name]
    N, starts = cfg["N"], cfg["starts"]
    opts, S0, r = bench.make_surface(cfg["nK"], cfg["nT"], N=N, put_itm=cfg["put_itm"])
    cal = dhcos.DoubleHestonJumpCalibrator(S0, r, opts, N=N)
    surf = cal._get_surface()
    K, T = cal._option_arrays()
    mkt_iv = dhcos.implied_vol(cal.market_prices, S0, K, T, r, 0.0,
                               [o["option_type"] for o in opts])
    w = np.isfinite(mkt_iv).astype(np.float64)
    surf.set_iv_market(mkt_iv, w)
    S, M = 14 * starts, len(opts)
    steps = bench.step_params(cal, 16, starts, seed=7)
    ctx = surf.ctx
    dev = torch.device("cuda", ctx.device)
    d_steps = torch.from_numpy(steps).to(dev)
    d_sse = torch.empty(S, dtype=torch.float64, device=dev)
    d_bad = torch.empty(S, dtype=torch.int32, device=dev)
    d_prices = torch.empty((S, M), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.Stream(device=dev)
    st = stream.cuda_stream
    rec = lambda j: d_steps[j % 16].data_ptr()                                  # noqa: E731
    legs = {
        "loss_dev": lambda j: surf.loss_dev(rec(j), S, d_sse.data_ptr(), d_bad.data_ptr(),
                                            N=N, stream=st),
        "loss_iv_dev": lambda j: surf.loss_iv_dev(rec(j), S, d_sse.data_ptr(), d_bad.data_ptr(),
                                                  d_prices.data_ptr(), N=N, stream=st),
        "price_dev": lambda j: surf.price_dev(rec(j), S, d_prices.data_ptr(), N=N, stream=st),
    }
    out = {"config": name, "options": M, "N": N, "param_sets": S, "reps": reps,
           "market_vols_without_a_vol": int(np.count_nonzero(w == 0))}
    for leg, run in legs.items():
        med, lo = event_us(run, stream, reps, warmup)
        out[leg + "_us"] = {"median": med, "min": lo}
    # the stage alone, over the prices of request 0 (left resident by a price_dev call)
    surf.price_dev(rec(0), S, d_prices.data_ptr(), N=N, stream=st)
    med, lo = event_us(lambda j: surf.iv_sse_dev(rec(0), d_prices.data_ptr(), S,
                                                 d_sse.data_ptr(), d_bad.data_ptr(), stream=st),
                       stream, reps, warmup)
    out["iv_sse_dev_us"] = {"median": med, "min": lo}
    stream.synchronize()
    out["n_bad_total"] = int(d_bad.sum().item())
    out["ratio_iv_over_price_objective"] = out["loss_iv_dev_us"]["median"] / \
        out["loss_dev_us"]["median"]
    out["stage_quotes_per_s"] = S * M / (out["iv_sse_dev_us"]["median"] * 1e-6)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dhcos import _native
    if _native.device_count() == 0:
        raise SystemExit("iv_objective_time: no gfx950 device (nothing is timed on the CPU)")
    res = {"shapes": [shape(name, a.reps, a.warmup) for name in ("c2", "c3")]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
