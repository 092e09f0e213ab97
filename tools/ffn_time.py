"""Measures the warm-start network: the inference kernel against torch, and the hybrid calibration
against the default single start.  Nothing here is a gate; the figures go to DESIGN.md 3.22.

    python tools/ffn_time.py [--train 100000] [--epochs 200] [--sizes 256,4096]
                             [--out profiles/ffn_time.json]

Inference: ffn_forward_kernel (dh_ffn_forward_dev on a side stream) at the default widths, B = 1,
256, 4,096 and 1,000,000, timed by HIP events (torch.cuda.Event on that stream), median of 7 after
warm-up, beside torch's float32 evaluation of the same folded network on the same GPU, and the
share of the 157.3 TFLOP/s fp32 peak the real (unpadded) FLOPs reach at 1M.

Hybrid: train on `--train` generator samples (np.random.seed(0)), then on generator markets of
another seed run calibrate_batch with x0s=model, with the default single start (multi_start=1,
whose starts are formed by a host loop inside the call) and with that same start handed over as an
array (the fair comparison of wall times), for gradient="analytic" and method="lm", at maxiter 300 and 10: median final loss,
median requests per start, share of tolerance stops, wall time (the inference included; second of
two calls).  Also the network-only mean relative price error beside the generator's 2 % noise.
Needs a gfx950 device.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_FP32 = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", type=int, default=100_000)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--sizes", default="256,4096")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ffn_time.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    for p in (ROOT, os.path.join(ROOT, "option-pricing-ffn-lbfgs_amd")):
        sys.path.insert(0, p)
    import dhcos
    from dhcos import _native
    from dhcos.ffn import DEFAULT_HIDDEN, build_stack
    from dhcos.generator import MATURITIES, STRIKES_PCT, grid_surface
    if _native.device_count() == 0:
        raise SystemExit("ffn_time: no gfx950 device (nothing is timed on the CPU)")
    ctx = _native.default_context()
    dev = torch.device("cuda", ctx.device)
    out = {"widths": [11, *DEFAULT_HIDDEN, 13]}

    # ---- training
    model, hist = dhcos.train_ffn_on_generator(a.train, gen_seed=0, epochs=a.epochs, seed=0)
    out["training"] = dict(samples=a.train, seconds=hist["seconds"], epochs_run=len(hist["val"]),
                           best_epoch=hist["best_epoch"], best_val=hist["best_val"])
    print("training", out["training"], flush=True)

    # ---- inference
    ffn = model.on_device()
    net = build_stack(model.widths).to(dev)
    lin = [m for m in net if isinstance(m, torch.nn.Linear)]
    with torch.no_grad():
        for m, W, b in zip(lin, model.weights, model.biases):
            m.weight.copy_(torch.from_numpy(W))
            m.bias.copy_(torch.from_numpy(b))
        for m in net:
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_var.fill_(1.0 - m.eps)
    net.eval()
    flops = 2 * sum(int(W.size) for W in model.weights)
    side = torch.cuda.Stream(dev)
    np.random.seed(1)
    g = dhcos.generate_synthetic_calibrations(4096, None, as_arrays=True, verbose=False)
    rows = []
    for B in (1, 256, 4096, 1_000_000):
        idx = np.arange(B) % 4096
        d_mkt = torch.from_numpy(np.ascontiguousarray(g["market_prices"][idx])).to(dev)
        d_sp = torch.from_numpy(np.ascontiguousarray(g["spot"][idx])).to(dev)
        d_x0 = torch.empty((B, 13), dtype=torch.float64, device=dev)
        z = torch.from_numpy(((model.input_features(g["market_prices"][idx], g["spot"][idx])
                               - model.x_mean) / model.x_std).astype(np.float32)).to(dev)
        torch.cuda.synchronize(dev)

        def timed(fn, stream):
            ms = []
            for rep in range(10):                      # 3 warm-up, 7 timed
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                if rep >= 3:
                    ms.append(e0.elapsed_time(e1))
            return float(np.median(ms))

        t_kernel = timed(lambda: ctx.ffn_forward_dev(ffn, d_mkt, d_sp, x0=d_x0, stream=side), side)
        with torch.no_grad(), torch.cuda.stream(side):
            t_torch = timed(lambda: net(z), side)
        rows.append(dict(B=B, kernel_ms=t_kernel, torch_fp32_ms=t_torch,
                         kernel_tflops=flops * B / (t_kernel * 1e-3) / 1e12,
                         share_of_fp32_peak=flops * B / (t_kernel * 1e-3) / PEAK_FP32))
        print(rows[-1], flush=True)
    out["inference"] = rows

    # ---- hybrid
    sizes = [int(s) for s in a.sizes.split(",")]
    np.random.seed(2)
    g = dhcos.generate_synthetic_calibrations(max(sizes), None, as_arrays=True, verbose=False)
    r = float(g["risk_free"])
    surf = grid_surface(ctx, STRIKES_PCT, MATURITIES)[0]
    pred = model.predict_parameters(g["market_prices"], g["spot"])
    rec = np.zeros((pred.shape[0], 16))
    rec[:, :13], rec[:, 13], rec[:, 14] = pred, g["spot"], r
    px = surf.price(rec, 128)                          # strikes in percent of each record's spot
    rel = np.abs(px - g["market_prices"]) / g["market_prices"]
    out["ffn_only_mean_rel_price_error"] = float(np.mean(rel))
    out["generator_noise"] = 0.02
    print("network-only mean relative price error", out["ffn_only_mean_rel_price_error"],
          flush=True)
    hybrid = []
    from dhcos.batch import _grid, default_starts
    K, T, flags, _ = _grid(STRIKES_PCT, MATURITIES, None, True)
    for B in sizes:
        mkt, sp = g["market_prices"][:B], g["spot"][:B]
        # the default single start of every market as an array, formed outside the timed call:
        # multi_start=1 forms the same starts in a host loop inside it
        X_default = default_starts(mkt, sp, np.full(B, r), K[None, :] * sp[:, None] / 100.0, T,
                                   flags, 1)
        for kind, kw in (("analytic", dict(gradient="analytic")), ("lm", dict(method="lm"))):
            for maxiter in (300, 10):
                for start in ("ffn", "default", "default_array"):
                    for rep in range(2):               # the second call is the timed one
                        np.random.seed(3)
                        t0 = time.perf_counter()
                        res = dhcos.calibrate_batch(
                            mkt, sp, r, maxiter=maxiter,
                            **(dict(x0s=model) if start == "ffn" else dict(multi_start=1)
                               if start == "default" else dict(x0s=X_default)), **kw)
                        wall = time.perf_counter() - t0
                    fun = res.fun[:, 0]
                    ok = np.isfinite(fun)
                    task = res.start_task[:, 0]
                    stops = (np.isin(task, (1, 2, 3)) if kind == "lm" else res.status[:, 0] == 0)
                    hybrid.append(dict(B=B, driver=kind, maxiter=maxiter, start=start,
                                       wall_ms=wall * 1e3, finite=int(ok.sum()),
                                       median_final_loss=float(np.median(fun[ok])),
                                       median_requests=float(np.median(res.nfev[:, 0])),
                                       tolerance_stops=float(np.mean(stops))))
                    print(hybrid[-1], flush=True)
    out["hybrid"] = hybrid
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
