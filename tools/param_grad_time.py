"""Times the analytic loss + gradient request against the forward-difference request of another
build of the library, and calibrate() both ways.

    python tools/param_grad_time.py --parent-lib PATH/libdhcos_parent.so [--rounds 7] [--reps 50]
                                    [--out profiles/param_grad_time.json]

What is timed, on bench.py's C1 (5 x 3 options, N = 128), C2 (32 x 32, N = 256) and C3 (100 x 100,
N = 512) surfaces with a clean market priced at the seed-1 draw, for S = 1 and S = 3 starts drawn
around it:
  * dh_surface_loss_grad_dev of this tree's library on the context's stream (the analytic request:
    records, the fourteen planes, the reduction), and
  * dh_surface_fg of the library at --parent-lib (a build of the parent commit): the same starts'
    forward-difference request, 14 S points.  It is a host call that returns after its own
    synchronisation; the events sit on the context's stream around it, so its figure holds its
    device work and the host time between its launches, as a SciPy driver sees it.
  * calibrate(300, 3) wall time with gradient="fd" and gradient="analytic" on C1 and C2, this
    tree's library, under np.random.seed(0) (--no-calibrate skips it).
The yardstick is the parent's FD request.

How: this process never opens the GPU.  It starts one fresh child process per (library, case, S)
measurement and alternates the two libraries, `rounds` times; a child loads one library, warms up
with 5 requests, then takes HIP events around each of `reps` requests and reports their median.
The figure of a (library, case, S) is the median over the rounds' medians.  Needs a gfx950 device.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"c1": dict(nK=5, nT=3, N=128, put_itm=False),
         "c2": dict(nK=32, nT=32, N=256, put_itm=False),
         "c3": dict(nK=100, nT=100, N=512, put_itm=True)}
LO = np.array([0.025, 1.5, 0.025, 0.2, -0.85, 0.02, 0.3, 0.025, 0.1, -0.7, 0.05, -0.08, 0.03])
HI = np.array([0.08, 4.5, 0.065, 0.5, -0.4, 0.07, 1.2, 0.07, 0.35, -0.2, 0.25, -0.01, 0.12])
NEW_EXPORTS = ("dh_surface_param_sens", "dh_surface_param_sens_dev", "dh_param_sens_pairs",
               "dh_surface_loss_grad", "dh_surface_loss_grad_dev")
S0, RATE = 100.0, 0.03


def case_inputs(name):
    """bench.py's surface of the case, the seed-1 draw and three starts 5 % around it (in x)."""
    cfg = CASES[name]
    kk, tt = np.meshgrid(np.linspace(0.8, 1.2, cfg["nK"]) * S0, np.linspace(0.1, 2.0, cfg["nT"]))
    K, T = kk.ravel(), tt.ravel()
    call = np.ones(K.size, dtype=bool) if not cfg["put_itm"] else (K >= S0)
    true = LO + (HI - LO) * np.random.RandomState(1).rand(13)
    x = np.log(np.abs(true))
    x[[4, 9]] = np.arctanh(true[[4, 9]])
    x[11] = true[11]
    X = x + 0.05 * np.random.RandomState(3).uniform(-1, 1, (3, 13))
    return true, X, K, T, call, cfg["N"]


def _setup(a):
    import torch  # before the first libdhcos call: one HIP runtime (dhcos/_native.py)
    sys.path[:0] = [ROOT, os.path.join(ROOT, "option-pricing-ffn-lbfgs_amd")]
    from dhcos import _native
    if a.what == "fd":             # a library of before this feature has no such exports to bind
        for name in NEW_EXPORTS:
            _native.SIGNATURES.pop(name, None)
    if _native.device_count() == 0:
        raise SystemExit("param_grad_time: no gfx950 device (nothing is timed on the CPU)")
    return torch, _native


def worker(a):
    """One measurement in this (fresh) process: prints {"median_ms": x, ...}."""
    torch, _native = _setup(a)
    true, X, K, T, call, N = case_inputs(a.case)
    X = np.ascontiguousarray(X[:a.starts])
    ctx = _native.default_context()
    dev = torch.device("cuda", ctx.device)
    rec = np.zeros((1, 16))
    rec[0, :13], rec[0, 13], rec[0, 14] = true, S0, RATE
    plain = _native.Surface(ctx, K, T, call)
    mkt = plain.price(rec, N)[0]
    plain.close()
    surf = _native.Surface(ctx, K, T, call, mkt)
    stream = torch.cuda.ExternalStream(ctx.stream, device=dev)
    S = X.shape[0]
    if a.what == "analytic":
        d_x = torch.from_numpy(X).to(dev)
        d_f = torch.empty(S, dtype=torch.float64, device=dev)
        d_g = torch.empty((S, 13), dtype=torch.float64, device=dev)
        d_bad = torch.empty(S, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)

        def one():
            surf.loss_grad_dev(d_x.data_ptr(), S, S0, RATE, d_f.data_ptr(), d_g.data_ptr(),
                               d_bad.data_ptr(), N=N)
    else:
        last = {}

        def one():
            last["fg"] = surf.fg(X, S0, RATE, N)
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
    f = d_f.cpu().numpy() if a.what == "analytic" else last["fg"][0]
    surf.close()
    print(json.dumps({"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)),
                      "max_ms": float(np.max(ms)), "f": [float(v) for v in f]}))


def calibrate_worker(a):
    """calibrate(300, 3) wall time, median of reps runs after one warm-up run."""
    torch, _native = _setup(a)
    from dhcos import DoubleHestonJumpCalibrator
    true, _, K, T, call, N = case_inputs(a.case)
    rec = np.zeros((1, 16))
    rec[0, :13], rec[0, 13], rec[0, 14] = true, S0, RATE
    plain = _native.Surface(_native.default_context(), K, T, call)
    mkt = plain.price(rec, N)[0]
    plain.close()
    opts = [{"strike": float(k), "maturity": float(t), "price": float(p),
             "option_type": "call" if c else "put"} for k, t, p, c in zip(K, T, mkt, call)]
    times, res = [], None
    for i in range(a.reps + 1):
        np.random.seed(0)
        cal = DoubleHestonJumpCalibrator(S0, RATE, opts, N=N, gradient=a.what)
        cal._get_surface()
        t0 = time.perf_counter()
        res = cal.calibrate(300, 3)
        if i:
            times.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"median_ms": float(np.median(times)), "final_loss": float(res.final_loss),
                      "nit": int(res.iterations), "requests": int(cal.lockstep_launches),
                      "loss_evals": int(cal.loss_evals), "message": str(res.message)}))


def measure(lib, what, case, starts, reps, mode="request"):
    env = dict(os.environ, DHCOS_LIB=os.path.abspath(lib))
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--what", what, "--case",
           case, "--starts", str(starts), "--reps", str(reps)]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if res.returncode != 0:
        raise SystemExit(f"param_grad_time: worker {what} {case} failed ({res.returncode}):\n"
                         f"{res.stdout}\n{res.stderr}")
    return json.loads(res.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-calibrate", action="store_true")
    ap.add_argument("--worker", choices=("request", "calibrate"), default=None)
    ap.add_argument("--what", choices=("fd", "analytic"))
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--starts", type=int, default=1)
    a = ap.parse_args()
    if a.worker == "request":
        return worker(a)
    if a.worker == "calibrate":
        return calibrate_worker(a)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("param_grad_time: --parent-lib must name a build of the parent commit")
    this_lib = os.path.join(ROOT, "option-pricing-ffn-lbfgs_amd", "dhcos", "libdhcos.so")
    res = {"rounds": a.rounds, "reps": a.reps, "requests": {}, "calibrate": {}}
    for case, cfg in CASES.items():
        for S in (1, 3):
            runs = {"fd_parent": [], "analytic": []}
            for _ in range(a.rounds):                       # alternate the two libraries
                runs["fd_parent"].append(measure(a.parent_lib, "fd", case, S, a.reps))
                runs["analytic"].append(measure(this_lib, "analytic", case, S, a.reps))
            fd = float(np.median([x["median_ms"] for x in runs["fd_parent"]]))
            an = float(np.median([x["median_ms"] for x in runs["analytic"]]))
            res["requests"][f"{case}_S{S}"] = {
                "options": cfg["nK"] * cfg["nT"], "N": cfg["N"], "S": S, "fd_parent_ms": fd,
                "analytic_ms": an, "analytic_over_fd": an / fd,
                "fd_parent_ms_rounds": [x["median_ms"] for x in runs["fd_parent"]],
                "analytic_ms_rounds": [x["median_ms"] for x in runs["analytic"]],
                "f_fd": runs["fd_parent"][0]["f"], "f_analytic": runs["analytic"][0]["f"]}
            print(case, S, json.dumps(res["requests"][f"{case}_S{S}"]), flush=True)
    if not a.no_calibrate:
        for case in ("c1", "c2"):
            out = {w: measure(this_lib, w, case, 3, 5, "calibrate") for w in ("fd", "analytic")}
            res["calibrate"][case] = out
            print(case, "calibrate(300, 3)", json.dumps(out), flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
