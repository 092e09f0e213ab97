"""Times the coupled-path Monte Carlo Greeks against the plain pricer and against today's route.

    python tools/mc_greeks_time.py [--paths 1048576] [--steps-per-year 64] [--reps 7]
                                   [--ab-lib other/libdhcos.so] [--out profiles/mc_greeks_time.json]

The generator's 15 options (strikes 90 .. 110 at T = 0.25, 0.5, 1) as a mix of the four kinds, P = 1
and P = 64 parameter sets, device pointers in and out, HIP events around the two launches on a
stream of the caller.  Three calls from the same build:
    greeks    dh_mc_greeks_dev on the P records;
    plain     dh_mc_price_dev on the P records (one walk);
    stacked   dh_mc_price_dev on the seven bumped records per set (base, spot +-, v0_1 +-, v0_2 +-):
              central differences without this entry point, and without their standard errors.
A measurement is one fresh process: it warms each call up once, then times the three in turn, once
each.  The figures are medians over --reps such processes, with the ratios greeks / plain and
greeks / stacked formed per process.  With --ab-lib, `plain` is also timed on that other build of
the library (the parent commit's, say), the two builds in alternating fresh processes, to show the
pricer's own time against its run-to-run spread.  Needs a gfx950 device.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "option-pricing-ffn-lbfgs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

README = np.array([0.04, 2.5, 0.04, 0.3, -0.7, 0.04, 0.8, 0.04, 0.2, -0.5, 0.15, -0.04, 0.08])
LO = np.array([0.025, 1.5, 0.025, 0.2, -0.85, 0.02, 0.3, 0.025, 0.1, -0.7, 0.05, -0.08, 0.03])
HI = np.array([0.08, 4.5, 0.065, 0.5, -0.4, 0.07, 1.2, 0.07, 0.35, -0.2, 0.25, -0.01, 0.12])
SPOT, RATE, EPS, BUMP = 100.0, 0.03, 1e-2, 5e-2
KINDS = ({"kind": "european"}, {"kind": "asian"}, {"kind": "up_and_out", "barrier": 130.0},
         {"kind": "down_and_out", "barrier": 80.0})


def options():
    grid = [(float(k), t) for t in (0.25, 0.5, 1.0) for k in (90, 95, 100, 105, 110)]
    return [dict({"strike": k, "maturity": t, "option_type": "call" if i % 2 == 0 else "put"},
                 **KINDS[i % 4]) for i, (k, t) in enumerate(grid)]


def records(P):
    sets = README[None] if P == 1 else LO + (HI - LO) * np.random.RandomState(0).rand(P, 13)
    rec = np.zeros((P, 16))
    rec[:, :13] = sets
    rec[:, 13], rec[:, 14] = SPOT, RATE
    return rec


def stacked(rec):
    """[7 P, 16]: per set the base record, spot (1 +- eps), v0_1 (1 +- b), v0_2 (1 +- b)."""
    out = np.repeat(rec, 7, axis=0).reshape(len(rec), 7, 16)
    out[:, 1, 13] *= 1.0 + EPS
    out[:, 2, 13] *= 1.0 - EPS
    for k, (col, sign) in enumerate(((0, 1.0), (0, -1.0), (5, 1.0), (5, -1.0)), start=3):
        out[:, k, col] *= 1.0 + sign * BUMP
    return out.reshape(-1, 16)


def child(a):
    """One measurement: {call: milliseconds} on one line of JSON."""
    import torch
    from dhcos import _native
    from dhcos.montecarlo import _options
    if a.plain_only:
        # The other build may predate entry points that this binding declares.  _native.load()
        # binds lazily, on first use, every name that SIGNATURES holds at that moment: dropping
        # here, before anything has called load(), the names that the library does not export
        # makes it bind the rest.
        import ctypes
        lib = ctypes.CDLL(_native.LIB_PATH)
        for name in [n for n in _native.SIGNATURES if not hasattr(lib, n)]:
            del _native.SIGNATURES[name]
    if _native.device_count() == 0:
        raise SystemExit("mc_greeks_time: no gfx950 device (nothing is timed on the CPU)")
    ctx = _native.default_context()
    dev = f"cuda:{ctx.device}"
    opts = _options(options(), a.steps_per_year)
    rec = records(a.child)
    d_rec, d_stack = torch.from_numpy(rec).to(dev), torch.from_numpy(stacked(rec)).to(dev)
    stream = torch.cuda.Stream(dev)
    calls = {"plain": lambda: ctx.mc_price_dev(d_rec, opts, a.paths, a.steps_per_year, 1,
                                               stream=stream)}
    if not a.plain_only:
        calls["greeks"] = lambda: ctx.mc_greeks_dev(d_rec, opts, a.paths, a.steps_per_year, 1, EPS,
                                                    BUMP, stream=stream)
        calls["stacked"] = lambda: ctx.mc_price_dev(d_stack, opts, a.paths, a.steps_per_year, 1,
                                                    stream=stream)
    res = {}
    with torch.cuda.stream(stream):
        for fn in calls.values():              # warm-up: the scratch of every call is allocated
            fn()
        stream.synchronize()
        for name, fn in calls.items():
            t0, t1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            t0.record(stream)
            out = fn()
            t1.record(stream)
            t1.synchronize()
            assert bool(torch.isfinite(out[0]).all())
            res[name] = t0.elapsed_time(t1)
    print("MC_GREEKS_TIME " + json.dumps(res))


def measure(a, P, lib=None, plain_only=False):
    env = dict(os.environ)
    if lib:
        env["DHCOS_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(P), "--paths", str(a.paths),
           "--steps-per-year", str(a.steps_per_year)] + (["--plain-only"] if plain_only else [])
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if out.returncode:                         # the first failure ends the run: nothing is retried
        raise SystemExit(f"mc_greeks_time: a measurement exited with {out.returncode}:\n"
                         + out.stderr[-2000:])
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("MC_GREEKS_TIME ")][-1]
    return json.loads(line.split(" ", 1)[1])


def resource_usage():
    """VGPRs, scratch, occupancy and LDS of mc_greeks_kernel as `make resource-usage` reported
    them (profiles/mc_greeks_resource_usage.txt), or {} without that record."""
    path = os.path.join(ROOT, "profiles", "mc_greeks_resource_usage.txt")
    if not os.path.exists(path):
        return {}
    block = open(path).read().split("mc_greeks_kernel", 1)[-1].split("Function Name", 1)[0]
    keys = {"VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
            "Occupancy [waves/SIMD]": "occupancy_waves_per_simd",
            "LDS Size [bytes/block]": "lds_bytes_per_block"}
    out = {}
    for line in block.splitlines():
        for k, name in keys.items():
            if f" {k}: " in line:
                out[name] = int(line.rsplit(":", 1)[1])
    return out


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=1 << 20)
    ap.add_argument("--steps-per-year", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ab-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--plain-only", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {"paths": a.paths, "steps_per_year": a.steps_per_year, "options": len(options()),
           "reps": a.reps, "spot_bump": EPS, "v0_bump": BUMP,
           "mc_greeks_kernel": resource_usage()}
    for P in (1, 64):
        runs = [measure(a, P) for _ in range(a.reps)]
        row = {name + "_ms": spread([r[name] for r in runs])
               for name in ("greeks", "plain", "stacked")}
        row["greeks_vs_plain"] = spread([r["greeks"] / r["plain"] for r in runs])
        row["greeks_vs_stacked"] = spread([r["greeks"] / r["stacked"] for r in runs])
        if a.ab_lib:
            ab = {"this": [], "other": []}
            for _ in range(a.reps):            # the two builds in alternating fresh processes
                ab["this"].append(measure(a, P, None, True)["plain"])
                ab["other"].append(measure(a, P, a.ab_lib, True)["plain"])
            row["plain_this_build_ms"] = spread(ab["this"])
            row["plain_other_build_ms"] = spread(ab["other"])
        res[f"P{P}"] = row
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
