"""Measured accuracy of the fp64 elementary functions of csrc/dh_device.h on the GPU: runs
dh_math_probe over tests/golden/math_truth.npz (mpmath truth as double-doubles) and writes each
function's worst error, in the function's own metric, with the input where it occurred, to
profiles/math_accuracy.json.  tests/test_gpu_math.py asserts the bounds with the same code
(select / errors below); this tool only records.

Metrics (the primitives table):
  ulp      error in ulps of the true result (results below 2^-1022: in units of 2^-1074)
  abs53    error in units of 2^-53, absolute (dsincos_t: table + angle addition)
  logabs   error in ulps of max(|log x|, 2^-8) (dlog_t: no relative path near 1)
  cabs     componentwise error in ulps of |z|, z the true complex result

Usage: python tools/math_accuracy.py [--out profiles/math_accuracy.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRUTH = os.path.join(ROOT, "tests", "golden", "math_truth.npz")

# function -> (group, metric, output labels, families outside the accuracy metric)
SPEC = {
    "dsincos": ("sincos", "ulp", ("sin", "cos"), ("nonfinite", "beyond_domain")),
    "dsincos_t": ("sincos", "abs53", ("sin", "cos"), ("nonfinite", "beyond_domain")),
    "dexp": ("exp", "ulp", ("exp",), ()),
    "dexp_nonpos": ("exp", "ulp", ("exp",), ()),
    "dexp_t": ("exp", "ulp", ("exp",), ()),
    "dexp_t_nonpos": ("exp", "ulp", ("exp",), ()),
    "dlog": ("log", "ulp", ("log",), ()),
    "dlog_t": ("log", "logabs", ("log",), ("not_positive_normal",)),
    "datan2": ("atan2", "ulp", ("atan2",), ("x_negative_zero", "nan", "infinite")),
    "datan2_t": ("atan2", "ulp", ("atan2",), ("x_negative_zero", "nan", "infinite", "zero_zero")),
    "drcp": ("rcp", "ulp", ("rcp",), ("subnormal", "huge")),
    "dsqrt_rsqrt": ("sqrt", "ulp", ("sqrt", "rsqrt"), ("zero_inf",)),
    "dsqrt_rsqrt_pos": ("sqrt", "ulp", ("sqrt", "rsqrt"), ("zero_inf",)),
    "csqrt_p": ("csqrt", "cabs", ("re", "im"), ()),
    "cdiv": ("cdiv", "cabs", ("re", "im"), ("zero_divisor",)),
    "cdiv_rcp": ("cdiv_rcp", "cabs", ("re", "im"), ()),
}
NONPOS = ("dexp_nonpos", "dexp_t_nonpos")          # probed on x <= 0 (and NaN) only


def load_truth(path=TRUTH):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def family(T, group, *names):
    """Mask of the group's points in the named families."""
    fams = list(T[group + "__families"])
    for n in names:
        if n not in fams:
            raise KeyError(f"{group}: no family {n}")
    return np.isin(T[group + "__fam"], [fams.index(n) for n in names])


def select(fn, T):
    """Indices of the group's points that fn is probed on."""
    g = SPEC[fn][0]
    x = T[g + "__x"]
    keep = ~(x > 0.0) if fn in NONPOS else np.ones(x.size, dtype=bool)
    return np.flatnonzero(keep)


def probe(fn, T, idx, math_probe):
    """fn over the selected points -> list of output arrays."""
    g = SPEC[fn][0]
    x = T[g + "__x"][idx]
    if g + "__bx" in T:
        x = np.concatenate([x, T[g + "__bx"][idx]])
        y = np.concatenate([T[g + "__y"][idx], T[g + "__by"][idx]])
    else:
        y = T[g + "__y"][idx] if g + "__y" in T and g in ("atan2", "csqrt") else None
    out = math_probe(fn, x, y)
    return list(out) if isinstance(out, tuple) else [out]


def errors(fn, T, idx, outs):
    """-> (err [n_out][n], counted [n]): each output's error in fn's metric at the selected points,
    and which of them count (finite truth, inside the accuracy families)."""
    g, metric, labels, outside = SPEC[fn]
    hi = [T[f"{g}__hi{k}"][idx] for k in range(len(labels))]
    lo = [T[f"{g}__lo{k}"][idx] for k in range(len(labels))]
    counted = ~family(T, g, *outside)[idx] if outside else np.ones(idx.size, dtype=bool)
    for h in hi:
        counted &= np.isfinite(h)
    with np.errstate(all="ignore"):
        if metric == "cabs":
            unit = [np.spacing(np.hypot(hi[0], hi[1]))] * 2
        elif metric == "abs53":
            unit = [np.full(idx.size, 2.0 ** -53)] * 2
        elif metric == "logabs":
            unit = [np.spacing(np.maximum(np.abs(hi[0]), 2.0 ** -8))]
        else:
            unit = [np.spacing(np.abs(h)) for h in hi]
        err = [np.abs((o - h) - l) / u for o, h, l, u in zip(outs, hi, lo, unit)]
    return err, counted


def worst(fn, T, idx, outs):
    """Per output label: the largest counted error and the input where it occurred."""
    g, metric, labels, _ = SPEC[fn]
    err, counted = errors(fn, T, idx, outs)
    rep = {}
    for lab, e in zip(labels, err):
        e = np.where(counted, e, -1.0)
        e = np.where(np.isnan(e), np.inf, e)
        w = int(np.argmax(e))
        at = {c: float(T[f"{g}__{c}"][idx][w]) for c in ("x", "y", "bx", "by") if f"{g}__{c}" in T}
        rep[lab] = {"max_err": float(e[w]), "at": at, "at_hex": {c: v.hex() for c, v in at.items()},
                    "points": int(counted.sum())}
    return {"metric": metric, "outputs": rep}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "math_accuracy.json"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "option-pricing-ffn-lbfgs_amd"))
    import torch  # noqa: F401  (before the first libdhcos call: one HIP runtime)
    from dhcos import _native
    T = load_truth()
    rep = {"fixture": "tests/golden/math_truth.npz", "probe": "dh_math_probe", "functions": {}}
    for fn in SPEC:
        idx = select(fn, T)
        rep["functions"][fn] = worst(fn, T, idx, probe(fn, T, idx, _native.math_probe))
        for lab, r in rep["functions"][fn]["outputs"].items():
            print(f"{fn:16s} {lab:6s} {rep['functions'][fn]['metric']:7s} max {r['max_err']:.4f} "
                  f"over {r['points']} points at {r['at']}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rep, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
