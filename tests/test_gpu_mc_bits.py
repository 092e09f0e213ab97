"""The Monte Carlo entry points against their own recorded bits (tests/golden/mc_parent_bits.json).

The fixture was recorded on an MI355X at the commit before the path walkers were consolidated (one
step, one price kernel, one paths kernel), through the same C-ABI and from this module's own list
of cases: ``python tests/test_gpu_mc_bits.py`` rewrites it.  Every output of every case must be
equal bit for bit: arrays of up to 64 values are held as ``float.hex`` strings, larger ones as the
SHA-256 of their little-endian bytes.  The cases are the smallest that reach what the
consolidation touched: two chunks with one live lane in the second, all four option kinds with two
options on one step and a strike of 0, a set without jumps (the jump draw is voted away) and one
with lambda dt near 1, a block that sums two chunks (more chunks than slots), a path counter whose
low word carries, a ragged second wave, and the Longstaff-Schwartz pricer on the walker's paths.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

import mc_reference as R

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mc_parent_bits.json")
SPOT, RATE, SEED = 100.0, 0.03, 7
ANTI, CTRL = 1, 2                              # DH_MC_VR_ANTITHETIC, DH_MC_VR_CONTROL
VR_NAMES = ("price", "stderr", "base_price", "base_stderr", "beta", "control_mean")

EIGHT = [                                      # steps 2, 4, 8 of 8 per year; two share step 4
    {"strike": 100.0, "maturity": 0.25, "option_type": "call"},
    {"strike": 95.0, "maturity": 1.0, "option_type": "put"},
    {"strike": 100.0, "maturity": 0.5, "option_type": "call", "kind": "asian"},
    {"strike": 105.0, "maturity": 1.0, "option_type": "put", "kind": "asian"},
    {"strike": 100.0, "maturity": 0.5, "option_type": "call", "kind": "up_and_out",
     "barrier": 120.0},
    {"strike": 110.0, "maturity": 1.0, "option_type": "put", "kind": "up_and_out",
     "barrier": 115.0},
    {"strike": 90.0, "maturity": 0.25, "option_type": "call", "kind": "down_and_out",
     "barrier": 92.0},
    {"strike": 0.0, "maturity": 1.0, "option_type": "call", "kind": "asian"},
]
ONE = [{"strike": 100.0, "maturity": 1.0, "option_type": "call"}]
LSM = [{"strike": 100.0, "maturity": 1.0, "option_type": "put"},      # 4 dates
       {"strike": 100.0, "maturity": 0.5, "option_type": "call"}]     # 2 dates


def _records(spy):
    """Two sets: no jumps, and the stressed set with lambda_j / steps_per_year = 0.95."""
    from dhcos import _native
    sets = np.stack([R.README_PARAMS, R.STRESSED_PARAMS])
    sets[0, 10] = 0.0
    sets[1, 10] = 0.95 * spy
    rec = np.zeros((2, _native.PARAM_STRIDE))
    rec[:, :13] = sets
    rec[:, 13], rec[:, 14] = SPOT, RATE
    return rec


def _price(ctx, options, walks, spy, flags):
    from dhcos.montecarlo import _options
    n = 2 * walks if flags & ANTI else walks          # `walks` samples: pairs under ANTI
    if flags == 0:
        out = ctx.mc_price(_records(spy), _options(options, spy), n, spy, SEED)
    else:
        out = ctx.mc_price_vr(_records(spy), _options(options, spy), n, spy, SEED, flags)
    return dict(zip(VR_NAMES, out))


def _paths(ctx, mirror):
    rec, obs = _records(8), np.array([1, 3, 8], dtype=np.int32)
    if mirror is None:
        return {"paths": ctx.mc_paths(rec, obs, 2 ** 32 - 3, 70, 8, SEED)}
    return {"paths": ctx.mc_paths_vr(rec, obs, 2 ** 32 - 3, 70, 8, SEED, mirror)}


def _lsm(ctx):
    from dhcos.american import _options
    opts, dates = _options(LSM, 8, 2)
    out = ctx.lsm_price(_records(8), opts, dates, 257, 8, 2, SEED, policy=True)
    return dict(zip(("price", "stderr", "european", "european_stderr", "coef", "exercise_date"),
                    out))


CASES = {}
for _f in (0, ANTI, CTRL, ANTI | CTRL):
    CASES[f"price_257_flags{_f}"] = lambda ctx, f=_f: _price(ctx, EIGHT, 257, 8, f)
    CASES[f"price_block_loop_flags{_f}"] = lambda ctx, f=_f: _price(ctx, ONE, 1025 * 256, 2, f)
CASES["paths"] = lambda ctx: _paths(ctx, None)
CASES["paths_vr_mirror0"] = lambda ctx: _paths(ctx, 0)
CASES["paths_vr_mirror1"] = lambda ctx: _paths(ctx, 1)
CASES["lsm_257"] = _lsm


def _bits(a):
    a = np.ascontiguousarray(a)
    if a.size <= 64 and a.dtype == np.float64:
        return [float(v).hex() for v in a.ravel()]
    return {"shape": list(a.shape), "dtype": a.dtype.newbyteorder("<").str,
            "sha256": hashlib.sha256(a.astype(a.dtype.newbyteorder("<")).tobytes()).hexdigest()}


def _run(name, ctx):
    return {k: _bits(v) for k, v in CASES[name](ctx).items()}


@pytest.fixture(scope="module")
def ctx():
    from dhcos import _native
    return _native.default_context()


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as fh:
        return json.load(fh)


def test_the_fixture_holds_every_case(recorded):
    assert sorted(recorded) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_bits_of_the_parent_commit(ctx, recorded, name):
    got, want = _run(name, ctx), recorded[name]
    assert sorted(got) == sorted(want)
    for field in want:
        assert got[field] == want[field], (name, field)


if __name__ == "__main__":
    import torch  # noqa: F401  before the first libdhcos call: one HIP runtime (dhcos/_native.py)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "option-pricing-ffn-lbfgs_amd")]
    from dhcos import _native
    context = _native.default_context()
    result = {name: _run(name, context) for name in sorted(CASES)}
    out = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    with open(out, "w") as fh:
        json.dump(result, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(f"{out}: {len(result)} cases")
