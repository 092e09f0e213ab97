"""CPU checks of the Monte Carlo pricer: the NumPy restatement of DESIGN.md 3.15
(tests/mc_reference.py) against Philox's known answers, against the oracle's COS prices, against
the 50-digit walk of the same step (tests/golden/mc_truth.npz) and against the CIR moments, every
ValueError of dhcos.monte_carlo (raised before the native library is loaded), and the three new
exports of libdhcos.so."""
import os
import re
import subprocess

import numpy as np
import pytest

import mc_reference as R
from conftest import GOLDEN
from oracle import dh_oracle as O

SPOT, RATE = 100.0, 0.03
CALLS = [{"strike": float(k), "maturity": float(t), "option_type": "call"}
         for k, t in zip(R.GRID_K, R.GRID_T)]


@pytest.mark.parametrize("ctr, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, want):
    got = R.philox4x32_10(*ctr, *key)
    assert " ".join("%08x" % int(w) for w in got) == want
    # vectorised over counters: the same words at any place in an array
    c0 = np.array([5, ctr[0], 7], dtype=np.uint64)
    vec = R.philox4x32_10(c0, ctr[1], ctr[2], ctr[3], *key)
    assert " ".join("%08x" % int(w[1]) for w in vec) == want


def test_uniform_and_normal_maps():
    top = np.uint64(0xFFFFFFFF)
    assert R.uniform(np.uint64(0), np.uint64(0)) == 2.0 ** -53
    assert R.uniform(top, top) == 1.0 - 2.0 ** -53
    assert R.uniform(np.uint64(1 << 31), np.uint64(0)) == 0.5 + 2.0 ** -53
    u = R.draws(7, np.arange(20000), 3)
    for k in (0, 3, 6):                                   # the uniforms
        assert 0.0 < u[k].min() and u[k].max() < 1.0
        assert abs(u[k].mean() - 0.5) < 4 / np.sqrt(12 * 20000)
    for k in (1, 2, 4, 5, 7):                             # the normals
        assert abs(u[k].mean()) < 4 / np.sqrt(20000) and abs(u[k].std() - 1) < 4 / np.sqrt(40000)
    # a path's draws depend on (seed, path, step) alone
    one = R.draws(7, np.array([123]), 3)
    assert all(a[123] == b[0] for a, b in zip(u, one))


def test_restatement_prices_the_model_of_the_cos_pricer():
    """2^17 paths at 32 steps per year on the generator's 15 calls: every price within 4 of its
    standard errors of the oracle's COS price (N = 512), the discounted mean of S_T within 4 of
    its own of spot.  No allowance for time-step bias."""
    price, err, fwd, fwd_err = R.price(R.README_PARAMS, SPOT, RATE, CALLS, 1 << 17, 32, seed=2024)
    cos = O.price_many(R.README_PARAMS, SPOT, R.GRID_K, R.GRID_T, RATE, True, 512)
    z = np.abs(price - cos) / err
    zf = np.abs(fwd - SPOT) / fwd_err
    print(f"max |MC - COS| / stderr {z.max():.2f}; forward {zf.max():.2f}")
    assert np.all(z <= 4.0), z
    assert np.all(zf <= 4.0), zf


# ---- the 50-digit truth fixture (tests/golden/make_mc_truth.py) -----------------------------------
@pytest.fixture(scope="module")
def truth():
    with np.load(os.path.join(GOLDEN, R.TRUTH_FILE)) as z:
        return {k: z[k] for k in z.files}


def test_truth_fixture_is_the_configuration_the_tests_walk(truth):
    """The fixture's pin: it holds the configuration of mc_reference.TRUTH_*, reaches every branch
    of the step away from the switches, and its stored errors are those of its stored restatement
    (a fresh computation: truth_errors in plain float64)."""
    n = R.TRUTH_PATHS.size
    assert np.array_equal(truth["paths"], R.TRUTH_PATHS) and truth["paths"].dtype == np.uint64
    assert int(truth["seed"]) == R.TRUTH_SEED == 0x9E3779B900000005
    assert np.array_equal(truth["sets"], R.TRUTH_SETS)
    assert (int(truth["steps_per_year"]), tuple(truth["obs_steps"])) == (R.TRUTH_SPY, R.TRUTH_OBS)
    assert (float(truth["spot"]), float(truth["rate"])) == (R.TRUTH_SPOT, R.TRUTH_RATE)
    # the high words: the seed's is live, the paths' take three values and carry inside a wave
    assert R.TRUTH_SEED >> 32 != 0
    assert {int(p) >> 32 for p in R.TRUTH_PATHS} == {0, 1, 5}
    assert {(1 << 32) - 1, 1 << 32} <= {int(p) for p in R.TRUTH_PATHS}
    # the two degenerate sets are what the validation just admits
    z, c = R.TRUTH_SETS[2], R.TRUTH_SETS[3]
    assert z[0] == z[5] == z[10] == 0.0 and (z[4], z[9]) == (0.999, -0.999)
    assert c[12] == 0.0 and c[10] / R.TRUTH_SPY == 1.0 and c[11] == -0.04
    hi, lo = truth["truth"], truth["truth_lo"]
    assert hi.shape == lo.shape == truth["restatement"].shape == (4, n, 3, 6)
    assert np.all(np.isfinite(hi)) and np.all(np.abs(lo) <= 0.5 * np.spacing(np.abs(hi)))
    counts = dict(zip(truth["count_names"].tolist(), truth["counts"].tolist()))
    assert set(counts) == {"quad", "expo", "zero", "n1", "n2"} and min(counts.values()) > 0, counts
    assert counts["quad"] + counts["expo"] == 4 * n * 8 * 2
    assert 0 < np.sum(hi[..., 1:3] == 0.0) <= counts["zero"] <= counts["expo"]
    assert truth["psi_gap"] > 1e-9 and truth["u_gap"] > 1e-9
    rel, ab = R.truth_errors(truth["restatement"], hi, lo)
    assert np.array_equal(rel, truth["rel_err"]) and np.array_equal(ab, truth["abs_err"])
    assert os.path.getsize(os.path.join(GOLDEN, R.TRUTH_FILE)) < (1 << 16)


def test_restatement_matches_the_50_digit_truth(truth):
    """The NumPy restatement, run here, against the mpmath walk of the same step: 4e-15 relative on
    all six statistics, plus 1e-15 absolute on the variances; an exact 0 of the truth (the
    exponential branch's v' = 0) is an exact 0.  Measured where the fixture was generated: 5.5e-16
    on S, max, min, sum; 2.7e-15 / 4.2e-15 on v1 / v2 (both at the v0 = 0 set, on variances below
    1e-2, where the absolute 6e-17 is what counts), 2.3e-16 absolute.  exp, log, sin and cos of
    NumPy differ in the last bit between CPUs, so the stored figures are pinned to the stored
    restatement (test above) and this run to the bar."""
    hi, lo = truth["truth"], truth["truth_lo"]
    stats = R.new_stats()
    got = R.truth_restatement(stats)
    assert stats["psi_gap"] > 1e-9 and stats["u_gap"] > 1e-9, stats
    counts = dict(zip(truth["count_names"].tolist(), truth["counts"].tolist()))
    assert {k: stats[k] for k in counts} == counts        # the same decisions as the truth's
    zero = hi == 0.0
    assert zero.any() and not zero[..., [0, 3, 4, 5]].any()
    assert np.all(got[zero] == 0.0) and np.all(got[~zero] != 0.0)
    rel, ab = R.truth_errors(got, hi, lo)
    print(f"restatement vs 50-digit truth: worst relative error (S, v1, v2, max, min, sum) {rel}; "
          f"worst absolute error on v1, v2 {ab}; stored {truth['rel_err']}, {truth['abs_err']}")
    bar = 4e-15 * np.abs(hi)
    bar[..., 1:3] += 1e-15
    d = np.abs((got - hi) - lo)
    assert np.all(d <= bar), float(np.max(d[~zero] / bar[~zero]))
    # the stored restatement passes the same bar: its figures are fit to scale the device's bar
    assert np.all(np.abs((truth["restatement"] - hi) - lo) <= bar)


@pytest.mark.parametrize("which", [0, 1])
def test_restatement_has_the_cir_moments(which):
    """2^16 paths, 8 steps per year, step 8, seed 0x9E3779B900000005: the sample mean and variance
    of v1 and v2 within 4 of their standard errors of the CIR closed forms, the discounted mean of
    S_T within 4 of its own of spot (mc_reference.moment_z_scores has the derivation).  4 is the
    statistical bar alone."""
    p = R.TRUTH_SETS[which]
    state, _ = R.simulate(p, SPOT, RATE, np.arange(1 << 16), 8, 8, R.TRUTH_SEED)
    z = R.moment_z_scores(p, state, SPOT, RATE, 1.0)
    print(f"restatement moments, set {which}: " + ", ".join(f"{k} {v:.2f}" for k, v in z.items()))
    assert all(v <= 4.0 for v in z.values()), z


def test_cir_closed_forms_are_the_fixed_point_of_the_step_recursion():
    """E[v'] = theta + (E[v] - theta) E and Var[v'] = K1 E[v] + K2 + E^2 Var[v], iterated 8 times
    from (v0, 0), give the closed forms at T = 1 to rounding."""
    for p in (R.README_PARAMS, R.STRESSED_PARAMS):
        for i in (0, 1):
            v0, kappa, theta, sigma = p[5 * i:5 * i + 4]
            f = R.Factor(kappa, theta, sigma, 0.0, 1.0 / 8)
            mean, var = v0, 0.0
            for _ in range(8):
                mean, var = theta + (mean - theta) * f.e, f.k1 * mean + f.k2 + f.e * f.e * var
            want_m, want_v = R.cir_moments(v0, kappa, theta, sigma, 1.0)
            assert abs(mean - want_m) <= 1e-15 * want_m and abs(var - want_v) <= 2e-15 * want_v


# ---- every refusal of dhcos.monte_carlo, without the native library --------------------------------
def _with(**kw):
    p = dict(zip(["v1_0", "kappa1", "theta1", "sigma1", "rho1", "v2_0", "kappa2", "theta2",
                  "sigma2", "rho2", "lambda_j", "mu_j", "sigma_j"], R.README_PARAMS))
    p.update(kw)
    return p


def _opt(**kw):
    o = {"strike": 100.0, "maturity": 0.5, "option_type": "call"}
    o.update(kw)
    return [o]


BAD_CALLS = {
    "nan parameter": dict(parameters=_with(mu_j=np.nan)),
    "infinite rate": dict(risk_free=np.inf),
    "v0 < 0": dict(parameters=_with(v2_0=-1e-3)),
    "kappa = 0": dict(parameters=_with(kappa1=0.0)),
    "theta < 0": dict(parameters=_with(theta2=-0.04)),
    "sigma = 0": dict(parameters=_with(sigma1=0.0)),
    "rho = 1": dict(parameters=_with(rho1=1.0)),
    "rho < -1": dict(parameters=_with(rho2=-1.5)),
    "lambda < 0": dict(parameters=_with(lambda_j=-0.1)),
    "lambda dt > 1": dict(parameters=_with(lambda_j=65.0)),
    "sigma_j < 0": dict(parameters=_with(sigma_j=-0.1)),
    "spot = 0": dict(spot=0.0),
    "missing name": dict(parameters={"kappa1": 2.0}),
    "wrong width": dict(parameters=np.ones((2, 12))),
    "spot shape": dict(spot=np.array([100.0, 101.0])),
    "n_paths = 1": dict(n_paths=1),
    "steps_per_year = 0": dict(steps_per_year=0),
    "seed < 0": dict(seed=-1),
    "maturity off the grid": dict(options=_opt(maturity=0.51)),
    "maturity below one step": dict(options=_opt(maturity=0.001)),
    "unknown kind": dict(options=_opt(kind="lookback")),
    "barrier = 0": dict(options=_opt(kind="up_and_out", barrier=0.0)),
    "barrier < 0": dict(options=_opt(kind="down_and_out", barrier=-5.0)),
    "barrier missing": dict(options=_opt(kind="up_and_out")),
    "strike < 0": dict(options=_opt(strike=-1.0)),
    "no options": dict(options=[]),
    "too many options": dict(options=_opt() * 65),
}


@pytest.fixture
def no_native(monkeypatch):
    from dhcos import _native

    def refuse(*a, **k):
        raise AssertionError("the native library was reached")
    monkeypatch.setattr(_native, "load", refuse)
    monkeypatch.setattr(_native, "default_context", refuse)


@pytest.mark.parametrize("case", sorted(BAD_CALLS))
def test_monte_carlo_refuses_before_the_native_library(case, no_native):
    import dhcos
    kw = dict(parameters=_with(), spot=SPOT, risk_free=RATE, options=_opt(), n_paths=1024,
              steps_per_year=64, seed=0)
    kw.update(BAD_CALLS[case])
    args = [kw.pop(k) for k in ("parameters", "spot", "risk_free", "options")]
    with pytest.raises(ValueError):
        dhcos.monte_carlo(*args, **kw)


def test_simulate_paths_and_instance_refusals(no_native):
    import dhcos
    from dhcos.montecarlo import simulate_paths
    for kw in (dict(obs_steps=[]), dict(obs_steps=[0, 1]), dict(obs_steps=[2, 2]),
               dict(obs_steps=[1.5]), dict(n_paths=0), dict(path0=-1),
               dict(parameters=_with(sigma2=0.0))):
        full = dict(parameters=_with(), obs_steps=[1, 2], n_paths=4, path0=0)
        full.update(kw)
        with pytest.raises(ValueError):
            simulate_paths(full.pop("parameters"), SPOT, RATE, full.pop("obs_steps"), **full)
    dh = dhcos.DoubleHeston(100, 105, 0.5, 0.03, *R.README_PARAMS, option_type="call")
    with pytest.raises(ValueError):
        dh.monte_carlo(n_paths=1)
    with pytest.raises(ValueError):
        dhcos.DoubleHeston(100, 105, 0.5, 0.03, *R.README_PARAMS, q=0.01).monte_carlo()


def test_valid_arguments_reach_the_native_library(no_native):
    """The refusals above are refusals of their one bad argument: the same call without it passes
    every check and goes on to the library (here replaced by a stub that says so)."""
    import dhcos
    with pytest.raises(AssertionError, match="native library was reached"):
        dhcos.monte_carlo(_with(), SPOT, RATE, _opt(), n_paths=1024)
    both = np.stack([R.README_PARAMS, R.STRESSED_PARAMS])
    with pytest.raises(AssertionError, match="native library was reached"):
        dhcos.monte_carlo(both, [100.0, 90.0], RATE,
                          _opt(kind="down_and_out", barrier=80.0, option_type="put"), n_paths=2)


def test_library_exports_the_new_symbols():
    from dhcos import _native
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (dh_[a-z_]+)\b", out))
    assert {"dh_mc_price", "dh_mc_price_dev", "dh_mc_paths"} <= exported
    assert {"dh_mc_price", "dh_mc_price_dev", "dh_mc_paths"} <= set(_native.SIGNATURES)
