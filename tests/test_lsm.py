"""CPU checks of the least-squares Monte Carlo pricer of American and Bermudan options
(csrc/dh_lsm.h): every ValueError of dhcos.american_monte_carlo (raised before the
native library is loaded), the C-ABI's struct and enum against the binding, and the NumPy
restatement of the backward pass (tests/lsm_reference.py) against a binomial tree in the
Black-Scholes limit, with the method's recorded in-sample bias (tests/golden/lsm_bias.json)."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import lsm_reference as L
import mc_reference as R
from conftest import GOLDEN, ROOT

SPOT, RATE = 100.0, 0.03
HEADER = os.path.join(ROOT, "include", "dhcos.h")


def _with(**kw):
    p = dict(zip(["v1_0", "kappa1", "theta1", "sigma1", "rho1", "v2_0", "kappa2", "theta2",
                  "sigma2", "rho2", "lambda_j", "mu_j", "sigma_j"], R.README_PARAMS))
    p.update(kw)
    return p


def _opt(**kw):
    o = {"strike": 100.0, "maturity": 0.5, "option_type": "put"}
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
    "strike < 0": dict(options=_opt(strike=-1.0)),
    "strike not finite": dict(options=_opt(strike=np.inf)),
    "no options": dict(options=[]),
    "too many options": dict(options=_opt() * 17),
    "exercise_every = 0": dict(exercise_every=0),
    "exercise_every not whole": dict(exercise_every=1.5),
    "maturity no multiple of exercise_every": dict(exercise_every=5),    # step 32
    "one maturity no multiple": dict(options=_opt() + _opt(maturity=0.25), exercise_every=32),
    "storage cap": dict(n_paths=1 << 40),
    "storage cap by sets": dict(parameters=np.tile(R.README_PARAMS, (4096, 1)), n_paths=1 << 20,
                                options=_opt(maturity=1.0)),
}


@pytest.fixture
def no_native(monkeypatch):
    from dhcos import _native

    def refuse(*a, **k):
        raise AssertionError("the native library was reached")
    monkeypatch.setattr(_native, "load", refuse)
    monkeypatch.setattr(_native, "default_context", refuse)


@pytest.mark.parametrize("case", sorted(BAD_CALLS))
def test_american_monte_carlo_refuses_before_the_native_library(case, no_native):
    import dhcos
    kw = dict(parameters=_with(), spot=SPOT, risk_free=RATE, options=_opt(), n_paths=1024,
              steps_per_year=64, seed=0)
    kw.update(BAD_CALLS[case])
    args = [kw.pop(k) for k in ("parameters", "spot", "risk_free", "options")]
    with pytest.raises(ValueError):
        dhcos.american_monte_carlo(*args, **kw)


def test_valid_arguments_reach_the_native_library(no_native):
    """The refusals above are refusals of their one bad argument: the same call without it passes
    every check and goes on to the library (here replaced by a stub that says so)."""
    import dhcos
    with pytest.raises(AssertionError, match="native library was reached"):
        dhcos.american_monte_carlo(_with(), SPOT, RATE, _opt(), n_paths=1024)
    both = np.stack([R.README_PARAMS, R.STRESSED_PARAMS])
    with pytest.raises(AssertionError, match="native library was reached"):
        dhcos.american_monte_carlo(both, [100.0, 90.0], RATE,
                                   _opt() + _opt(maturity=0.25, option_type="call") * 15,
                                   n_paths=2, exercise_every=16, policy=True)
    # the largest call under the storage cap: 16 GiB exactly
    with pytest.raises(AssertionError, match="native library was reached"):
        dhcos.american_monte_carlo(_with(), SPOT, RATE, _opt(maturity=1.0), steps_per_year=4,
                                   n_paths=(16 << 30) // (24 * 4 + 12))


def test_instance_method_refusals(no_native):
    import dhcos
    dh = dhcos.DoubleHeston(100, 105, 0.5, 0.03, *R.README_PARAMS, option_type="put")
    with pytest.raises(ValueError):
        dh.american_monte_carlo(n_paths=1)
    with pytest.raises(ValueError):
        dh.american_monte_carlo(exercise_every=5)
    with pytest.raises(ValueError):
        dhcos.DoubleHeston(100, 105, 0.5, 0.03, *R.README_PARAMS, q=0.01).american_monte_carlo()
    with pytest.raises(AssertionError, match="native library was reached"):
        dh.american_monte_carlo(n_paths=1024, exercise_every=4)


# ---- the C-ABI ------------------------------------------------------------------------------------
def _header_code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_option_struct_matches_the_header():
    from dhcos import _native
    body = re.search(r"typedef struct \{([^{}]*)\} dh_lsm_option;", _header_code()).group(1)
    want = [tuple(" ".join(d.split()).split(" ")) for d in body.split(";") if d.strip()]
    assert want == [("int32_t", "is_call"), ("int32_t", "pad"), ("double", "strike"),
                    ("double", "maturity")]
    ctype = {"int32_t": C.c_int32, "double": C.c_double}
    got = _native.LsmOption._fields_
    assert [f for f, _ in got] == [f for _, f in want]
    assert all(ty is ctype[cty] for (_, ty), (cty, _) in zip(got, want))
    assert C.sizeof(_native.LsmOption) == 24
    assert [getattr(_native.LsmOption, f).offset for f, _ in got] == [0, 4, 8, 16]


def test_limits_match_the_header_enum():
    from dhcos import _native, american
    enums = {}
    for body in re.findall(r"enum \{([^{}]*)\}", _header_code()):
        enums.update((k, int(v)) for k, v in re.findall(r"(DH_[A-Z_]+) = (-?\d+)", body))
    lsm = {k[3:]: v for k, v in enums.items() if k.startswith("DH_LSM_")}
    assert lsm == {"LSM_MAX_OPTIONS": 16, "LSM_BASIS": 10, "LSM_MIN_ITM": 64,
                   "LSM_SLOTS": lsm["LSM_SLOTS"], "LSM_MAX_GIB": lsm["LSM_MAX_GIB"]}
    for name, v in lsm.items():
        assert getattr(_native, name) == v, name
        assert name in _native.__all__
    mirrored = {n for n in vars(_native) if n.startswith("LSM_")}
    assert mirrored == set(lsm)
    assert (L.BASIS, L.MIN_ITM) == (_native.LSM_BASIS, _native.LSM_MIN_ITM)
    assert american.MAX_OPTIONS == 16 and american.MAX_BYTES == lsm["LSM_MAX_GIB"] << 30
    assert "LsmOption" in _native.__all__


def test_library_exports_the_new_symbols():
    from dhcos import _native
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (dh_[a-z_]+)\b", out))
    assert {"dh_lsm_price", "dh_lsm_price_dev"} <= exported
    assert list(_native.SIGNATURES)[-2:] == ["dh_lsm_price", "dh_lsm_price_dev"]


def test_native_refusals_need_no_device():
    """The C-ABI's own argument checks run before any device work: a null context here."""
    from dhcos import _native
    lib = _native.load()
    opt = (_native.LsmOption * 1)(_native.LsmOption(0, 0, 100.0, 0.5))
    assert lib.dh_lsm_price(None, None, 1, opt, 1, 1024, 64, 1, 0, None, None, None, None, None,
                            None) == -1
    assert b"null" in lib.dh_last_error()
    assert lib.dh_lsm_price_dev(None, None, 1, opt, 1, 1024, 64, 1, 0, None, None, None, None,
                                None, None, None) == -1


# ---- the restatement ------------------------------------------------------------------------------
def test_binomial_tree_against_closed_forms():
    """The tree's European value against Black-Scholes, and a Bermudan put between its European
    value and the same tree with more dates."""
    from math import erf, exp, log, sqrt
    S, K, r, s, T = L.BS_SPOT, 110.0, L.BS_RATE, L.BS_SIGMA, L.BS_T
    d1 = (log(S / K) + (r + 0.5 * s * s) * T) / (s * sqrt(T))

    def cdf(x):
        return 0.5 * (1.0 + erf(x / sqrt(2.0)))
    put = K * exp(-r * T) * cdf(-(d1 - s * sqrt(T))) - S * cdf(-d1)
    b8, e8 = L.crr_bermudan(S, K, r, s, T, 8, 250)
    b16, e16 = L.crr_bermudan(S, K, r, s, T, 16, 125)
    assert e8 == e16 and abs(e8 - put) < 2e-3
    assert e8 < b8 < b16
    # one date: the European value, whatever the tree; a call without dividends is never
    # exercised early
    b1, e1 = L.crr_bermudan(S, K, r, s, T, 1, 500)
    assert b1 == e1
    bc, ec = L.crr_bermudan(S, 90.0, r, s, T, 8, 100, is_call=True)
    assert abs(bc - ec) < 1e-12 * ec


def test_backward_pass_rules_on_a_hand_case():
    """Skip rule and bookkeeping: with fewer than 64 paths in the money nobody exercises early,
    every coefficient row is NaN and the price is the discounted maturity payoff."""
    rs = np.random.RandomState(0)
    n = 200
    S = 100.0 * np.exp(0.1 * rs.randn(n, 3))
    S[:, :2] = np.maximum(S[:, :2], 101.0)             # out of the money before maturity
    S[:40, 1] = 95.0                                   # ... but for 40 paths at date 2
    st = np.stack([S, np.full((n, 3), 0.04), np.full((n, 3), 0.04)], axis=2)
    out = L.backward_one(st, 100.0, False, 3, 0.05, 0.25, 0.04, 0.04)
    assert np.all(np.isnan(out["coef"])) and np.all(out["exercise_date"] == 3)
    disc = np.exp(-0.05 * 0.25)
    want = disc * np.mean(disc * (disc * np.maximum(100.0 - S[:, 2], 0.0)))
    assert abs(out["price"] - want) <= 4e-16 * want
    assert abs(out["european"] - want) <= 1e-15 * want
    # fewer dates than the states hold: the later dates are not read
    two = L.backward_one(st, 100.0, False, 2, 0.05, 0.25, 0.04, 0.04)
    assert np.all(two["exercise_date"] == 2)
    assert two["price"] == pytest.approx(disc * disc * np.mean(np.maximum(100.0 - S[:, 1], 0.0)),
                                         rel=1e-15)


@pytest.fixture(scope="module")
def bias():
    with open(os.path.join(GOLDEN, L.BIAS_FILE)) as fh:
        return json.load(fh)


def test_bias_fixture_is_the_configuration_the_tests_run(bias):
    assert bias["strikes"] == list(L.BS_STRIKES) and bias["seeds"] == list(L.BS_FIT_SEEDS)
    assert (bias["spot"], bias["rate"], bias["sigma"], bias["maturity"]) == (
        L.BS_SPOT, L.BS_RATE, L.BS_SIGMA, L.BS_T)
    assert (bias["dates"], bias["steps_per_year"], bias["n_paths"]) == (
        L.BS_DATES, L.BS_SPY, L.BS_PATHS)
    assert L.BS_TEST_SEED not in bias["seeds"]
    # the limit: v0 = theta, sigma = 1e-3 in both factors, no jumps, total variance sigma^2
    p = L.BS_PARAMS
    assert p[0] == p[2] and p[5] == p[7] and p[3] == p[8] == 1e-3 and p[10] == 0.0
    assert p[2] + p[7] == 0.04 and abs(L.BS_SIGMA ** 2 - 0.04) < 1e-17
    tree = L.bs_tree()
    assert np.allclose([t[0] for t in tree], bias["tree"], rtol=1e-12, atol=0)
    assert np.allclose([t[1] for t in tree], bias["tree_european"], rtol=1e-12, atol=0)


def test_restatement_prices_bermudan_puts_of_the_tree(bias):
    """Puts at K / S0 = 0.9, 1.0, 1.1, r = 0.05, T = 1, 8 exercise dates, 2^15 paths, a seed the
    recorded bias did not see: |LSM - tree| <= |recorded mean bias| + 4 stderr, and the tree's
    early-exercise premium exceeds that allowance at every strike (else the bound would also pass
    a pricer that never exercises early)."""
    out = L.bs_restatement(L.BS_TEST_SEED)
    assert not np.any(np.isnan(out["coef"][:, :L.BS_DATES - 1]))       # every date fitted
    assert np.all(np.isnan(out["coef"][:, L.BS_DATES - 1]))
    for j, k in enumerate(L.BS_STRIKES):
        tree, euro = bias["tree"][j], bias["tree_european"][j]
        allow = abs(bias["mean_bias"][j]) + 4.0 * out["stderr"][j]
        diff = out["price"][j] - tree
        print(f"K {k}: LSM {out['price'][j]:.4f} +- {out['stderr'][j]:.4f}, tree {tree:.4f} "
              f"(European {euro:.4f}), LSM - tree {diff:+.4f}, allowance {allow:.4f}, recorded "
              f"mean bias {bias['mean_bias'][j]:+.4f}, max z {bias['max_z'][j]:.2f}")
        assert tree - euro > allow, (k, tree - euro, allow)
        assert abs(diff) <= allow, (k, diff, allow)
        assert abs(out["european"][j] - euro) <= 4.0 * out["european_stderr"][j] + 2e-3


@pytest.mark.parametrize("n_paths, options", [(4096, L.DEV_OPTIONS), (1000, L.DEV_OPTIONS)])
def test_device_comparison_seed_does_not_hang_on_the_solver(n_paths, options):
    """The seed the GPU tests compare exercise dates on: solving by least squares on the design
    matrix instead of the normal equations changes no path's exercise date (mc_reference's paths,
    both parameter sets), so the comparison asks of the device nothing the restatement itself
    would not meet; and early exercise happens, so the comparison sees the rule at work."""
    obs = tuple(range(L.DEV_EVERY, L.DEV_SPY + 1, L.DEV_EVERY))
    for p in (R.README_PARAMS, R.STRESSED_PARAMS):
        _, st = R.simulate(p, L.DEV_SPOT, L.DEV_RATE, np.arange(n_paths), L.DEV_SPY, L.DEV_SPY,
                           L.DEV_SEED, obs)
        a = L.restate(st, p, options)
        b = L.restate(st, p, options, solver="lstsq")
        assert np.array_equal(a["exercise_date"], b["exercise_date"])
        dates = np.array(L.option_columns(options)[2])
        assert np.mean(a["exercise_date"] < dates[:, None]) > 0.05
        assert np.array_equal(np.isnan(a["coef"][..., 0]), np.isnan(b["coef"][..., 0]))
