"""CPU checks of the Monte Carlo pricer: the NumPy restatement of DESIGN.md 3.15
(tests/mc_reference.py) against Philox's known answers and against the oracle's COS prices, every
ValueError of dhcos.monte_carlo (raised before the native library is loaded), and the three new
exports of libdhcos.so."""
import re
import subprocess

import numpy as np
import pytest

import mc_reference as R
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
