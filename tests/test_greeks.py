"""CPU checks of the analytic COS Greeks: the NumPy restatement (tests/greeks_reference.py) against
the oracle's price and against central differences of it, and dhcos.greeks' argument checks."""
import numpy as np
import pytest

import greeks_reference as G
from oracle import dh_oracle as O

PRM = [0.04, 2.0, 0.04, 0.3, -0.5, 0.04, 1.5, 0.04, 0.2, -0.3, 0.5, -0.05, 0.10]
PRM2 = [0.03, 3.1, 0.05, 0.42, -0.7, 0.06, 0.8, 0.03, 0.18, -0.25, 0.15, -0.03, 0.07]
S0, R = 100.0, 0.03

# (params, K, T, is_call, N, q): calls and puts, T from 0.1 to 2, N in {128, 512}; the clamp is
# inactive in every one (asserted)
CASES = [
    (PRM, 100.0, 1.0, True, 128, 0.0),
    (PRM, 90.0, 0.1, False, 128, 0.0),
    (PRM, 110.0, 2.0, True, 512, 0.0),
    (PRM2, 105.0, 0.5, False, 512, 0.0),
    (PRM2, 95.0, 0.25, True, 128, 0.02),
    (PRM2, 120.0, 1.5, False, 128, 0.0),
    (PRM, 80.0, 0.75, True, 512, 0.01),
]
IDS = [f"{'call' if c[3] else 'put'}-K{c[1]:g}-T{c[2]:g}-N{c[4]}" for c in CASES]


def _price(prm, s0, K, T, call, N, q):
    return O.price_vec(prm, s0, K, T, R, call, N, q)


@pytest.fixture(scope="module")
def planes():
    return [G.greeks_vec(prm, S0, K, T, R, call, N, q) for prm, K, T, call, N, q in CASES]


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_price_plane_is_price_vec(planes, i):
    prm, K, T, call, N, q = CASES[i]
    assert planes[i]["price"] == _price(prm, S0, K, T, call, N, q)       # bit for bit


def test_price_plane_is_price_vec_on_a_clamped_option():
    for K, call in ((5.0, True), (3000.0, False)):
        assert G.clamp_active(PRM, S0, K, 0.1, R)
        assert G.greeks_vec(PRM, S0, K, 0.1, R, call, 256)["price"] == \
            O.price_vec(PRM, S0, K, 0.1, R, call, 256)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_spot_and_strike_greeks_match_central_differences(planes, i):
    """delta, gamma and dual delta against central differences of price_vec, spot step 1e-3 S0
    (strike step 1e-3 K), to 1e-4 relative: the quotient's own h^2 error."""
    prm, K, T, call, N, q = CASES[i]
    assert not G.clamp_active(prm, S0, K, T, R)
    h = 1e-3 * S0
    for s in (S0 - h, S0 + h):                        # and at the bumped spots
        assert not G.clamp_active(prm, s, K, T, R)
    up, mid, dn = (_price(prm, s, K, T, call, N, q) for s in (S0 + h, S0, S0 - h))
    hk = 1e-3 * K
    kup, kdn = (_price(prm, S0, k, T, call, N, q) for k in (K + hk, K - hk))
    fd = {"delta": (up - dn) / (2 * h), "gamma": (up - 2 * mid + dn) / h ** 2,
          "dual_delta": (kup - kdn) / (2 * hk)}
    for name, want in fd.items():
        got = planes[i][name]
        print(f"{IDS[i]} {name}: analytic {got:.12e} fd {want:.12e} rel {abs(got / want - 1):.2e}")
        assert abs(got - want) <= 1e-4 * abs(want), name


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_vegas_match_central_differences(planes, i):
    """vega1, vega2 against central differences in v01, v02 (step 1e-5) to 1e-7 relative.  The
    largest difference is the short put's (PRM, K = 90, T = 0.1, N = 128): 7.4e-8 and 7.7e-8, the
    quotient's own h^2 error where the price curves most in v0; every other case is below 4e-9."""
    prm, K, T, call, N, q = CASES[i]
    assert not G.clamp_active(prm, S0, K, T, R)
    for name, idx in (("vega1", 0), ("vega2", 5)):
        hi, lo = list(prm), list(prm)
        hi[idx] += 1e-5
        lo[idx] -= 1e-5
        for bumped in (hi, lo):                       # v0 moves the cumulant range
            assert not G.clamp_active(bumped, S0, K, T, R)
        want = (_price(hi, S0, K, T, call, N, q) - _price(lo, S0, K, T, call, N, q)) \
            / (hi[idx] - lo[idx])
        got = planes[i][name]
        print(f"{IDS[i]} {name}: analytic {got:.12e} fd {want:.12e} rel {abs(got / want - 1):.2e}")
        assert abs(got - want) <= 1e-7 * abs(want), name


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_euler_identity(planes, i):
    """price = S0 delta + K dual_delta (the series is homogeneous of degree one in (S0, K) at a
    fixed range) to 1e-13 relative."""
    prm, K, T, call, N, q = CASES[i]
    g = planes[i]
    rel = abs(S0 * g["delta"] + K * g["dual_delta"] - g["price"]) / abs(g["price"])
    print(f"{IDS[i]}: euler rel {rel:.2e}")
    assert rel <= 1e-13


def _good():
    return dict(parameters=PRM, spot=S0, risk_free=R,
                options=[{"strike": 100.0, "maturity": 1.0, "option_type": "call"}])


@pytest.mark.parametrize("change, word", [
    (dict(parameters=PRM[:12]), "parameters"),
    (dict(parameters=np.zeros((2, 3, 13))), "parameters"),
    (dict(parameters={"v1_0": 0.04}), "parameters"),
    (dict(spot=np.nan), "spot"),
    (dict(spot=np.inf), "spot"),
    (dict(spot=0.0), "spot"),
    (dict(spot=-1.0), "spot"),
    (dict(spot=[100.0, 101.0]), "spot"),
    (dict(risk_free=np.nan), "risk_free"),
    (dict(risk_free=np.inf), "risk_free"),
    (dict(q=np.nan), "q"),
    (dict(options=[{"strike": 0.0, "maturity": 1.0, "option_type": "call"}]), "strike"),
    (dict(options=[{"strike": -5.0, "maturity": 1.0, "option_type": "put"}]), "strike"),
    (dict(options=[{"strike": 100.0, "maturity": 0.0, "option_type": "call"}]), "maturity"),
    (dict(options=[{"strike": 100.0, "maturity": -1.0, "option_type": "call"}]), "maturity"),
    (dict(options=[]), "options"),
    (dict(N=0), "N"),
    (dict(N=2049), "N"),
    (dict(N=12.5), "N"),
    (dict(L=0.0), "L"),
    (dict(L=np.inf), "L"),
])
def test_greeks_refuses_bad_arguments_before_loading_the_library(monkeypatch, change, word):
    import dhcos
    from dhcos import _native

    def no_load(*a, **k):
        raise AssertionError("the native library was reached")

    monkeypatch.setattr(_native, "load", no_load)
    monkeypatch.setattr(_native, "default_context", no_load)
    with pytest.raises(ValueError, match=word):
        dhcos.greeks(**{**_good(), **change})


def test_greeks_dataclass_fields():
    import dataclasses
    import dhcos
    assert [f.name for f in dataclasses.fields(dhcos.Greeks)] == list(G.PLANES)
    from dhcos import _native
    assert _native.GREEKS == G.PLANES
