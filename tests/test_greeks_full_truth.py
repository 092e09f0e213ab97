"""CPU checks of the full Greeks against a 50+-digit truth: the NumPy restatement
(tests/greeks_full_reference.py) on every case and plane of tests/golden/greeks_full_truth.json
(written by tests/golden/make_greeks_full_truth.py: the COS series in mpmath, dprice_dT, rho and
dual_gamma as term-by-term central differences in T, r and K at fixed [a, b], no derivative
formula), three deliberately wrong restatements, two identities on the truth, Dupire's quotient in
the Black-Scholes limit, and the Python entry points' refusals.

The unit of every bar is the fixture's `unit`, the plane's absolute term sum, as in
tests/test_greeks_truth.py.  Bar of the restatement: 10x the error the generator recorded for that
plane and N (another libm may round apart), and at least 10 * 2^-52; the generator's own cap on
what it records is 64 * 2^-52.
Measured by the generator, worst over N: dprice_dT 6.8e-15 (31 * 2^-52, N = 256), rho 2.6e-15,
dual_gamma 1.1e-15.
"""
import functools
import json
import os

import numpy as np
import pytest

import greeks_full_reference as GF
import greeks_reference as G

EPS = 2.0 ** -52
CAP = 64 * EPS
DEMO = [0.04, 2.0, 0.04, 0.3, -0.5, 0.04, 1.5, 0.04, 0.2, -0.3, 0.5, -0.05, 0.10]


@functools.lru_cache(maxsize=None)
def fixture():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                           "greeks_full_truth.json")) as fh:
        return json.load(fh)


def case_args(fix, c):
    return fix["sets"][c["set"]], c["S0"], c["K"], c["T"], c["r"], c["is_call"], c["N"], c["q"]


@functools.lru_cache(maxsize=None)
def restatement(wrong=None):
    """[cases, 3]: full_vec's NEW_PLANES on every case of the fixture, computed once."""
    fix = fixture()
    out = np.empty((len(fix["cases"]), len(GF.NEW_PLANES)))
    for i, c in enumerate(fix["cases"]):
        g = GF.full_vec(*case_args(fix, c), wrong=wrong)
        out[i] = [g[name] for name in GF.NEW_PLANES]
    return out


def relative_errors(got):
    fix = fixture()
    truth = np.array([c["truth"] for c in fix["cases"]])
    unit = np.array([c["unit"] for c in fix["cases"]])
    err = np.abs(got - truth)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(unit > 0, err / unit, np.where(err == 0, 0.0, np.inf))


def test_fixture_shape():
    fix = fixture()
    cases = fix["cases"]
    assert tuple(fix["planes"]) == GF.NEW_PLANES and len(fix["sets"]) == 4
    count = {g: sum(c["group"] == g for c in cases) for g in "ABCD"}
    assert count == {"A": 48, "B": 16, "C": 12, "D": 24}
    assert {c["N"] for c in cases if c["group"] in "AB"} == {128}
    assert {c["N"] for c in cases if c["group"] == "C"} == {256}
    assert {c["N"] for c in cases if c["group"] == "D"} == {1, 2, 17, 772, 773, 2048}
    assert {(c["S0"], c["r"], c["q"]) for c in cases if c["group"] == "B"} == \
        {(80.0, 0.01, 0.02), (125.0, 0.05, 0.0)}
    flags = [c["clamp"] for c in cases if c["group"] == "C"]
    assert any(flags) and not all(flags)
    assert not any(c["clamp"] for c in cases if c["group"] != "C")
    for c in cases:
        assert len(c["truth"]) == len(c["unit"]) == 3 and len(c["extra"]) == 4
        assert all(abs(t) <= u for t, u in zip(c["truth"], c["unit"]))
        assert c["clamp"] == G.clamp_active(fix["sets"][c["set"]], c["S0"], c["K"], c["T"], c["r"])
    for name in GF.NEW_PLANES:         # the generator's own condition
        assert set(fix["restatement_worst"][name]) == {str(c["N"]) for c in cases}
        assert max(fix["restatement_worst"][name].values()) <= CAP


def test_restatement_stays_within_ten_times_its_recorded_error():
    fix = fixture()
    rel = relative_errors(restatement())
    ns = np.array([c["N"] for c in fix["cases"]])
    for i, name in enumerate(GF.NEW_PLANES):
        print(f"{name:10s} worst |restatement - truth| / unit: " + "  ".join(
            f"N={n}: {rel[ns == n, i].max():.2e}" for n in sorted(set(ns))))
        for n in sorted(set(ns)):
            bar = max(10 * fix["restatement_worst"][name][str(n)], 10 * EPS)
            assert rel[ns == n, i].max() <= bar, (name, n, rel[ns == n, i].max(), bar)


@pytest.mark.parametrize("wrong, plane", list(zip(GF.WRONG, GF.NEW_PLANES)))
def test_a_wrong_restatement_is_refused(wrong, plane):
    """-r price dropped from dprice_dT, -T price dropped from rho, S0^2 / K^2 taken the wrong way
    in dual_gamma (K for 1 / K): each leaves the other planes alone and puts its own past the
    generator's cap on some case -- the fixture would not have been written."""
    rel = relative_errors(restatement(wrong))
    i = GF.NEW_PLANES.index(plane)
    assert rel[:, i].max() > CAP, (wrong, rel[:, i].max())
    others = [j for j in range(3) if j != i]
    assert np.array_equal(restatement(wrong)[:, others], restatement()[:, others])


def test_identities_hold_on_the_truth():
    """K^2 dual_gamma = S0^2 gamma and d price / dq = -(rho + T price) on the 80-digit truth, where
    gamma is a second difference in S0 and d/dq a difference in q: neither was made from the plane
    it is compared with.  To 1e-13 of the planes' units (the truth is stored in doubles)."""
    fix = fixture()
    ix = {n: i for i, n in enumerate(fix["extra"])}
    for c in fix["cases"]:
        dT, rho, dgam = c["truth"]
        price, gamma, dq = (c["extra"][ix[n]] for n in ("price", "gamma", "dprice_dq"))
        K, S0, T = c["K"], c["S0"], c["T"]
        assert abs(K * K * dgam - S0 * S0 * gamma) <= 1e-13 * K * K * c["unit"][2], c
        assert abs(dq + (rho + T * price)) <= 1e-13 * (c["unit"][1] + abs(T * price)), c


BS_SET = [0.04, 2.0, 0.04, 1e-3, 0.0, 0.04, 1.5, 0.04, 1e-3, 0.0, 0.0, -0.05, 0.10]
BS_MARKET = (100.0, 0.03, 0.01)        # S0, r, q
BS_GRID = [(T, 100.0 * m) for T in (0.5, 1.0) for m in (0.9, 1.0, 1.1)]


def bs_limit_local_var(T):
    v01, k1, t1, _, _, v02, k2, t2 = BS_SET[:8]
    return (t1 + (v01 - t1) * np.exp(-k1 * T)) + (t2 + (v02 - t2) * np.exp(-k2 * T))


@pytest.mark.parametrize("is_call", [True, False])
def test_local_var_in_the_black_scholes_limit(is_call):
    """sigma_1 = sigma_2 = 1e-3, rho_j = 0, lambda = 0 (the demo set otherwise), N = 512: the
    variances are deterministic to O(sigma^2), the leverage term vanishes at rho = 0, and Dupire's
    local variance is sum_j [theta_j + (v0_j - theta_j) e^{-kappa_j T}], to 1e-4 relative -- a
    condition: a wrong sign or a missing term in dprice_dT, dual_delta, dual_gamma or the quotient
    is an error of order one.  q = 0.01 so that both rate terms of the quotient take part.  All
    six (T, K) meet the bar; none was dropped."""
    S0, r, q = BS_MARKET
    for T, K in BS_GRID:
        got = GF.full_vec(BS_SET, S0, K, T, r, is_call, 512, q)["local_var"]
        want = bs_limit_local_var(T)
        print(f"T={T} K={K}: local_var {got:.10f}, closed form {want:.10f}, "
              f"relative {abs(got / want - 1):.2e}")
        assert abs(got - want) <= 1e-4 * want, (T, K, got, want)


def test_local_var_quotient_rule():
    f = GF.local_var_from_planes
    assert f(1.0, 2.0, -0.5, 0.01, 100.0, 0.03, 0.01) == \
        ((1.0 + ((0.03 - 0.01) * 100.0) * -0.5) + 0.01 * 2.0) / ((0.5 * (100.0 * 100.0)) * 0.01)
    assert np.isnan(f(1.0, 2.0, -0.5, 0.0, 100.0, 0.03, 0.0))          # denominator not > 0
    assert np.isnan(f(1.0, 2.0, -0.5, -1e-9, 100.0, 0.03, 0.0))
    assert np.isnan(f(np.inf, 2.0, -0.5, 0.01, 100.0, 0.03, 0.0))      # a plane not finite
    assert f(-1.0, 0.0, 0.0, 0.01, 100.0, 0.03, 0.0) < 0.0             # negative: not clipped


# ---- the Python entry points refuse before the library is loaded ---------------------------------
OPTS = [{"strike": 100.0, "maturity": 1.0, "option_type": "call"}]


@pytest.fixture
def no_library(monkeypatch):
    from dhcos import _native

    def boom(*a, **k):
        raise AssertionError("the native library was reached")
    monkeypatch.setattr(_native, "load", boom)
    monkeypatch.setattr(_native, "default_context", boom)


@pytest.mark.parametrize("kw", [dict(N=0), dict(N=2049), dict(N=12.5), dict(L=0.0),
                                dict(L=float("nan")), dict(L=-1.0)])
def test_greeks_full_refuses_bad_N_and_L(no_library, kw):
    import dhcos
    with pytest.raises(ValueError):
        dhcos.greeks_full(DEMO, 100.0, 0.03, OPTS, **kw)
    with pytest.raises(ValueError):
        dhcos.local_vol(DEMO, 100.0, 0.03, [90.0, 100.0], [0.5, 1.0], **kw)
    with pytest.raises(ValueError):
        dhcos.DoubleHeston.greeks_full_batch([DEMO], 100.0, [100.0], [1.0], 0.03, **kw)


def test_greeks_full_refuses_bad_shapes_and_options(no_library):
    import dhcos
    for bad in (DEMO[:12], [[DEMO, DEMO]], np.zeros((0, 13))):
        with pytest.raises(ValueError):
            dhcos.greeks_full(bad, 100.0, 0.03, OPTS)
    with pytest.raises(ValueError):
        dhcos.greeks_full(DEMO, -1.0, 0.03, OPTS)
    with pytest.raises(ValueError):
        dhcos.greeks_full([DEMO, DEMO], [100.0, 100.0, 100.0], 0.03, OPTS)
    with pytest.raises(ValueError):
        dhcos.greeks_full(DEMO, 100.0, 0.03, [])
    for k, t in ((0.0, 1.0), (-5.0, 1.0), (float("inf"), 1.0), (100.0, 0.0), (100.0, float("nan"))):
        with pytest.raises(ValueError):
            dhcos.greeks_full(DEMO, 100.0, 0.03,
                              [{"strike": k, "maturity": t, "option_type": "put"}])


def test_local_vol_refuses_bad_strikes_and_maturities(no_library):
    import dhcos
    good = [90.0, 100.0]
    for strikes, mats in (([], good), (good, []), ([[90.0, 100.0]], good), (good, [[0.5]]),
                          ([0.0, 100.0], good), ([-1.0], good), (good, [0.0]), (good, [-0.5]),
                          ([float("nan")], good), (good, [float("inf")]), (100.0, good)):
        with pytest.raises(ValueError):
            dhcos.local_vol(DEMO, 100.0, 0.03, strikes, mats)
    with pytest.raises(ValueError):
        dhcos.local_vol(DEMO[:5], 100.0, 0.03, good, good)


def test_full_greeks_properties():
    from dhcos import FullGreeks
    z = np.zeros(2)
    g = FullGreeks(np.array([10.0, 5.0]), z, z, z, z, z, np.array([3.0, -1.0]),
                   np.array([40.0, -20.0]), np.array([0.01, 0.02]), np.array([0.09, -0.01]),
                   np.array([2.0, 0.5]), np.float64(0.03))
    assert np.array_equal(g.theta, [-3.0, 1.0])
    assert np.array_equal(g.epsilon, [-(40.0 + 2.0 * 10.0), -(-20.0 + 0.5 * 5.0)])
    assert np.array_equal(g.density, np.exp(0.03 * np.array([2.0, 0.5])) * [0.01, 0.02])
    assert g.local_vol[0] == np.sqrt(0.09) and np.isnan(g.local_vol[1])
