"""CPU checks of the path pricer's variance reduction: the exact mirror of a
uniform, the NumPy restatement's estimator (tests/mc_vr_reference.py) on hand-made sums, the new
ValueErrors of dhcos.monte_carlo (raised before the native library is loaded), and the new exports
in the header, the binding and the library."""
import math
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import mc_reference as R
import mc_vr_reference as V
from test_native_abi import HEADER, header_code, header_functions

SPOT, RATE = 100.0, 0.03
NEW = ("dh_mc_price_vr", "dh_mc_price_vr_dev", "dh_mc_paths_vr")


@pytest.mark.parametrize("k", [0, 1, (1 << 51) - 1, 1 << 51, (1 << 52) - 2, (1 << 52) - 1])
def test_the_mirror_of_a_uniform_is_exact(k):
    """U = (2 k + 1) 2^-53 for a 52-bit k: U + (1 - U) == 1 with no rounding, and 1 - U is the
    uniform of the complementary k."""
    hi, lo = np.uint64((k >> 26) << 6), np.uint64((k & ((1 << 26) - 1)) << 6)
    u = float(R.uniform(hi, lo))
    assert Fraction(u) == Fraction(2 * k + 1, 1 << 53)
    m = float(V.mirror_uniform(u))
    assert Fraction(u) + Fraction(m) == 1 and u + m == 1.0
    odd = Fraction(m) * (1 << 53)
    assert odd.denominator == 1 and odd.numerator % 2 == 1 and 0 < odd.numerator < 1 << 53
    assert odd.numerator == 2 * ((1 << 52) - 1 - k) + 1
    assert 0.0 < m < 1.0


def test_mirrored_draws_negate_the_normals():
    a = V.draws(7, np.arange(64), 3)
    b = V.draws(7, np.arange(64), 3, mirror=True)
    for k in (0, 3, 6):
        assert np.all(a[k] + b[k] == 1.0)
    for k in (1, 2, 4, 5, 7):
        assert np.array_equal(a[k], -b[k])
    assert all(np.array_equal(x, y) for x, y in zip(a, R.draws(7, np.arange(64), 3)))


def _sums(y, c):
    return V.five_sums(np.asarray(y, dtype=np.float64), np.asarray(c, dtype=np.float64))


def test_estimator_on_hand_made_sums():
    # y = (1, 2, 3, 6), c = (1, 1, 2, 4): Cyy = 14, Ccc = 6, Cyc = 9, beta = 3/2
    y, c = [1.0, 2.0, 3.0, 6.0], [1.0, 1.0, 2.0, 4.0]
    s = _sums(y, c)
    assert s == (12.0, 50.0, 8.0, 22.0, 33.0)
    e = V.estimator(s, 4, 0.5, 0.75)
    assert e["beta"] == 1.5 and e["base_price"] == 1.5
    assert e["base_stderr"] == 0.5 * math.sqrt(14.0 / 12.0)
    assert e["price"] == 1.5 - 1.5 * (0.5 * 8.0 / 4.0 - 0.75)
    assert e["stderr"] == 0.5 * math.sqrt((14.0 - 1.5 * 9.0) / 12.0)
    x = V.estimator(s, 4, 0.5, 0.75, exact=True)
    for k in e:
        assert abs(e[k] - x[k]) <= 4 * 2.0 ** -53 * abs(x[k]), k
    # without the control flag: the plain estimator
    p = V.estimator(s, 4, 0.5, float("nan"), control=False)
    assert p["beta"] == 0.0 and p["price"] == p["base_price"] == 1.5
    assert p["stderr"] == p["base_stderr"] == e["base_stderr"]


def test_a_constant_control_gives_beta_zero():
    e = V.estimator(_sums([1.0, 2.0, 4.0], [3.0, 3.0, 3.0]), 3, 1.0, 2.0)
    assert e["beta"] == 0.0 and e["price"] == e["base_price"] and e["stderr"] == e["base_stderr"]
    z = V.estimator(_sums([1.0, 2.0, 4.0], [0.0, 0.0, 0.0]), 3, 1.0, 2.0)
    assert z["beta"] == 0.0 and z["price"] == z["base_price"]


def test_a_control_that_is_the_payoff_gives_beta_one_and_no_error():
    y = [0.0, 1.25, 7.5, 0.0, 3.0]
    e = V.estimator(_sums(y, y), 5, 0.97, 2.2)
    assert e["beta"] == 1.0 and e["stderr"] == 0.0
    assert abs(e["price"] - 2.2) <= 4 * 2.0 ** -53 * max(abs(e["base_price"]), 2.2)


def test_controls_by_kind():
    eu = {"strike": 100.0, "maturity": 0.5, "option_type": "call"}
    assert not V.has_twin(eu) and not V.has_twin(dict(eu, kind="asian", strike=0.0))
    for kind in ("asian", "up_and_out", "down_and_out"):
        assert V.has_twin(dict(eu, kind=kind, barrier=120.0))
    st = np.array([[110.0, 0.04, 0.04, 130.0, 95.0, 400.0]])
    y, c = V.sample_and_control(dict(eu, kind="up_and_out", barrier=120.0), 4, st)
    assert y[0] == 0.0 and c[0] == 10.0
    y, c = V.sample_and_control(eu, 4, st)
    assert y[0] == 10.0 and c[0] == 110.0
    mirror = np.array([[99.0, 0.04, 0.04, 130.0, 95.0, 440.0]])
    y, c = V.sample_and_control(dict(eu, kind="asian"), 4, st, mirror)
    assert y[0] == 0.5 * (0.0 + 10.0) and c[0] == 0.5 * (10.0 + 0.0)


# ---- the new refusals of dhcos.monte_carlo, without the native library ------------------------------
@pytest.fixture
def no_native(monkeypatch):
    from dhcos import _native

    def refuse(*a, **k):
        raise AssertionError("the native library was reached")
    monkeypatch.setattr(_native, "load", refuse)
    monkeypatch.setattr(_native, "default_context", refuse)


OPT = [{"strike": 100.0, "maturity": 0.5, "option_type": "call", "kind": "asian"}]


@pytest.mark.parametrize("kw", [dict(n_paths=1025, antithetic=True), dict(n_paths=2, antithetic=True),
                                dict(n_paths=3, antithetic=True, control_variate=True),
                                dict(n_paths=1, control_variate=True),
                                dict(n_paths=1024, control_variate=True, steps_per_year=0)])
def test_monte_carlo_refuses_before_the_native_library(kw, no_native):
    import dhcos
    with pytest.raises(ValueError):
        dhcos.monte_carlo(R.README_PARAMS, SPOT, RATE, OPT, **kw)
    dh = dhcos.DoubleHeston(SPOT, 105.0, 0.5, RATE, *R.README_PARAMS, option_type="call")
    if "steps_per_year" not in kw:
        with pytest.raises(ValueError):
            dh.monte_carlo(**kw)


@pytest.mark.parametrize("kw", [dict(n_paths=4, antithetic=True), dict(n_paths=3, control_variate=True),
                                dict(n_paths=1024, antithetic=True, control_variate=True)])
def test_valid_arguments_reach_the_native_library(kw, no_native):
    import dhcos
    with pytest.raises(AssertionError, match="native library was reached"):
        dhcos.monte_carlo(R.README_PARAMS, SPOT, RATE, OPT, **kw)
    from dhcos.montecarlo import simulate_paths
    with pytest.raises(AssertionError, match="native library was reached"):
        simulate_paths(R.README_PARAMS, SPOT, RATE, [1, 2], n_paths=4, mirror=True)
    with pytest.raises(ValueError):
        simulate_paths(R.README_PARAMS, SPOT, RATE, [2, 2], n_paths=4, mirror=True)


def test_result_carries_the_new_fields_and_the_plain_one_does_not():
    from dhcos.montecarlo import MonteCarloResult, VarianceReducedResult
    one = np.array([1.0])
    plain = MonteCarloResult(one, one, 8, 64, 0)
    assert not hasattr(plain, "beta") and [f for f in plain.__dataclass_fields__] == [
        "price", "stderr", "n_paths", "steps_per_year", "seed"]
    r = VarianceReducedResult(one, 0.5 * one, 8, 64, 0, one, 2.0 * one, one, one, True, True)
    assert isinstance(r, MonteCarloResult) and r.variance_ratio[0] == 16.0
    assert r.confidence()[0][0] == 1.0 - 1.96 * 0.5 and r.antithetic and r.control_variate


# ---- the exports ------------------------------------------------------------------------------------
def test_header_and_binding_carry_the_new_exports():
    from dhcos import _native
    assert set(NEW) <= set(header_functions()) and set(NEW) <= set(_native.SIGNATURES)
    code = header_code()
    flags = re.search(r"enum dh_mc_vr_flag \{([^{}]*)\}", code).group(1)
    assert dict(re.findall(r"(DH_MC_VR_[A-Z]+) = (\d+)", flags)) == {
        "DH_MC_VR_ANTITHETIC": str(_native.MC_VR_ANTITHETIC),
        "DH_MC_VR_CONTROL": str(_native.MC_VR_CONTROL)}
    assert (_native.MC_VR_ANTITHETIC, _native.MC_VR_CONTROL) == (V.ANTITHETIC, V.CONTROL) == (1, 2)
    assert int(re.search(r"DH_MC_VR_COS_N = (\d+)", code).group(1)) == _native.MC_VR_COS_N == V.COS_N
    assert float(re.search(r"#define DH_MC_VR_COS_L \(([\d.]+)\)", open(HEADER).read()).group(1)) \
        == _native.MC_VR_COS_L == V.COS_L
    # dh_mc_price_vr is dh_mc_price with flags and four more outputs; _dev adds the stream
    sig = _native.SIGNATURES
    assert len(sig["dh_mc_price_vr"][1]) == len(sig["dh_mc_price"][1]) + 5
    assert len(sig["dh_mc_price_vr_dev"][1]) == len(sig["dh_mc_price_vr"][1]) + 1
    assert len(sig["dh_mc_paths_vr"][1]) == len(sig["dh_mc_paths"][1]) + 1


def test_library_exports_the_new_symbols():
    from dhcos import _native
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    assert set(NEW) <= set(re.findall(r"\bT (dh_[a-z_]+)\b", out))
