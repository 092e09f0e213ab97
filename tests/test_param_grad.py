"""CPU checks of the analytic parameter sensitivities: the NumPy restatement
(tests/param_grad_reference.py) against the oracle's price, the Greeks restatement's vegas, the
50-digit truth fixture (tests/golden/param_grad_truth.json) and central differences of the oracle's
loss; and the refusals of dhcos.parameter_sensitivities and of the calibrator's gradient switch,
none of which loads the library."""
import dataclasses
import json
import os

import numpy as np
import pytest

import greeks_reference as G
import param_grad_reference as R
from conftest import GOLDEN
from oracle import dh_oracle as O

S0, RATE = 100.0, 0.03
PRM = [0.04, 2.0, 0.04, 0.3, -0.5, 0.04, 1.5, 0.04, 0.2, -0.3, 0.5, -0.05, 0.10]
OPTS = [(k, t, c) for t in (0.1, 1.0, 2.0) for k in (80.0, 100.0, 120.0) for c in (True, False)]


@pytest.fixture(scope="module")
def truth():
    with open(os.path.join(GOLDEN, "param_grad_truth.json")) as fh:
        return json.load(fh)


# ---- the restatement against what it restates --------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 128, 256])
def test_price_plane_is_price_vec_and_v0_planes_are_the_greeks_vegas_bit_for_bit(N):
    for K, T, call in OPTS + [(5.0, 0.1, True), (3000.0, 0.1, False)]:      # two clamped ones
        s = R.sens_vec(PRM, S0, K, T, RATE, call, N)
        g = G.greeks_vec(PRM, S0, K, T, RATE, call, N)
        assert s[0].tobytes() == np.float64(O.price_vec(PRM, S0, K, T, RATE, call, N)).tobytes()
        assert s[1].tobytes() == np.float64(g["vega1"]).tobytes()
        assert s[6].tobytes() == np.float64(g["vega2"]).tobytes()


def test_planes_are_in_the_parameter_order():
    assert R.PLANES == ("price",) + tuple(O.PARAM_NAMES) and len(R.PLANES) == 14


# ---- the restatement against 50-digit truth ----------------------------------------------------
# Bars: 10x the restatement's worst error per plane on the machine that generated the fixture, in
# units of max |plane| over the fixture (the fixture's "restatement_worst"; DESIGN.md 3.18 lists
# them).  The factor covers libm differences between hosts.  None comes out above 1e-8.
def test_restatement_matches_the_truth_fixture(truth):
    cases = truth["cases"]
    assert truth["planes"] == list(R.PLANES) and truth["N"] == 128
    assert len(cases) == 8 * 3 * 3 * 2
    assert any(abs(c["prm"][12] - 1e-3) < 1e-12 for c in cases)              # sigma_j small
    assert any(abs(c["prm"][4]) >= 0.9 and abs(c["prm"][9]) >= 0.9 for c in cases)
    want = np.array([c["truth"] for c in cases])
    got = np.array([R.sens_vec(c["prm"], c["S0"], c["K"], c["T"], c["r"], c["is_call"], 128,
                               ab=(c["a"], c["b"])) for c in cases])
    # the stored range is the oracle's own: the default range gives the same bits
    free = np.array([R.sens_vec(c["prm"], c["S0"], c["K"], c["T"], c["r"], c["is_call"], 128)
                     for c in cases[::7]])
    assert free.tobytes() == got[::7].tobytes()
    scale = np.max(np.abs(want), axis=0)
    assert np.allclose(scale, truth["plane_scale"], rtol=1e-12, atol=0)
    worst = np.max(np.abs(got - want), axis=0) / scale
    bars = 10.0 * np.array(truth["restatement_worst"])
    for name, w, b in zip(R.PLANES, worst, bars):
        print(f"{name:9s} worst {w:.3e} of max |plane|, bar {b:.3e}")
    assert np.all(bars <= 1e-8), dict(zip(R.PLANES, bars))
    assert np.all(bars > 0)
    assert np.all(worst <= bars), [R.PLANES[i] for i in np.flatnonzero(worst > bars)]


# ---- the restated loss gradient against central differences of the oracle's loss ---------------
def _central(x, market, h):
    g = np.empty(13)
    for i in range(13):
        e = np.zeros(13)
        e[i] = h
        g[i] = (O.loss(x + e, market, 100.0, 0.05) - O.loss(x - e, market, 100.0, 0.05)) / (2 * h)
    return g


def test_restated_loss_gradient_matches_central_differences(calib_golden):
    """At guesses_seed0[1]: Feller slack > 0 on one factor, < 0 on the other (asserted), so the
    penalty's derivative is live and no kink is near.  O.loss moves the range with the parameters,
    the restatement holds it: the issue measured that difference at 3e-9 to 4e-7 relative on the
    price derivatives, inside the quotient's error.  Bound per component: the central quotient's
    truncation error C h^2, estimated from the h / 2 quotient (q(h) - q(h/2) = 3/4 C h^2, so
    err(h) = 4/3 |q(h) - q(h/2)|), doubled for the next order; plus its rounding error, two losses
    each good to ~4 eps |f| over 2 h; plus 1e-6 |g| for the range's dependence on the parameters
    (the project's parity rule)."""
    market = calib_golden["test_market"]
    x = np.array(calib_golden["guesses_seed0"][1])
    p = O.to_params(x)
    slack = [p[3] ** 2 - 2 * p[1] * p[2], p[8] ** 2 - 2 * p[6] * p[7]]
    assert (slack[0] > 1e-3) != (slack[1] > 1e-3) and min(slack) < -1e-3, slack
    f, g = R.loss_grad(x, market, 100.0, 0.05)
    assert f == O.loss(x, market, 100.0, 0.05)
    assert np.count_nonzero(R.feller_grad_x(p)) == 3
    h = 1e-6
    q1, q2 = _central(x, market, h), _central(x, market, h / 2)
    bound = 2 * (4 / 3) * np.abs(q1 - q2) + 4 * np.finfo(float).eps * abs(f) / h + 1e-6 * np.abs(g)
    err = np.abs(g - q1)
    for i, n in enumerate(O.PARAM_NAMES):
        print(f"{n:9s} g {g[i]: .6e} central {q1[i]: .6e} err {err[i]:.2e} bound {bound[i]:.2e}")
    assert np.all(err <= bound), [O.PARAM_NAMES[i] for i in np.flatnonzero(err > bound)]


def test_restated_loss_gradient_of_an_invalid_set_is_zero(calib_golden):
    f, g = R.loss_grad(np.full(13, 5.0), calib_golden["test_market"], 100.0, 0.05)
    assert f == O.INVALID_LOSS and not g.any()


def test_feller_derivative_is_zero_on_the_kink(calib_golden):
    """The literature start sits on factor 2's kink (sigma^2 = 2 kappa theta to rounding, reference
    quirk Q12): whichever side rounding puts it, the forward quotient sees the penalty's slope
    (fd_guess0's g[8] = 80) and the analytic derivative is the one-sided rule of the contract."""
    x = np.array(calib_golden["guesses_seed0"][0])
    p = O.to_params(x)
    slack = p[8] ** 2 - 2 * p[6] * p[7]
    assert abs(slack) < 1e-15
    assert R.feller_grad_x(p)[8] == (2000.0 * p[8] ** 2 if slack > 0 else 0.0)


# ---- refusals, before the library loads ---------------------------------------------------------
def _good():
    return dict(parameters=PRM, spot=S0, risk_free=RATE,
                options=[{"strike": 100.0, "maturity": 1.0, "option_type": "call"}])


def _no_native(monkeypatch):
    from dhcos import _native

    def no_load(*a, **k):
        raise AssertionError("the native library was reached")

    monkeypatch.setattr(_native, "load", no_load)
    monkeypatch.setattr(_native, "default_context", no_load)


@pytest.mark.parametrize("change, word", [
    (dict(parameters=PRM[:12]), "parameters"),
    (dict(parameters=np.zeros((2, 3, 13))), "parameters"),
    (dict(parameters={"v1_0": 0.04}), "parameters"),
    (dict(spot=np.nan), "spot"),
    (dict(spot=0.0), "spot"),
    (dict(spot=[100.0, 101.0]), "spot"),
    (dict(risk_free=np.inf), "risk_free"),
    (dict(q=np.nan), "q"),
    (dict(options=[{"strike": 0.0, "maturity": 1.0, "option_type": "call"}]), "strike"),
    (dict(options=[{"strike": 100.0, "maturity": -1.0, "option_type": "call"}]), "maturity"),
    (dict(options=[]), "options"),
    (dict(N=0), "N"),
    (dict(N=1025), "N"),
    (dict(N=2048), "N"),
    (dict(N=12.5), "N"),
    (dict(L=0.0), "L"),
    (dict(L=np.inf), "L"),
])
def test_parameter_sensitivities_refuses_bad_arguments_before_loading_the_library(
        monkeypatch, change, word):
    import dhcos
    _no_native(monkeypatch)
    with pytest.raises(ValueError, match=word):
        dhcos.parameter_sensitivities(**{**_good(), **change})


def test_dataclass_fields_and_binding_constants():
    import dhcos
    from dhcos import _native
    assert [f.name for f in dataclasses.fields(dhcos.ParameterSensitivities)] == list(R.PLANES)
    assert _native.PARAM_SENS == R.PLANES
    assert _native.PARAM_GRAD_MAX_N == 1024
    assert tuple(dhcos.calibrator.PARAM_NAMES) == R.PLANES[1:]


def test_calibrator_refuses_what_the_analytic_gradient_does_not_cover(monkeypatch, calib_golden):
    import dhcos
    from dhcos import DoubleHestonJumpCalibrator as Cal
    _no_native(monkeypatch)
    market = calib_golden["test_market"]
    with pytest.raises(ValueError, match="gradient"):
        Cal(100.0, 0.05, market, gradient="exact")
    with pytest.raises(ValueError, match="objective"):
        Cal(100.0, 0.05, market, objective="iv", gradient="analytic")
    with pytest.raises(ValueError, match="N"):
        Cal(100.0, 0.05, market, N=2048, gradient="analytic")

    class OwnLoss(Cal):
        def compute_loss(self, x):
            return 0.0

    class OwnBatch(Cal):
        def loss_batch(self, X, track=True):
            return np.zeros(len(X))

    for cls in (OwnLoss, OwnBatch):
        with pytest.raises(ValueError, match="subclass"):
            cls(100.0, 0.05, market, gradient="analytic")
        assert cls(100.0, 0.05, market).gradient == "fd"
    cal = Cal(100.0, 0.05, market, gradient="analytic")
    assert cal.gradient == "analytic" and Cal(100.0, 0.05, market).gradient == "fd"
    with pytest.raises(ValueError, match="driver"):
        cal.calibrate(maxiter=1, multi_start=1, driver="device")
    with pytest.raises(ValueError, match="driver"):        # the sharded path calls it directly
        dhcos.calibrator.run_starts_device(cal, [np.zeros(13)], 1)
    assert dhcos.calibrator._native_surface(cal, 1) is None      # the FD request loop is not used
