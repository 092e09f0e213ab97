"""CPU checks of the vol objective's exact gradient, gradient="vega" (DESIGN.md 3.20): the switch's
refusals, none of which loads the library, the defaults, and the restatement
(tests/iv_grad_reference.py) against central differences of its own loss.

The central-difference bar, max |g - g_cd| <= 1e-6 max |g|, is a formula check, not a precision
check: a wrong vega or a missing weight moves the gradient by O(1) of itself.  Parameter sets are
drawn inside tests/test_gpu_batch_grad.py's LO..HI box under its RandomState(4); measured on the
two grids (h = 1e-5 in x, N = 64): 15 options <= 5.4e-9, 70 options <= 1.0e-8 of max |g|, no vega
below 8.5 and no vol below 0.29, so no option is near the clamp."""
import inspect

import numpy as np
import pytest

import iv_grad_reference as V
import param_grad_reference as R
from oracle import dh_oracle as O

MKT = np.full((2, 15), 5.0)
IVS = np.full((2, 15), 0.2)
SPOTS = np.array([100.0, 101.0])
X0S = np.zeros((2, 1, 13))
LO = np.array([0.025, 1.5, 0.025, 0.2, -0.85, 0.02, 0.3, 0.025, 0.1, -0.7, 0.05, -0.08, 0.03])
HI = np.array([0.08, 4.5, 0.065, 0.5, -0.4, 0.07, 1.2, 0.07, 0.35, -0.2, 0.25, -0.01, 0.12])
MARKET = [{"strike": 100.0, "maturity": 1.0, "price": 9.0, "option_type": "call"}]


def _no_native(monkeypatch):
    from dhcos import _native

    def no_load(*a, **k):
        raise AssertionError("the native library was reached")

    monkeypatch.setattr(_native, "load", no_load)
    monkeypatch.setattr(_native, "default_context", no_load)


# ---- the switch ----------------------------------------------------------------------------------

def test_vega_refuses_the_price_objective(monkeypatch):
    import dhcos
    _no_native(monkeypatch)
    with pytest.raises(ValueError, match="objective"):
        dhcos.calibrate_batch(MKT, SPOTS, 0.03, x0s=X0S, gradient="vega")
    with pytest.raises(ValueError, match="objective"):
        dhcos.calibrate_batch(MKT, SPOTS, 0.03, x0s=X0S, gradient="vega", objective="price")
    with pytest.raises(ValueError, match="objective"):
        dhcos.DoubleHestonJumpCalibrator(100.0, 0.05, MARKET, gradient="vega")


def test_vega_refuses_a_series_past_its_table(monkeypatch):
    import dhcos
    _no_native(monkeypatch)
    for N in (1025, 0):
        with pytest.raises(ValueError, match="N"):
            dhcos.calibrate_batch(MKT, SPOTS, 0.03, x0s=X0S, gradient="vega", objective="iv",
                                  market_ivs=IVS, N=N)
        with pytest.raises(ValueError, match="N"):
            dhcos.DoubleHestonJumpCalibrator(100.0, 0.05, MARKET, gradient="vega", objective="iv",
                                             market_ivs=[0.2], N=N)


def test_analytic_still_refuses_the_vol_objective_and_points_to_vega(monkeypatch):
    import dhcos
    _no_native(monkeypatch)
    with pytest.raises(ValueError, match="objective.*vega"):
        dhcos.calibrate_batch(MKT, SPOTS, 0.03, x0s=X0S, gradient="analytic", objective="iv",
                              market_ivs=IVS)
    with pytest.raises(ValueError, match="objective.*vega"):
        dhcos.DoubleHestonJumpCalibrator(100.0, 0.05, MARKET, gradient="analytic", objective="iv")


def test_the_gradient_values_and_defaults():
    import dhcos
    from dhcos import batch
    assert batch.IV_GRADIENTS == ("fd", "vega")
    assert batch.GRADIENTS == ("fd", "analytic")
    for fn in (dhcos.calibrate_batch, dhcos.DoubleHestonJumpCalibrator.__init__):
        params = inspect.signature(fn).parameters
        assert params["gradient"].default == "fd" and params["objective"].default == "price"
    assert batch.check_gradient("vega", "iv", 1024) == "vega"
    assert batch.check_gradient("fd", "iv", 4096) == "fd"
    with pytest.raises(ValueError, match="gradient"):
        batch.check_gradient("exact", "iv", 128)
    cal = dhcos.DoubleHestonJumpCalibrator(100.0, 0.05, MARKET, gradient="vega", objective="iv",
                                           market_ivs=[0.2])
    assert (cal.gradient, cal.objective) == ("vega", "iv")
    with pytest.raises(ValueError, match="driver"):
        cal.calibrate(maxiter=1, multi_start=1, driver="device")


def test_binding_lists_the_new_exports():
    from dhcos import _native
    for name in ("dh_surface_iv_grad_rows_dev", "dh_surface_loss_iv_grad_rows_dev",
                 "dh_surface_loss_iv_grad_rows", "dh_calibrate_lbfgs_batch_iv_grad"):
        assert name in _native.SIGNATURES
    assert (_native.SIGNATURES["dh_calibrate_lbfgs_batch_iv_grad"]
            == _native.SIGNATURES["dh_calibrate_lbfgs_batch_iv"])
    for name in ("iv_grad_rows_dev", "loss_iv_grad_rows", "loss_iv_grad_rows_dev",
                 "calibrate_lbfgs_batch_iv_grad"):
        assert callable(getattr(_native.Surface, name))


# ---- the restatement ---------------------------------------------------------------------------------

def grid_of(name):
    from dhcos.generator import MATURITIES, STRIKES_PCT
    if name == "pct15":
        k, t = np.asarray(STRIKES_PCT, dtype=float), np.asarray(MATURITIES, dtype=float)
    else:
        k, t = np.array([85.0, 90.0, 95.0, 100.0, 105.0, 110.0, 115.0]), np.linspace(0.2, 2.0, 10)
    return np.tile(k, t.size), np.repeat(t, k.size)


def test_vega_is_the_black_scholes_vega():
    """Against the textbook form S sqrt(T) phi(d1) and a central difference of the price."""
    S0, r = 100.0, 0.03
    for K, T, v in [(90.0, 0.5, 0.25), (100.0, 1.0, 0.2), (130.0, 2.0, 0.4), (100.0 * np.exp(0.03), 1.0, 0.3)]:
        d1 = (np.log(S0 / K) + (r + 0.5 * v * v) * T) / (v * np.sqrt(T))
        want = S0 * np.sqrt(T) * np.exp(-0.5 * d1 * d1) / np.sqrt(2 * np.pi)
        got = V.vega(v, S0, K, T, r)
        assert abs(got - want) <= 1e-13 * want
        for call in (True, False):
            cd = (V.bs_price(v + 1e-6, S0, K, T, r, call) - V.bs_price(v - 1e-6, S0, K, T, r, call)) / 2e-6
            assert abs(got - cd) <= 1e-7 * want
    assert not V.vega(0.0, S0, 90.0, 1.0, r) > 0.0 and not V.vega(np.nan, S0, 90.0, 1.0, r) > 0.0
    assert not V.vega(0.0, S0, 100.0, 1.0, 0.0) > 0.0            # at the money: 0 / 0


@pytest.mark.parametrize("grid, n_sets", [("pct15", 3), ("abs70", 2)])
def test_gradient_matches_central_differences_of_the_loss(grid, n_sets):
    K, T = grid_of(grid)
    M, N, S0, r, h = K.size, 64, 100.0, 0.03, 1e-5
    call = np.ones(M, dtype=bool)
    rs = np.random.RandomState(4)
    P = LO + (HI - LO) * rs.rand(n_sets, 13)
    base = LO + (HI - LO) * rs.rand(13)
    prices = np.array([O.price_vec(base, S0, k, t, r, True, N) for k, t in zip(K, T)])
    mkt_iv = V.vols_as_used(prices, S0, K, T, r, call) + rs.uniform(-0.02, 0.02, M)
    w = rs.uniform(0.25, 4.0, M)
    w[1] = 0.0
    mkt_iv[1] = np.nan                                   # anything may stand under a zero weight
    for p in P:
        slack = [p[3] ** 2 - 2 * p[1] * p[2], p[8] ** 2 - 2 * p[6] * p[7]]
        assert min(abs(s) for s in slack) > 1e-3         # off the Feller kink
        x = O.from_params(p)
        f, g, iv = V.loss_grad(x, K, T, call, mkt_iv, w, S0, r, N)
        assert np.all(iv > 0.1) and f == pytest.approx(V.loss(x, K, T, call, mkt_iv, w, S0, r, N),
                                                       rel=1e-12)
        cd = np.empty(13)
        for i in range(13):
            e = np.zeros(13)
            e[i] = h
            cd[i] = (V.loss(x + e, K, T, call, mkt_iv, w, S0, r, N)
                     - V.loss(x - e, K, T, call, mkt_iv, w, S0, r, N)) / (2 * h)
        worst = np.max(np.abs(g - cd)) / np.max(np.abs(g))
        print(f"{grid}: max |g - g_cd| / max |g| = {worst:.2e}; min vega "
              f"{np.min(V.vega(iv, S0, K, T, r)):.2f}, min vol {iv.min():.3f}")
        assert worst <= 1e-6


def test_a_clamped_option_adds_its_residual_and_no_gradient():
    K, T = grid_of("pct15")
    S0, r, N = 100.0, 0.0, 64
    call = np.ones(15, dtype=bool)
    rs = np.random.RandomState(7)
    p = LO + (HI - LO) * rs.rand(13)
    planes = V.planes_of(p, S0, K, T, r, call, N)
    iv = V.vols_as_used(planes[0], S0, K, T, r, call)
    mkt_iv = iv + 0.01
    w = np.full(15, 2.0)
    f, g, sse, bad = V.reduce_planes(planes, p, iv, mkt_iv, w, S0, K, T, r)
    c = int(np.argmin(K))                                # the deepest in-the-money call
    crafted = planes.copy()
    crafted[0, c] = np.nextafter(S0 - K[c], 0.0)         # one ulp below its lower bound (r = 0)
    iv2 = V.vols_as_used(crafted[0], S0, K, T, r, call)
    assert iv2[c] == 0.0 and np.array_equal(np.delete(iv2, c), np.delete(iv, c))
    f2, g2, sse2, bad2 = V.reduce_planes(crafted, p, iv2, mkt_iv, w, S0, K, T, r)
    assert bad == bad2 == 0
    # its residual: w (0 - mkt)^2 in place of w (0.01)^2
    assert sse2 - sse == pytest.approx(w[c] * (mkt_iv[c] ** 2 - 0.01 ** 2), rel=1e-9)
    # no gradient: the other fourteen options' alone
    keep = np.ones(15, dtype=bool)
    keep[c] = False
    w0 = w.copy()
    w0[c] = 0.0
    _, g_rest, _, _ = V.reduce_planes(planes, p, iv, mkt_iv, w0, S0, K, T, r)
    assert np.allclose(g2 - R.feller_grad_x(p), (g_rest - R.feller_grad_x(p)) * w0.sum() / w.sum(),
                       rtol=1e-12, atol=0.0)
    assert np.any(g2 != g)
    # a bad price at a positive weight: the invalid set
    crafted[0, 3] = np.nan
    iv3 = V.vols_as_used(crafted[0], S0, K, T, r, call)
    f3, g3, _, bad3 = V.reduce_planes(crafted, p, iv3, mkt_iv, w, S0, K, T, r)
    assert (f3, bad3) == (1e10, 1) and not g3.any()
