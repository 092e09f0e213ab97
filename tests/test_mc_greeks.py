"""CPU checks of the coupled-path Monte Carlo Greeks: the NumPy restatement
(tests/mc_greeks_reference.py) against central differences, at the estimator's own steps, of the
oracle's COS prices; its spot bumps against walks at the bumped spot; and every ValueError of
dhcos.monte_carlo_greeks, raised before the native library is asked for a device."""
import numpy as np
import pytest

import mc_greeks_reference as G
import mc_reference as R
from oracle import dh_oracle as O


def _cos(options, rate):
    K = np.array([o["strike"] for o in options])
    T = np.array([o["maturity"] for o in options])
    call = np.array([o["option_type"] == "call" for o in options])
    return lambda p, s: O.price_many(p, s, K, T, rate, call, 512)


def test_restatement_matches_cos_central_differences():
    """The statistical case (2^16 paths at 32 steps per year, three strikes at each of three
    maturities up to half a year, puts and calls): delta, gamma and both vegas of every option
    within 4 of their own standard errors of the central differences, at the same eps and b, of the
    oracle's COS prices (q = 0, N = 512); the price likewise.  No allowance for time-step bias."""
    value, err = G.greeks(G.STAT_PARAMS, G.STAT_SPOT, G.STAT_RATE, G.STAT_OPTIONS, G.STAT_PATHS,
                          G.STAT_SPY, G.STAT_SEED, G.STAT_SPOT_BUMP, G.STAT_V0_BUMP)
    cos = _cos(G.STAT_OPTIONS, G.STAT_RATE)
    want = (cos(G.STAT_PARAMS, G.STAT_SPOT),) + G.cos_differences(
        cos, G.STAT_PARAMS, G.STAT_SPOT, G.STAT_SPOT_BUMP, G.STAT_V0_BUMP)
    assert np.all(err > 0.0)
    for g, name in enumerate(G.NAMES):
        z = np.abs(value[:, g] - want[g]) / err[:, g]
        print(f"{name}: max |MC - COS difference| / stderr {z.max():.2f}")
        assert np.all(z <= 4.0), (name, z)
    # the price plane is the pricer's restatement, to the order of the sums
    price, perr, _, _ = R.price(G.STAT_PARAMS, G.STAT_SPOT, G.STAT_RATE, G.STAT_OPTIONS,
                                G.STAT_PATHS, G.STAT_SPY, G.STAT_SEED)
    assert np.allclose(value[:, 0], price, rtol=1e-12, atol=0.0)
    assert np.allclose(err[:, 0], perr, rtol=1e-10, atol=0.0)


def test_scaled_statistics_are_the_walk_at_the_bumped_spot():
    """Spot enters a path only as S = S0 exp(x): the base path's S, max, min and sum times u are
    those of the walk at spot S0 u, to the rounding of u (S0 e^x) against (S0 u) e^x; and the walk
    from a bumped v0_1 shares factor 2's variance path with the base walk bit for bit."""
    idx, obs = np.arange(300, dtype=np.uint64), (2, 8)
    base = R.simulate(R.STRESSED_PARAMS, 100.0, 0.03, idx, 8, 8, 5, obs)[1]
    for u in (1.0 + 1e-2, 1.0 - 1e-2):
        moved = R.simulate(R.STRESSED_PARAMS, 100.0 * u, 0.03, idx, 8, 8, 5, obs)[1]
        for j in range(2):
            got = G.scaled(base[:, j], u)
            assert np.array_equal(got[:, 1:3], moved[:, j, 1:3])
            assert np.allclose(got[:, [0, 3, 4]], moved[:, j][:, [0, 3, 4]], rtol=5e-16, atol=0.0)
            assert np.allclose(got[:, 5], moved[:, j, 5], rtol=3e-15, atol=0.0)
    sets = G.bumped_sets(R.STRESSED_PARAMS, 5e-2)
    assert sets[1, 0] > sets[0, 0] > sets[2, 0] > 0.0 and sets[3, 5] > sets[0, 5] > sets[4, 5] > 0.0
    assert np.array_equal(np.delete(sets[1:3], 0, axis=1), np.delete(sets[:1].repeat(2, 0), 0, 1))
    v1_up = R.simulate(sets[1], 100.0, 0.03, idx, 8, 8, 5, obs)[1]
    assert np.array_equal(v1_up[..., 2], base[..., 2]) and not np.array_equal(v1_up[..., 1],
                                                                              base[..., 1])


def test_knock_out_term_of_a_barrier_delta():
    """An up-and-out whose barrier lies between max and u+ max on some paths: their y_S+ is 0 while
    y_S- is not, so the delta sample carries -y_S- / (2 h), the difference quotient's knock-out
    term."""
    idx = np.arange(2000, dtype=np.uint64)
    state = R.simulate(R.README_PARAMS, 100.0, 0.03, idx, 8, 8, 5, (8,))[1][:, 0]
    o = {"strike": 90.0, "maturity": 1.0, "option_type": "call", "kind": "up_and_out",
         "barrier": 115.0}
    eps = 1e-2
    crossing = (state[:, 3] < 115.0) & ((1.0 + eps) * state[:, 3] >= 115.0) & (state[:, 0] > 95.0)
    assert crossing.sum() >= 5
    states = np.stack([state] * 5)
    g = G.samples(states, R.README_PARAMS, 100.0, o, 8, eps, 5e-2)
    want = -((1.0 - eps) * state[crossing, 0] - 90.0) / (2.0 * eps * 100.0)
    assert np.array_equal(g[1, crossing], want) and np.all(want < -1.0)
    assert np.all(g[3:] == 0.0)                   # the same states on both sides of a v0 bump


OPTS = [{"strike": 100.0, "maturity": 0.5, "option_type": "call"}]


@pytest.mark.parametrize("kw, match", [
    ({"spot_bump": 0.0}, "spot_bump"), ({"spot_bump": 1.0}, "spot_bump"),
    ({"spot_bump": float("nan")}, "spot_bump"), ({"spot_bump": -1e-2}, "spot_bump"),
    ({"v0_bump": 0.0}, "v0_bump"), ({"v0_bump": 1.5}, "v0_bump"),
    ({"v0_bump": float("inf")}, "v0_bump"), ({"n_paths": 1}, "n_paths"),
    ({"steps_per_year": 0}, "steps_per_year"), ({"seed": -1}, "seed"),
])
def test_argument_refusals(kw, match):
    import dhcos
    with pytest.raises(ValueError, match=match):
        dhcos.monte_carlo_greeks(R.README_PARAMS, 100.0, 0.03, OPTS, **kw)


def test_record_and_option_refusals():
    """monte_carlo's checks of the records and the options, and the one of its own: a v0 of 0 has
    no relative bump.  All before the library is asked for a device."""
    import dhcos
    for col, name in ((0, "v1_0"), (5, "v2_0")):
        p = np.stack([R.README_PARAMS, R.README_PARAMS])
        p[1, col] = 0.0
        with pytest.raises(ValueError, match=f"{name} of set 1 is 0"):
            dhcos.monte_carlo_greeks(p, 100.0, 0.03, OPTS)
    p = R.README_PARAMS.copy()
    p[3] = -0.3
    with pytest.raises(ValueError, match="sigma1 of set 0 must be > 0"):
        dhcos.monte_carlo_greeks(p, 100.0, 0.03, OPTS)
    with pytest.raises(ValueError, match="parameters"):
        dhcos.monte_carlo_greeks(R.README_PARAMS[:12], 100.0, 0.03, OPTS)
    with pytest.raises(ValueError, match="whole number"):
        dhcos.monte_carlo_greeks(R.README_PARAMS, 100.0, 0.03,
                                 [{"strike": 100.0, "maturity": 0.51, "option_type": "call"}])
    with pytest.raises(ValueError, match="needs a barrier"):
        dhcos.monte_carlo_greeks(R.README_PARAMS, 100.0, 0.03,
                                 [{"strike": 100.0, "maturity": 0.5, "option_type": "call",
                                   "kind": "up_and_out"}])
    with pytest.raises(ValueError, match="q = 0"):
        dhcos.DoubleHeston(100, 100, 1.0, 0.05, 0.04, 2.0, 0.04, 0.3, -0.5, 0.04, 1.5, 0.04, 0.2,
                           -0.3, 0.5, -0.05, 0.1, q=0.01).monte_carlo_greeks()


def test_exports_and_result_fields():
    import dataclasses

    import dhcos
    from dhcos import _native, montecarlo
    assert "monte_carlo_greeks" in dhcos.__all__ and "MonteCarloGreeks" in dhcos.__all__
    assert "monte_carlo_greeks" in montecarlo.__all__
    fields = [f.name for f in dataclasses.fields(dhcos.MonteCarloGreeks)]
    assert fields[:10] == [n + s for n in G.NAMES for s in ("", "_stderr")]
    assert _native.MC_GREEKS == G.NAMES
    lib = _native.load()
    assert lib.dh_mc_greeks(None, None, 1, None, 1, 2, 8, 0, 1e-2, 5e-2, None, None) == -1
    assert b"ctx is null" in lib.dh_last_error()
    res = dhcos.MonteCarloGreeks(*(np.full(2, float(k)) for k in range(10)), 4, 8, 0, 1e-2, 5e-2)
    lo, hi = res.confidence(2.0)["gamma"]
    assert np.array_equal(lo, [4.0 - 2.0 * 5.0] * 2) and np.array_equal(hi, [14.0] * 2)
