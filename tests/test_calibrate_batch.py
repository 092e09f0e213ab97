"""CPU checks of dhcos.calibrate_batch's host side (no device): argument checking, the winner rule
on stubbed per-start results, the default starts' use of the global RNG, and the new exports'
null-argument handling."""
import numpy as np
import pytest

from dhcos import batch as Bt
from dhcos import _native
from dhcos.calibrator import DoubleHestonJumpCalibrator, PARAM_NAMES, x_to_model
from dhcos.generator import MATURITIES, STRIKES_PCT


def _markets(B, seed=0):
    rs = np.random.RandomState(seed)
    spots = 100.0 + 5.0 * rs.randn(B)
    K, T, flags, mode = Bt._grid(STRIKES_PCT, MATURITIES, None, True)
    Kabs = K[None, :] * spots[:, None] / 100.0
    mkt = np.maximum(spots[:, None] - Kabs, 0.0) + 2.0 + rs.rand(B, K.size)
    return mkt, spots, np.full(B, 0.03), Kabs, T, flags


def test_grid_and_market_shapes_are_checked():
    K, T, flags, mode = Bt._grid(STRIKES_PCT, MATURITIES, None, True)
    assert K.size == T.size == 15 and flags.all() and mode == _native.STRIKE_PCT_SPOT
    assert np.array_equal(K[:5], STRIKES_PCT) and np.array_equal(T[:5], np.full(5, 0.25))
    K, T, flags, mode = Bt._grid(None, [0.5, 1.0], [90.0, 100.0, 110.0], [True, False] * 3)
    assert mode == _native.STRIKE_ABSOLUTE and K.size == 6 and flags.tolist() == [True, False] * 3
    with pytest.raises(ValueError):
        Bt._grid([], MATURITIES, None, True)
    with pytest.raises(ValueError):
        Bt._grid(STRIKES_PCT, [0.5, -1.0], None, True)
    with pytest.raises(ValueError):
        Bt._grid(STRIKES_PCT, MATURITIES, None, [True, False])
    mkt, spots, r, *_ = _markets(4)
    m, s, rr = Bt.check_markets(mkt, spots, 0.03, 15)
    assert m.shape == (4, 15) and rr.shape == (4,) and np.all(rr == 0.03)
    for bad in (dict(market_prices=mkt[:, :14]), dict(market_prices=mkt[0]),
                dict(spots=spots[:3]), dict(spots=np.where(np.arange(4) == 2, 0.0, spots)),
                dict(spots=np.where(np.arange(4) == 1, -5.0, spots)),
                dict(spots=np.where(np.arange(4) == 1, np.nan, spots)),
                dict(risk_free=np.full(3, 0.03)), dict(risk_free=np.inf)):
        args = dict(market_prices=mkt, spots=spots, risk_free=0.03)
        args.update(bad)
        with pytest.raises(ValueError):
            Bt.check_markets(args["market_prices"], args["spots"], args["risk_free"], 15)
    # the checks run before any device work
    with pytest.raises(ValueError):
        Bt.calibrate_batch(mkt, np.zeros(4), 0.03)
    with pytest.raises(ValueError):
        Bt.calibrate_batch(mkt, spots, 0.03, x0s=np.zeros((3, 2, 13)))


def test_native_batch_arguments_are_checked():
    mkt, spots, r, *_ = _markets(3)
    x0 = np.zeros((6, 13))
    mof = np.repeat(np.arange(3), 2)
    out = _native.lb_batch_args(15, mkt, spots, r, x0, mof)
    assert out[4].dtype == np.int32 and out[4].tolist() == mof.tolist()
    for bad in ([0, 0, 1, 1, 2, 3], [0, 0, 1, 1, 2, -1], [0.0, 0, 1, 1, 2, 2.5], [0, 1, 2]):
        with pytest.raises(ValueError):
            _native.lb_batch_args(15, mkt, spots, r, x0, np.array(bad))
    with pytest.raises(ValueError):
        _native.lb_batch_args(15, mkt, np.array([100.0, 0.0, 100.0]), r, x0, mof)
    with pytest.raises(ValueError):
        _native.lb_batch_args(15, mkt, spots, np.array([0.03, np.nan, 0.03]), x0, mof)
    with pytest.raises(ValueError):
        _native.lb_batch_args(14, mkt, spots, r, x0, mof)
    lib = _native.load()
    assert lib.dh_calibrate_lbfgs_batch(None, None, None, None, None, 1, None, None, 1, 128, 10.0,
                                        None, None, None) == -1
    assert b"null" in lib.dh_last_error()
    assert lib.dh_surface_loss_rows(None, None, None, None, None, 1, 1, 128, 10.0, None, None,
                                    None) == -1
    assert lib.dh_surface_loss_rows_dev(None, None, None, None, None, 1, None, None, None) == -1


def test_x0s_as_arrays_or_dicts():
    rs = np.random.RandomState(1)
    X = 0.1 * rs.randn(3, 2, 13) - 2.0
    assert np.array_equal(Bt.resolve_starts(X, 3), X)
    assert np.array_equal(Bt.resolve_starts(X.tolist(), 3), X)
    cal = DoubleHestonJumpCalibrator(100.0, 0.03, [])
    dicts = [[cal.transform_params(X[b, s]) for s in range(2)] for b in range(3)]
    got = Bt.resolve_starts(dicts, 3)
    want = np.array([[cal.inverse_transform_params(d) for d in row] for row in dicts])
    assert np.array_equal(got, want) and np.allclose(got, X, rtol=1e-12)
    with pytest.raises(ValueError):
        Bt.resolve_starts(X[:2], 3)                              # a market short
    with pytest.raises(ValueError):
        Bt.resolve_starts(X[:, :, :12], 3)
    with pytest.raises(ValueError):
        Bt.resolve_starts(X[0], 3)
    with pytest.raises(ValueError):
        Bt.resolve_starts([dicts[0], dicts[1], [dicts[2][0], X[2, 1]]], 3)   # dicts and arrays
    with pytest.raises(ValueError):
        Bt.resolve_starts([dicts[0], dicts[1], dicts[2][:1]], 3)             # ragged
    with pytest.raises(ValueError):
        Bt.resolve_starts(dicts[0] + dicts[1][:1], 3)            # [B] dicts, not [B][S]
    short = dict(dicts[0][0])
    del short["mu_j"]
    with pytest.raises(ValueError):
        Bt.resolve_starts([[short, dicts[0][1]], dicts[1], dicts[2]], 3)


def test_winner_rule():
    inf, nan = np.inf, np.nan
    fun = np.array([[3.0, 1.0, 2.0],          # plain minimum
                    [2.0, 2.0, 5.0],          # a tie: the first wins (strict <)
                    [nan, 4.0, 4.0],          # NaN never wins; then the tie rule
                    [nan, nan, nan],          # every start failed
                    [inf, inf, nan],          # inf is not below the initial inf
                    [1e10, nan, 1e10],        # an invalid-price loss still wins, as there
                    [5.0, nan, 4.0]])
    assert Bt.pick_winners(fun).tolist() == [1, 0, 1, -1, -1, 0, 2]
    lib = _native.load()
    import ctypes as C
    for row, want in zip(fun, Bt.pick_winners(fun)):          # dh_best_start's rule, row by row
        rec = np.ascontiguousarray(np.stack([np.arange(3.0), row], axis=1))
        best = C.c_int32(7)
        assert lib.dh_best_start(rec.ctypes.data, 3, 2, 0, 1, C.byref(best)) == 0
        assert best.value == want
    assert Bt.pick_winners(np.empty((2, 0))).tolist() == [-1, -1]


def test_summary_rows_on_stubbed_results():
    B, S, M = 4, 3, 15
    mkt, spots, r, Kabs, T, flags = _markets(B)
    rs = np.random.RandomState(3)
    X = 0.1 * rs.randn(B, S, 13) - 2.0
    fun = np.array([[3.0, 1.0, 2.0], [2.0, 2.0, 5.0], [np.nan] * 3, [np.nan, 7.0, 7.0]])
    nit = np.arange(B * S).reshape(B, S)
    task = np.full((B, S), 4402)
    task[0, 1] = 5504
    status = np.where(task == 4402, 0, 1)
    asked = []

    def model_prices_of(params, markets):
        asked.append(markets.tolist())
        return np.full((len(markets), M), 1.5) + markets[:, None]

    res = Bt.summarize(mkt, spots, r, Kabs, T, flags, X, fun, nit, nit + 1, task, status,
                       fun.copy(), 14 * (nit + 1), 0.01 * nit, model_prices_of)
    assert asked == [[0, 1, 3]]                                # every winner in one call
    assert res.best_start.tolist() == [1, 0, -1, 1]
    assert res.final_loss.tolist() == [1.0, 2.0, np.inf, 7.0]
    assert res.iterations.tolist() == [1, 3, 0, 10] and res.success.tolist() == [False, True,
                                                                                  False, True]
    assert np.array_equal(res.x[0], X[0, 1]) and np.array_equal(res.parameters[0],
                                                                x_to_model(X[0, 1]))
    assert np.all(res.model_prices[3] == 4.5)
    lost = res.result(2)                                       # lbfgs_calibrator.py:318-333
    assert lost.message == "All optimization starts failed" and lost.success is False
    assert lost.final_loss == np.inf and lost.iterations == 0
    assert lost.parameters == {n: 0.0 for n in PARAM_NAMES} and not np.any(lost.model_prices)
    assert np.array_equal(lost.market_prices, mkt[2])
    won = res.result(0)
    assert won.message == "STOP: TOTAL NO. OF ITERATIONS REACHED LIMIT" and won.success is False
    assert won.spot == spots[0] and won.risk_free == 0.03 and won.final_loss == 1.0
    assert [o["strike"] for o in won.market_options] == Kabs[0].tolist()
    assert res.result(1).message.startswith("CONVERGENCE")


def test_default_starts_consume_the_rng_as_the_loop_does():
    B, S = 4, 5
    mkt, spots, r, Kabs, T, flags = _markets(B)
    np.random.seed(123)
    got = Bt.default_starts(mkt, spots, r, Kabs, T, flags, S)
    state_batch = np.random.get_state()[1].copy()
    after_batch = np.random.uniform()
    np.random.seed(123)
    want = []
    for b in range(B):                       # what a loop of calibrate(multi_start=S) draws
        opts = [{"strike": Kabs[b, j], "maturity": T[j], "price": mkt[b, j],
                 "option_type": "call"} for j in range(15)]
        want.append(DoubleHestonJumpCalibrator(spots[b], r[b], opts).start_points(S))
    assert np.array_equal(np.random.get_state()[1], state_batch)
    assert np.random.uniform() == after_batch
    assert np.array_equal(got, np.array(want))
    assert not np.array_equal(got[0, 1], got[1, 1])            # guess 1 draws per market
    assert not np.array_equal(got[0, 2], got[1, 2])            # guess 2 reads the market
