"""CPU checks of the vol-space batch calibration's host side (no device): calibrate_batch's
objective / market_ivs / iv_weights checking, the three new exports in the header, the binding and
the library with their null-argument handling, and the new result fields on stubbed per-start
results (the device part is tests/test_gpu_calibrate_batch_iv.py)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

from dhcos import batch as Bt
from dhcos import _native
from dhcos.generator import MATURITIES, STRIKES_PCT

NEW = ("dh_surface_iv_sse_rows_dev", "dh_surface_loss_iv_rows", "dh_calibrate_lbfgs_batch_iv")


def _markets(B, seed=0):
    rs = np.random.RandomState(seed)
    spots = 100.0 + 5.0 * rs.randn(B)
    K, T, flags, mode = Bt._grid(STRIKES_PCT, MATURITIES, None, True)
    Kabs = K[None, :] * spots[:, None] / 100.0
    mkt = np.maximum(spots[:, None] - Kabs, 0.0) + 2.0 + rs.rand(B, K.size)
    return mkt, spots, np.full(B, 0.03), Kabs, T, flags


def test_header_binding_and_library_have_the_three_exports():
    txt = open(os.path.join(ROOT, "include", "dhcos.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    fns = set(re.findall(r"\b(dh_[a-z_]+)\s*\(", txt))
    for f in NEW:
        assert f in fns, f
        assert f in _native.SIGNATURES, f
        assert hasattr(_native.load(), f), f
    for m in ("loss_terms_iv_rows", "iv_sse_rows_dev", "calibrate_lbfgs_batch_iv"):
        assert callable(getattr(_native.Surface, m)), m


def test_null_arguments_are_rejected():
    lib = _native.load()
    for rc in (lib.dh_surface_iv_sse_rows_dev(None, None, None, None, None, None, None, 1, None,
                                              None, None, None),
               lib.dh_surface_loss_iv_rows(None, None, None, None, None, None, 1, 1, 128, 10.0,
                                           None, None, None, None),
               lib.dh_calibrate_lbfgs_batch_iv(None, None, None, None, None, None, 1, None, None,
                                               1, 128, 10.0, None, None, None)):
        assert rc == -1
        assert b"null" in lib.dh_last_error()


def test_objective_argument_is_checked_before_anything_else():
    mkt, spots, r, *_ = _markets(3)
    state = np.random.get_state()[1].copy()
    with pytest.raises(ValueError, match="bogus"):
        Bt.calibrate_batch(mkt, spots, 0.03, objective="bogus")
    with pytest.raises(ValueError, match="objective"):
        Bt.calibrate_batch(mkt, spots, 0.03, objective=None)
    # vols and weights belong to the vol objective
    with pytest.raises(ValueError, match="objective='iv'"):
        Bt.calibrate_batch(mkt, spots, 0.03, market_ivs=np.full((3, 15), 0.2))
    with pytest.raises(ValueError, match="objective='iv'"):
        Bt.calibrate_batch(mkt, spots, 0.03, objective="price", iv_weights=np.ones(15))
    assert np.array_equal(np.random.get_state()[1], state)      # no start was drawn
    assert Bt.check_objective("price") == "price" and Bt.check_objective("iv") == "iv"


def test_market_vols_and_weights_are_checked():
    B, M = 3, 15
    iv = np.full((B, M), 0.2) + 0.01 * np.arange(M)
    got_iv, got_w = Bt.check_iv_market(iv, None, B, M)
    assert got_iv.shape == (B, M) and got_iv.flags.c_contiguous and np.array_equal(got_iv, iv)
    assert got_w.shape == (B, M) and np.all(got_w == 1.0)
    w1 = np.linspace(0.0, 2.0, M)
    got_w = Bt.check_iv_market(iv, w1, B, M)[1]                 # [M]: every market's
    assert got_w.shape == (B, M) and got_w.flags.c_contiguous
    assert all(np.array_equal(got_w[b], w1) for b in range(B))
    w2 = np.arange(B * M, dtype=float).reshape(B, M)
    assert np.array_equal(Bt.check_iv_market(iv, w2, B, M)[1], w2)
    # shapes
    for bad_iv in (iv[:2], iv[:, :14], iv[0], iv.reshape(B, M, 1)):
        with pytest.raises(ValueError, match="market_ivs"):
            Bt.check_iv_market(bad_iv, None, B, M)
    for bad_w in (np.ones(14), np.ones((2, M)), np.ones((B, M, 1)), 1.0, np.ones((M, B))):
        with pytest.raises(ValueError, match="iv_weights"):
            Bt.check_iv_market(iv, bad_w, B, M)
    # signs and values of the weights
    for v in (-1.0, np.nan, np.inf):
        w = np.ones((B, M))
        w[1, 4] = v
        with pytest.raises(ValueError, match=r"\[1, 4\]"):
            Bt.check_iv_market(iv, w, B, M)
    w = np.ones((B, M))
    w[2] = 0.0
    with pytest.raises(ValueError, match=r"market\(s\) \[2\] sum to zero"):
        Bt.check_iv_market(iv, w, B, M)
    with pytest.raises(ValueError, match="sum to zero"):
        Bt.check_iv_market(iv, np.zeros(M), B, M)
    # a market vol that is not one, at a positive weight: named; at weight 0: admitted
    for v in (np.nan, -0.1, np.inf):
        hole = iv.copy()
        hole[0, 3] = hole[2, 14] = v
        with pytest.raises(ValueError, match=r"\[\[0, 3\], \[2, 14\]\]"):
            Bt.check_iv_market(hole, None, B, M)
        w = np.ones((B, M))
        w[0, 3] = w[2, 14] = 0.0
        got_iv, got_w = Bt.check_iv_market(hole, w, B, M)
        assert np.array_equal(got_w, w)
        assert np.array_equal(got_iv, hole, equal_nan=True)
    # through calibrate_batch: before any RNG draw and before any device work
    mkt, spots, r, *_ = _markets(B)
    state = np.random.get_state()[1].copy()
    hole = iv.copy()
    hole[1, 7] = np.nan
    with pytest.raises(ValueError, match=r"\[\[1, 7\]\]"):
        Bt.calibrate_batch(mkt, spots, 0.03, objective="iv", market_ivs=hole)
    with pytest.raises(ValueError, match="market_ivs"):
        Bt.calibrate_batch(mkt, spots, 0.03, objective="iv", market_ivs=iv[:2])
    with pytest.raises(ValueError, match="iv_weights"):
        Bt.calibrate_batch(mkt, spots, 0.03, objective="iv", market_ivs=iv,
                           iv_weights=np.ones(14))
    with pytest.raises(ValueError):
        Bt.calibrate_batch(mkt, spots, 0.03, objective="iv", market_ivs=iv,
                           iv_weights=-np.ones(15))
    assert np.array_equal(np.random.get_state()[1], state)


def test_native_batch_iv_arguments_are_checked():
    B, M = 3, 15
    iv = np.full((B, M), 0.2)
    got_iv, got_w = _native.iv_rows(M, iv, None)
    assert got_w.shape == (B, M) and np.all(got_w == 1.0) and got_iv.dtype == np.float64
    with pytest.raises(ValueError):
        _native.iv_rows(14, iv, None)
    with pytest.raises(ValueError):
        _native.iv_rows(M, iv, np.ones((B, 14)))
    w = np.ones((B, M))
    w[0, 0] = -0.5
    with pytest.raises(ValueError, match=r"\[0, 0\]"):
        _native.iv_rows(M, iv, w)


def test_summary_carries_the_vol_fields_on_stubbed_results():
    B, S, M = 4, 3, 15
    mkt, spots, r, Kabs, T, flags = _markets(B)
    rs = np.random.RandomState(3)
    X = 0.1 * rs.randn(B, S, 13) - 2.0
    fun = np.array([[3e-4, 1e-4, 2e-4], [2e-4, 2e-4, 5e-4], [np.nan] * 3, [np.nan, 7e-4, 7e-4]])
    nit = np.arange(B * S).reshape(B, S)
    task = np.full((B, S), 4402)
    status = np.zeros((B, S), dtype=np.int64)
    ivs = 0.2 + 0.01 * rs.rand(B, M)
    wts = np.ones((B, M))
    wts[:, 2] = 0.0
    asked = []

    def model_of(params, markets):
        asked.append(markets.tolist())
        return (np.full((len(markets), M), 1.5) + markets[:, None],
                np.full((len(markets), M), 0.25) + 0.01 * markets[:, None])

    res = Bt.summarize(mkt, spots, r, Kabs, T, flags, X, fun, nit, nit + 1, task, status,
                       fun.copy(), 14 * (nit + 1), 0.01 * nit, model_of, 7, objective="iv",
                       market_ivs=ivs, iv_weights=wts)
    assert asked == [[0, 1, 3]]                                # prices and vols from one call
    assert res.objective == "iv" and res.iterations_enqueued == 7
    assert res.market_ivs is ivs and res.iv_weights is wts
    assert res.best_start.tolist() == [1, 0, -1, 1]
    assert res.final_loss.tolist() == [1e-4, 2e-4, np.inf, 7e-4]
    assert np.all(res.model_prices[3] == 4.5) and np.all(res.model_ivs[3] == 0.28)
    assert np.all(res.model_ivs[0] == 0.25)
    assert not np.any(res.model_ivs[2]) and not np.any(res.model_prices[2])   # the failure row
    lost = res.result(2)
    assert lost.message == "All optimization starts failed" and lost.final_loss == np.inf
    assert res.result(0).final_loss == 1e-4
    # the price objective's summary: the defaults, as every existing construction gets them
    res = Bt.summarize(mkt, spots, r, Kabs, T, flags, X, fun, nit, nit + 1, task, status,
                       fun.copy(), 14 * (nit + 1), 0.01 * nit,
                       lambda p, m: np.zeros((len(m), M)))
    assert res.objective == "price"
    assert res.market_ivs is None and res.iv_weights is None and res.model_ivs is None
    with pytest.raises(ValueError, match="bogus"):
        Bt.summarize(mkt, spots, r, Kabs, T, flags, X, fun, nit, nit + 1, task, status,
                     fun.copy(), 14 * (nit + 1), 0.01 * nit, model_of, objective="bogus")
