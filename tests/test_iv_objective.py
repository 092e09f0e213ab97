"""CPU-side checks of the implied-vol calibration objective: the C-ABI boundary of
dh_surface_set_iv_market, dh_surface_iv_sse_dev, dh_surface_loss_iv_dev and dh_surface_loss_iv
without a device, and DoubleHestonJumpCalibrator(objective="iv")'s host arithmetic and bookkeeping
over a stub surface (the device part is tests/test_gpu_iv_objective.py)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ("dh_surface_set_iv_market", "dh_surface_iv_sse_dev", "dh_surface_loss_iv_dev",
       "dh_surface_loss_iv")


def header_functions():
    txt = open(os.path.join(ROOT, "include", "dhcos.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(dh_[a-z_]+)\s*\(", txt))


def market(n=6):
    return [{"strike": 90.0 + 4.0 * i, "maturity": 0.5 + 0.25 * (i % 3), "price": 5.0 + i,
             "option_type": "call" if i % 2 else "put"} for i in range(n)]


class StubSurface:
    """loss_terms_iv answers with fixed (sse, n_bad) rows, cycled over the request's records."""

    def __init__(self, sse, bad):
        self.sse, self.bad = np.asarray(sse, dtype=np.float64), np.asarray(bad, dtype=np.int32)
        self.calls = []

    def loss_terms_iv(self, rec, N=128, L=10.0, want_prices=False, want_iv=False):
        rec = np.asarray(rec)
        self.calls.append((rec.copy(), N))
        idx = np.arange(rec.shape[0]) % self.sse.size
        return self.sse[idx].copy(), self.bad[idx].copy()

    def loss_terms(self, *a, **k):
        raise AssertionError("the price objective's request under objective='iv'")

    def fg(self, *a, **k):
        raise AssertionError("dh_surface_fg under objective='iv'")


def stub_cal(sse, bad, weights=None, n=6):
    from dhcos import DoubleHestonJumpCalibrator
    cal = DoubleHestonJumpCalibrator(100.0, 0.03, market(n), objective="iv",
                                     market_ivs=np.full(n, 0.2), iv_weights=weights)
    stub = StubSurface(sse, bad)
    cal._get_surface = lambda: stub
    return cal, stub


def test_header_and_binding_have_the_four_functions():
    from dhcos import _native
    fns = header_functions()
    for f in NEW:
        assert f in fns, f
        assert f in _native.SIGNATURES, f
        assert hasattr(_native.load(), f), f
    for m in ("set_iv_market", "loss_terms_iv", "iv_sse_dev", "loss_iv_dev"):
        assert callable(getattr(_native.Surface, m)), m


def test_null_arguments_are_rejected():
    from dhcos import _native
    lib = _native.load()
    a = np.ones(4)
    b = np.zeros(4, dtype=np.int32)
    p, q = a.ctypes.data, b.ctypes.data
    for rc in (lib.dh_surface_set_iv_market(None, p, p),
               lib.dh_surface_set_iv_market(None, None, None),
               lib.dh_surface_iv_sse_dev(None, None, p, p, 1, p, q, None, None),
               lib.dh_surface_loss_iv_dev(None, None, p, 1, 128, 10.0, p, q, None, None, None),
               lib.dh_surface_loss_iv(None, None, p, 1, 128, 10.0, p, q, None, None)):
        assert rc == -1
        assert b"null" in lib.dh_last_error()


def test_objective_argument():
    from dhcos import DoubleHestonJumpCalibrator
    cal = DoubleHestonJumpCalibrator(100.0, 0.03, market())
    assert cal.objective == "price"
    with pytest.raises(ValueError, match="bogus"):
        DoubleHestonJumpCalibrator(100.0, 0.03, market(), objective="bogus")
    with pytest.raises(ValueError):
        DoubleHestonJumpCalibrator(100.0, 0.03, market(), objective="iv",
                                   iv_weights=[1, 1, -1, 1, 1, 1])
    with pytest.raises(ValueError):
        DoubleHestonJumpCalibrator(100.0, 0.03, market(), objective="iv", iv_weights=np.zeros(6))
    w = np.array([1.0, 0.0, 2.0, 0.5, 0.0, 3.0])
    cal = DoubleHestonJumpCalibrator(100.0, 0.03, market(), objective="iv",
                                     market_ivs=np.full(6, 0.25), iv_weights=w)
    assert cal.objective == "iv"
    assert np.array_equal(cal.market_ivs, np.full(6, 0.25)) and np.array_equal(cal.iv_weights, w)
    cal = DoubleHestonJumpCalibrator(100.0, 0.03, market(), objective="iv")
    assert cal.market_ivs is None and np.array_equal(cal.iv_weights, np.ones(6))   # vols: lazily


def test_device_driver_is_refused_before_any_draw():
    from dhcos import DoubleHestonJumpCalibrator
    cal = DoubleHestonJumpCalibrator(100.0, 0.03, market(), objective="iv")
    np.random.seed(5)
    before = np.random.get_state()
    with pytest.raises(ValueError, match="device"):
        cal.calibrate(maxiter=3, multi_start=3, driver="device")
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1])
    assert before[2:] == after[2:]


def test_loss_batch_formula_and_bookkeeping():
    from dhcos import calibrator as C
    sse = np.array([0.5, 0.25, 3.0, 0.125, 7.0])
    bad = np.array([0, 0, 2, 0, 1])
    w = np.array([1.0, 0.0, 2.0, 0.5, 0.25, 3.0])
    cal, stub = stub_cal(sse, bad, w)
    rng = np.random.RandomState(3)
    X = np.tile(cal.get_initial_guess(0), (5, 1)) + 0.3 * rng.standard_normal((5, 13))
    X[1, 3] = np.log(2.0)                     # sigma1 = 2: Feller violated, a positive penalty
    P = C.x_to_model(X)
    pen = C.feller_penalty(P)
    assert pen[1] > 0
    want = np.where(bad > 0, 1e10, sse / w.sum() + pen)
    got = cal.loss_batch(X)
    assert np.array_equal(got, want)
    assert cal.n_calls == 5 and cal.loss_evals == 5
    valid = want[bad == 0]
    assert cal.best_loss == valid.min()
    (rec, N), = stub.calls
    assert N == cal.N and rec.shape == (5, 16)
    assert np.array_equal(rec[:, :13], P)
    assert np.all(rec[:, 13] == 100.0) and np.all(rec[:, 14] == 0.03) and np.all(rec[:, 15] == 0.0)
    # track=False: the evaluations count, n_calls and best_loss stay
    cal.loss_batch(X[:2], track=False)
    assert cal.n_calls == 5 and cal.loss_evals == 7 and cal.best_loss == valid.min()
    # compute_loss and compute_loss_and_grad follow from loss_batch
    one = cal.compute_loss(X[3])              # a request of one record: the stub's row 0
    assert isinstance(one, float) and one == sse[0] / w.sum() + pen[3]
    assert cal.n_calls == 6
    f, g = cal.compute_loss_and_grad(X[0])
    assert cal.n_calls == 20 and g.shape == (13,)
    assert stub.calls[-1][0].shape == (14, 16)


def test_price_objective_bookkeeping_is_the_same():
    """The same stub answers under objective='price' through loss_terms: the two objectives differ
    in the normaliser only (sum of the weights against M)."""
    from dhcos import DoubleHestonJumpCalibrator
    sse = np.array([0.5, 0.25, 3.0, 0.125, 7.0])
    bad = np.array([0, 0, 2, 0, 1])
    cal_iv, _ = stub_cal(sse, bad)                                  # unit weights: sum = M = 6
    cal_p = DoubleHestonJumpCalibrator(100.0, 0.03, market())

    class PriceStub:
        def loss_terms(self, rec, N=128, L=10.0, want_prices=False):
            return sse.copy(), bad.astype(np.int32), None

    cal_p._get_surface = lambda: PriceStub()
    X = np.tile(cal_p.get_initial_guess(0), (5, 1)) + 0.1 * np.arange(5)[:, None]
    assert np.array_equal(cal_iv.loss_batch(X), cal_p.loss_batch(X))
    assert (cal_iv.n_calls, cal_iv.best_loss, cal_iv.loss_evals) == \
        (cal_p.n_calls, cal_p.best_loss, cal_p.loss_evals)


def test_empty_market_and_unresolvable_type():
    from dhcos import DoubleHestonJumpCalibrator
    cal = DoubleHestonJumpCalibrator(100.0, 0.03, [], objective="iv")
    out = cal.loss_batch(np.zeros((3, 13)))
    assert out.shape == (3,) and np.all(np.isnan(out))
    opts = market()
    opts[2]["option_type"] = ""
    cal = DoubleHestonJumpCalibrator(100.0, 0.03, opts, objective="iv")
    assert np.array_equal(cal.loss_batch(np.zeros((2, 13))), np.full(2, 1e10))


def test_fg_batch_is_one_request_of_14_points_per_start():
    from dhcos import calibrator as C
    rng = np.random.RandomState(8)
    sse = rng.uniform(0.1, 2.0, size=42)
    bad = np.zeros(42, dtype=np.int32)
    bad[17] = 1
    cal, stub = stub_cal(sse, bad)
    X0 = np.tile(cal.get_initial_guess(0), (3, 1)) + 0.2 * rng.standard_normal((3, 13))
    f, g, low = cal.fg_batch(X0)
    assert len(stub.calls) == 1
    rec, _ = stub.calls[0]
    assert rec.shape == (14 * 3, 16)
    X, dx = C.fd_request_points_many(X0)
    assert np.array_equal(rec[:, :13], C.x_to_model(X))
    F = np.where(bad > 0, 1e10, sse / 6.0 + C.feller_penalty(C.x_to_model(X))).reshape(3, 14)
    wf, wg, wlow = C._fg_rows(F, dx)
    assert np.array_equal(f, wf) and np.array_equal(g, wg) and np.array_equal(low, wlow)
    assert cal.n_calls == 0 and cal.loss_evals == 42          # track=False, as the price objective
    # the loops take the generic path: no request slot for this objective
    assert C._native_surface(cal, 1) is None
    assert C._pipeline_surface(cal, 3, True) is None
