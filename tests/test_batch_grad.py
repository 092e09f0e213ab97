"""CPU checks of calibrate_batch's gradient switch: its refusals, none of which
loads the library, its default, and the rows restatement (tests/batch_grad_reference.py) against the
one-market restatement it is built from."""
import inspect

import numpy as np
import pytest

import batch_grad_reference as BR
import param_grad_reference as R

MKT = np.full((2, 15), 5.0)
SPOTS = np.array([100.0, 101.0])
X0S = np.zeros((2, 1, 13))


def _no_native(monkeypatch):
    from dhcos import _native

    def no_load(*a, **k):
        raise AssertionError("the native library was reached")

    monkeypatch.setattr(_native, "load", no_load)
    monkeypatch.setattr(_native, "default_context", no_load)


def test_analytic_gradient_refuses_the_vol_objective(monkeypatch):
    import dhcos
    _no_native(monkeypatch)
    with pytest.raises(ValueError, match="objective"):
        dhcos.calibrate_batch(MKT, SPOTS, 0.03, x0s=X0S, gradient="analytic", objective="iv",
                              market_ivs=np.full((2, 15), 0.2))


def test_analytic_gradient_refuses_a_series_past_its_table(monkeypatch):
    import dhcos
    _no_native(monkeypatch)
    with pytest.raises(ValueError, match="N"):
        dhcos.calibrate_batch(MKT, SPOTS, 0.03, x0s=X0S, gradient="analytic", N=2048)
    with pytest.raises(ValueError, match="N"):
        dhcos.calibrate_batch(MKT, SPOTS, 0.03, x0s=X0S, gradient="analytic", N=1025)


def test_unknown_gradient_is_refused(monkeypatch):
    import dhcos
    _no_native(monkeypatch)
    with pytest.raises(ValueError, match="gradient"):
        dhcos.calibrate_batch(MKT, SPOTS, 0.03, x0s=X0S, gradient="exact")


def test_the_default_gradient_is_fd():
    import dhcos
    from dhcos import batch
    assert inspect.signature(dhcos.calibrate_batch).parameters["gradient"].default == "fd"
    assert batch.GRADIENTS == ("fd", "analytic")
    fields = {f.name: f.default for f in batch.BatchCalibrationResult.__dataclass_fields__.values()}
    assert fields["gradient"] == "fd" and fields["loss_evals"] == 0
    assert batch.check_gradient("fd", "iv", 4096) == "fd"          # "fd" carries no new limits
    assert batch.check_gradient("analytic", "price", 1024) == "analytic"


def test_binding_lists_the_new_exports():
    from dhcos import _native
    for name in ("dh_surface_loss_grad_rows", "dh_surface_loss_grad_rows_dev",
                 "dh_calibrate_lbfgs_batch_grad"):
        assert name in _native.SIGNATURES
    assert (_native.SIGNATURES["dh_calibrate_lbfgs_batch_grad"]
            == _native.SIGNATURES["dh_calibrate_lbfgs_batch"])
    for name in ("loss_grad_rows", "loss_grad_rows_dev", "calibrate_lbfgs_batch_grad"):
        assert callable(getattr(_native.Surface, name))


def test_rows_restatement_is_loss_grad_per_set(calib_golden):
    """One market: the bits of loss_grad.  Two markets: each set against its own row, whatever
    shares the call."""
    market = calib_golden["test_market"]
    X = np.array(calib_golden["guesses_seed0"][:2] + [[5.0] * 13])
    f, g = BR.loss_grad_rows(X, [market], [100.0], [0.05], [0, 0, 0], N=64)
    for s in range(3):
        want = R.loss_grad(X[s], market, 100.0, 0.05, 64)
        assert f[s] == want[0] and g[s].tobytes() == want[1].tobytes()
    assert f[2] == 1e10 and not g[2].any()
    K = np.array([o["strike"] for o in market]) * 1.02
    T = np.array([o["maturity"] for o in market])
    prices = np.array([o["price"] for o in market]) * 1.03
    other = BR.market_of_row(K, T, np.ones(15, bool), prices)
    f2, g2 = BR.loss_grad_rows(X[[1, 0]], [other, market], [102.0, 100.0], [0.04, 0.05], [0, 1],
                               N=64)
    assert f2[1] == f[0] and g2[1].tobytes() == g[0].tobytes()
    want = R.loss_grad(X[1], other, 102.0, 0.04, 64)
    assert f2[0] == want[0] and g2[0].tobytes() == want[1].tobytes() and f2[0] != f[1]
