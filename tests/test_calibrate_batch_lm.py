"""calibrate_batch(method=...) argument handling and ParameterUncertainty's algebra: no device.

The algebra is held to closed forms on hand-made Hessians:
  * diagonal H = diag(h): pinv = diag(1 / h), covariance_x = 2 f / dof diag(1 / h), condition =
    max h / min h, weakest = the axis of min h, rank 13 -- to 1e-12 relative (a dozen roundings of
    eigh and the products on entries of order one);
  * H = Q diag(h) Q' with one h exactly 0 (rank 12): that direction is cut, covariance_x @ H is the
    projector I - q q' (to 1e-9: eigh's error 13 eps times the condition 1e4 of the kept part);
  * a market without a winner: NaN and rank -1."""
import inspect

import numpy as np
import pytest

from dhcos import ParameterUncertainty, _native, batch as Bt, calibrate_batch

M = 15
MKT = np.full((1, M), 5.0)


def test_method_values_and_refusals():
    with pytest.raises(ValueError, match="method must be 'lbfgs' or 'lm'"):
        calibrate_batch(MKT, [100.0], 0.03, method="gauss")
    with pytest.raises(ValueError, match="price objective only"):
        calibrate_batch(MKT, [100.0], 0.03, method="lm", objective="iv")
    with pytest.raises(ValueError, match="gradient='vega'"):
        calibrate_batch(MKT, [100.0], 0.03, method="lm", gradient="vega")
    for bad_n in (0, 1025, 128.0):
        with pytest.raises(ValueError, match="method='lm': N must be a whole number"):
            calibrate_batch(MKT, [100.0], 0.03, method="lm", N=bad_n)
    assert Bt.check_method("lm", "fd", "price", 1024) == "lm"
    assert Bt.check_method("lm", "analytic", "price", 1) == "lm"
    assert Bt.check_method("lbfgs", "fd", "iv", 4096) == "lbfgs"      # lbfgs: check_gradient's job
    # the default optimiser's checks are unchanged
    with pytest.raises(ValueError, match="gradient must be"):
        calibrate_batch(MKT, [100.0], 0.03, gradient="exact")
    with pytest.raises(ValueError, match="gradient='analytic': N"):
        calibrate_batch(MKT, [100.0], 0.03, gradient="analytic", N=2048)


def test_defaults_are_unchanged():
    sig = inspect.signature(calibrate_batch)
    assert sig.parameters["gradient"].default == "fd"
    assert sig.parameters["method"].default == "lbfgs"
    assert Bt.BatchCalibrationResult.__dataclass_fields__["method"].default == "lbfgs"


def test_message_map():
    assert sorted(_native.LM_MESSAGES) == [1, 2, 3, 4, 5, 6, 7]
    for code in (1, 2, 3):
        assert Bt.task_message(code, "lm").startswith("CONVERGENCE")
    assert Bt.task_message(4, "lm").startswith("STOP") and "MAXITER" in Bt.task_message(4, "lm")
    assert "MAXFUN" in Bt.task_message(5, "lm")
    assert Bt.task_message(6, "lm").startswith("ABNORMAL")
    assert "X0" in Bt.task_message(7, "lm")
    assert Bt.task_message(4401).startswith("CONVERGENCE")            # SciPy's, as before
    # through a result: the winner's code under its method, the failure row's message
    B, S = 2, 1
    z = np.zeros
    fun = np.array([[0.5], [np.nan]])
    res = Bt.summarize(np.ones((B, M)), np.full(B, 100.0), np.full(B, 0.03), np.ones((B, M)),
                       np.ones(M), np.ones(M, bool), z((B, S, 13)), fun, z((B, S), int),
                       z((B, S), int), np.array([[2], [6]]), np.array([[0], [2]]), fun,
                       z((B, S), int), z((B, S)), lambda p, w: np.ones((len(w), M)), method="lm")
    assert res.method == "lm" and res.message(0) == _native.LM_MESSAGES[2]
    assert res.success[0] and not res.success[1] and res.message(1) == Bt.FAILED_MESSAGE
    with pytest.raises(ValueError, match="option grid"):
        res.uncertainty()


def test_uncertainty_algebra_diagonal():
    h = np.array([4.0, 1.0, 9.0, 2.0, 0.5, 3.0, 7.0, 0.25, 5.0, 6.0, 8.0, 10.0, 1.5])
    x = np.linspace(-1.0, 1.0, 13)
    f = 3e-4
    u = Bt.gauss_newton_uncertainty(np.diag(h)[None], [f], x[None], M)
    assert isinstance(u, ParameterUncertainty) and u.dof == 2 and u.rank[0] == 13
    want = 2.0 * f / 2 * np.diag(1.0 / h)
    assert np.allclose(u.covariance_x[0], want, rtol=1e-12, atol=1e-18)
    assert np.isclose(u.condition[0], 10.0 / 0.25, rtol=1e-12)
    e7 = np.zeros(13)
    e7[7] = 1.0
    assert np.allclose(u.weakest[0], e7, atol=1e-12)
    j = np.exp(x)
    j[[4, 9]] = 1.0 - np.tanh(x[[4, 9]]) ** 2
    j[11] = 1.0
    assert np.allclose(Bt.transform_jacobian(x), j, rtol=1e-15)
    assert np.allclose(u.stderr[0], j * np.sqrt(f / h), rtol=1e-12)
    assert np.allclose(u.covariance[0], np.diag(j * j * f / h), rtol=1e-12, atol=1e-18)
    assert Bt.gauss_newton_uncertainty(np.eye(13)[None], [f], x[None], 70).dof == 57


def test_uncertainty_algebra_rank_deficient():
    rs = np.random.RandomState(3)
    Q, _ = np.linalg.qr(rs.randn(13, 13))
    h = np.logspace(0, 4, 13)
    h[5] = 0.0
    H = (Q * h) @ Q.T
    H = 0.5 * (H + H.T)
    u = Bt.gauss_newton_uncertainty(H[None], [1e-3], np.zeros((1, 13)), 28)
    assert u.rank[0] == 12 and u.dof == 15
    assert u.condition[0] > 1e12                                       # inf, or 1 / a rounding
    q = Q[:, 5]
    assert abs(abs(u.weakest[0] @ q) - 1.0) <= 1e-9
    proj = u.covariance_x[0] @ H / (2.0 * 1e-3 / 15)
    assert np.allclose(proj, np.eye(13) - np.outer(q, q), atol=1e-9)
    assert np.all(np.isfinite(u.stderr[0]))


def test_uncertainty_without_a_winner():
    H = np.stack([np.eye(13), np.full((13, 13), np.nan)])
    u = Bt.gauss_newton_uncertainty(H, [1e-3, np.nan], np.zeros((2, 13)), M,
                                    valid=[True, False])
    assert u.rank.tolist() == [13, -1]
    assert np.all(np.isfinite(u.covariance[0]))
    for a in (u.hessian[1], u.covariance_x[1], u.covariance[1], u.stderr[1], u.weakest[1]):
        assert np.all(np.isnan(a))
    assert np.isnan(u.condition[1])
