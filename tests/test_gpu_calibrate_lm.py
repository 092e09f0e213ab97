"""GPU tests of the Levenberg-Marquardt batch calibration (dh_calibrate_lm_batch,
dhcos.calibrate_batch(method="lm"), BatchCalibrationResult.uncertainty()), on the
reference's 15-option test market and the generator's 3 x 5 grid at N = 128, at most 8 starts.

  1. replay: every traced request's (f, g) is Surface.gauss_newton_rows at the traced x, bit for
     bit; fed (f, g, H) request by request, the CPU build of the state machine
     (tests/native/liblmhost.so) asks for the same next x bit for bit and ends with the same x, fun,
     nit, nfev and code;
  2. results do not depend on the chunk size or on what else is in the batch (compaction included);
  3. fun <= the loss at x0 and best_loss == fun; maxiter = 3 stops at nit == 3 with that code; a
     start with an invalid loss at x0 ends at once with fun == 1e10 and x == x0;
  4. on 8 zero-residual markets (market prices = the device's own prices of generator-range
     parameters) from x* + 0.05 randn, LM's median final loss and median request count are not
     above those of the analytic-gradient L-BFGS-B on the same starts;
  5. uncertainty() on those markets: hessian is gauss_newton_rows at the winners' x; covariance_x @
     H is the projector onto the retained eigenspace to 13 eps condition (eigh's backward error,
     amplified by the conditioning of the retained part, which RANK_RCOND bounds by 1e12) -- the
     bar is 1e-13 min(condition, 1 / RANK_RCOND); stderr is finite where rank == 13."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
from oracle import dh_oracle as O

pytestmark = pytest.mark.gpu

LO = np.array([0.025, 1.5, 0.025, 0.2, -0.85, 0.02, 0.3, 0.025, 0.1, -0.7, 0.05, -0.08, 0.03])
HI = np.array([0.08, 4.5, 0.065, 0.5, -0.4, 0.07, 1.2, 0.07, 0.35, -0.2, 0.25, -0.01, 0.12])
MAXFUN = 1071
N = 128
TOLERANCE_STOPS = (1, 2, 3)
D = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def native():
    from dhcos import _native
    if _native.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return _native


def lmhost():
    lib = C.CDLL(os.path.join(ROOT, "tests", "native", "liblmhost.so"))
    lib.lmh_begin.argtypes = [C.c_void_p, D]
    lib.lmh_point.argtypes = [C.c_void_p, D]
    lib.lmh_set_fgh.argtypes = [C.c_void_p, C.c_double, D, D]
    lib.lmh_resume.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double]
    lib.lmh_result.argtypes = [C.c_void_p, D, D, D, C.POINTER(C.c_int)]
    return lib


def ptr(a):
    return np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(D)


@pytest.fixture(scope="module")
def zero_markets(native):
    """8 markets on the generator's grid whose prices are the device's own prices of x*, and one
    start each at x* + 0.05 randn."""
    from dhcos.generator import MATURITIES, STRIKES_PCT, grid_surface
    rs = np.random.RandomState(17)
    B = 8
    surf = grid_surface(native.default_context(), STRIKES_PCT, MATURITIES)[0]
    truth = LO + (HI - LO) * rs.rand(B, 13)
    spots = 100.0 * (1 + 0.05 * rs.randn(B))
    rates = np.full(B, 0.03)
    rec = np.zeros((B, 16))
    rec[:, :13], rec[:, 13], rec[:, 14] = truth, spots, rates
    mkt = surf.price(rec, N)
    xs = np.array([O.from_params(p) for p in truth])
    X = xs + 0.05 * rs.randn(B, 13)
    return dict(surf=surf, mkt=mkt, spots=spots, rates=rates, X=X, xs=xs)


def run_lm(m, sel, maxiter=100, chunk=8, X=None):
    sel = list(sel)
    X = m["X"][sel] if X is None else X
    res, _ = m["surf"].calibrate_lm_batch(m["mkt"][sel], m["spots"][sel], m["rates"][sel], X,
                                          np.arange(len(sel), dtype=np.int32), N,
                                          maxiter=maxiter, maxfun=MAXFUN, chunk=chunk)
    return res


def same_start(a, b):
    return (np.array_equal(np.array(a.x[:]), np.array(b.x[:])) and a.fun == b.fun
            and (a.nit, a.nfev, a.task, a.n_calls, a.warnflag) ==
            (b.nit, b.nfev, b.task, b.n_calls, b.warnflag) and a.best_loss == b.best_loss)


# ---- 1. replay -----------------------------------------------------------------------------------

def test_device_replays_bitwise_on_cpu_build(native, calib_golden):
    market = calib_golden["test_market"]
    K = np.array([o["strike"] for o in market], dtype=np.float64)
    T = np.array([o["maturity"] for o in market], dtype=np.float64)
    mkt = np.array([o["price"] for o in market], dtype=np.float64)
    x0 = np.array(calib_golden["guesses_seed0"][1], dtype=np.float64)
    ctx = native.default_context()
    surf = native.Surface(ctx, K, T, np.ones(15, bool))
    maxiter = 30
    try:
        ctx.set_lb_trace(4096)
        (res,), _ = surf.calibrate_lm_batch(mkt[None, :], [100.0], [0.05], x0[None, :], [0], N,
                                            maxiter=maxiter, maxfun=MAXFUN)
        tr = ctx.read_lb_trace()
        ctx.set_lb_trace(0)
        assert res.n_calls == res.nfev == len(tr)
        rows = tr[np.argsort(tr[:, 1])]
        assert np.array_equal(rows[:, 1], np.arange(len(rows)))
        assert np.all(rows[:, 0] == 0) and np.all(rows[:, 29] == 0)
        assert np.array_equal(rows[0, 3:16], x0)
        f, g, bad, H = surf.gauss_newton_rows(rows[:, 3:16], mkt[None, :], [100.0], [0.05],
                                              np.zeros(len(rows), np.int32), N)
    finally:
        ctx.set_lb_trace(0)
        surf.close()
    print(f"{len(rows)} requests, nit {res.nit}, code {res.task}, f0 {rows[0, 2]:.6e} fun {res.fun:.6e}")
    assert f.tobytes() == np.ascontiguousarray(rows[:, 2]).tobytes()
    assert g.tobytes() == np.ascontiguousarray(rows[:, 16:29]).tobytes()
    lib = lmhost()
    eps = np.finfo(float).eps
    st = C.create_string_buffer(lib.lmh_state_size())
    more = lib.lmh_begin(st, ptr(x0))
    xe = np.empty(13)
    k = 0
    while more:
        lib.lmh_point(st, xe.ctypes.data_as(D))
        assert np.array_equal(xe, rows[k, 3:16]), k
        lib.lmh_set_fgh(st, f[k], ptr(g[k]), ptr(H[k]))
        more = lib.lmh_resume(st, maxiter, MAXFUN, (1e-9 / eps) * eps, 1e-6)
        k += 1
    assert k == len(rows) == res.nfev
    x, fun, best, info = np.empty(13), C.c_double(), C.c_double(), (C.c_int * 5)()
    lib.lmh_result(st, x.ctypes.data_as(D), C.byref(fun), C.byref(best), info)
    assert np.array_equal(x, np.array(res.x[:])) and fun.value == res.fun
    assert best.value == res.best_loss
    assert list(info) == [res.nit, res.nfev, res.task, res.warnflag, res.n_calls]
    assert res.nit >= 2 and res.fun < rows[0, 2]


# ---- 2. invariance, 3. the ends ---------------------------------------------------------------

def test_results_do_not_depend_on_chunk_or_batch(zero_markets):
    m = zero_markets
    base = run_lm(m, range(8), maxiter=12)
    print("nfev:", [q.nfev for q in base], "codes:", [q.task for q in base])
    for chunk in (1, 3):
        got = run_lm(m, range(8), maxiter=12, chunk=chunk)
        assert all(same_start(a, b) for a, b in zip(got, base)), chunk
    alone = run_lm(m, [5], maxiter=12)[0]
    assert same_start(alone, base[5])
    # a start at the minimiser itself finishes at its first request: compaction with 7 others live
    sel = [3, 5, 0, 6, 1, 7, 2, 4]
    X = m["X"][sel].copy()
    X[2] = m["xs"][0]
    mixed = run_lm(m, sel, maxiter=12, X=X, chunk=1)
    assert mixed[2].nfev == 1 and mixed[2].nit == 0 and mixed[2].task == 1
    for i, b in enumerate(sel):
        if i != 2:
            assert same_start(mixed[i], base[b]), (i, b)
    assert len({q.nfev for q in mixed}) > 1


def test_monotone_maxiter_and_invalid_x0(zero_markets):
    m = zero_markets
    X = m["X"].copy()
    X[7, 0] = X[7, 5] = 40.0                          # v0 = e^40: prices not finite
    f0 = m["surf"].loss_grad_rows(X, m["mkt"], m["spots"], m["rates"], np.arange(8), N)[0]
    assert f0[7] == 1e10 and np.all(np.isfinite(f0[:7]))
    res = run_lm(m, range(8), maxiter=3, X=X)
    for i, q in enumerate(res[:7]):
        print(f"start {i}: f0 {f0[i]:.6e} fun {q.fun:.6e} nit {q.nit} nfev {q.nfev} code {q.task}")
        assert q.fun <= f0[i] and q.best_loss == q.fun and q.n_calls == q.nfev
        assert q.nit <= 3 and (q.task == 4 and q.nit == 3 or q.task in TOLERANCE_STOPS)
    assert any(q.task == 4 and q.nit == 3 and q.warnflag == 1 for q in res[:7])
    bad = res[7]
    assert bad.fun == 1e10 and np.array_equal(np.array(bad.x[:]), X[7])
    assert (bad.task, bad.nit, bad.nfev, bad.warnflag) == (7, 0, 1, 2)
    assert bad.best_loss == np.inf


# ---- 4. convergence against the existing driver, 5. uncertainty ----------------------------------

def test_lm_is_not_behind_lbfgs_on_zero_residual_markets(native, zero_markets):
    import dhcos
    m = zero_markets
    lm = dhcos.calibrate_batch(m["mkt"], m["spots"], m["rates"], x0s=m["X"][:, None, :],
                               maxiter=100, method="lm")
    lb = dhcos.calibrate_batch(m["mkt"], m["spots"], m["rates"], x0s=m["X"][:, None, :],
                               maxiter=100, gradient="analytic")
    for name, r in (("lm", lm), ("lbfgs analytic", lb)):
        print(f"{name}: losses {np.array2string(r.fun[:, 0], precision=3)} requests "
              f"{r.nfev[:, 0].tolist()} tolerance stops {int(r.success.sum())}/8 codes "
              f"{r.task.tolist()}")
    print(f"medians: loss lm {np.median(lm.fun):.3e} lbfgs {np.median(lb.fun):.3e}; requests lm "
          f"{np.median(lm.nfev)} lbfgs {np.median(lb.nfev)}")
    assert lm.method == "lm" and lb.method == "lbfgs" and lm.gradient == "analytic"
    assert np.array_equal(lm.n_calls, lm.nfev) and np.all(lm.best_start == 0)
    assert np.median(lm.fun) <= np.median(lb.fun)
    assert np.median(lm.nfev) <= np.median(lb.nfev)
    assert all(lm.message(b) == native.LM_MESSAGES[int(lm.task[b])] for b in range(8))
    # 5. uncertainty() at the winners
    u = lm.uncertainty()
    f, g, bad, H = m["surf"].gauss_newton_rows(lm.x, m["mkt"], m["spots"], m["rates"],
                                               np.arange(8), N)
    assert u.hessian.tobytes() == H.tobytes() and u.dof == 2
    from dhcos.batch import RANK_RCOND
    for b in range(8):
        e, V = np.linalg.eigh(H[b])
        keep = e > RANK_RCOND * e[-1]
        proj = V[:, keep] @ V[:, keep].T
        got = u.covariance_x[b] @ H[b] / (2.0 * f[b] / u.dof) if f[b] > 0 else proj
        bar = 1e-13 * min(u.condition[b], 1.0 / RANK_RCOND)
        print(f"market {b}: condition {u.condition[b]:.3e} rank {u.rank[b]} projector err "
              f"{np.max(np.abs(got - proj)):.3e} bar {bar:.3e}")
        assert u.rank[b] == keep.sum()
        assert np.max(np.abs(got - proj)) <= bar
        if u.rank[b] == 13:
            assert np.all(np.isfinite(u.stderr[b]))
    ub = lb.uncertainty()                               # works after either method
    assert ub.hessian.shape == (8, 13, 13) and np.all(ub.rank >= 1)
