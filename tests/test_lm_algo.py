"""The Levenberg-Marquardt state machine (csrc/dh_lm.h) on the CPU: its build
(tests/native/liblmhost.so) against the NumPy restatement (tests/lm_reference.py) bit for bit,
request by request, and its minima against scipy.optimize.least_squares(method="lm").

Problems are residual problems r(x) in 13 variables with the calibration loss's scaling:
f = sum r^2 / M, g = 2 J'r / M, H = 2 J'J / M.

Bars against SciPy (derived, not measured):
  * Rosenbrock (zero residual, H nonsingular at the minimiser): the run stops on max |g_i| <= pgtol,
    and near x* g = H (x - x*), so |x - x*|_2 <= sqrt(13) pgtol / lambda_min(H(x*)); doubled for
    the second-order term, plus SciPy's own stop (xtol = 1e-14 relative, on |x| ~ sqrt(13)).
  * Powell's singular function (H singular at x* = 0: r is quadratic in two directions): there
    f ~ |x|^4 and |g| ~ |x|^3 along the flat directions with unit-order constants (the smallest
    quartic coefficient is 1), so a pgtol stop gives |x| <= (pgtol)^(1/3) up to that constant; the
    bar is 3 pgtol^(1/3) against x* = 0, for both optimisers at the same tolerance."""
import ctypes as C
import os

import numpy as np
import pytest
from scipy.optimize import least_squares

import lm_reference as R
from conftest import ROOT

N = 13
D = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def lib():
    so = C.CDLL(os.path.join(ROOT, "tests", "native", "liblmhost.so"))
    so.lmh_begin.argtypes = [C.c_void_p, D]
    so.lmh_point.argtypes = [C.c_void_p, D]
    so.lmh_set_fgh.argtypes = [C.c_void_p, C.c_double, D, D]
    so.lmh_resume.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double]
    so.lmh_damping.argtypes = [C.c_void_p, D]
    so.lmh_result.argtypes = [C.c_void_p, D, D, D, C.POINTER(C.c_int)]
    return so


def p(a):
    return np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(D)


# ---- residual problems ---------------------------------------------------------------------------

def rosenbrock(x):
    r, J = np.zeros(N), np.zeros((N, N))
    for i in range(6):
        a, b = 2 * i, 2 * i + 1
        r[a], J[a, a], J[a, b] = 10.0 * (x[b] - x[a] ** 2), -20.0 * x[a], 10.0
        r[b], J[b, a] = 1.0 - x[a], -1.0
    r[12], J[12, 12] = x[12] - 1.0, 1.0
    return r, J


def powell(x):
    r, J = np.zeros(N), np.zeros((N, N))
    for i in range(3):
        a = 4 * i
        x1, x2, x3, x4 = x[a:a + 4]
        r[a], J[a, a], J[a, a + 1] = x1 + 10.0 * x2, 1.0, 10.0
        r[a + 1], J[a + 1, a + 2], J[a + 1, a + 3] = np.sqrt(5.0) * (x3 - x4), np.sqrt(5.0), -np.sqrt(5.0)
        r[a + 2] = (x2 - 2.0 * x3) ** 2
        J[a + 2, a + 1], J[a + 2, a + 2] = 2.0 * (x2 - 2.0 * x3), -4.0 * (x2 - 2.0 * x3)
        r[a + 3] = np.sqrt(10.0) * (x1 - x4) ** 2
        J[a + 3, a], J[a + 3, a + 3] = (2.0 * np.sqrt(10.0) * (x1 - x4),
                                        -2.0 * np.sqrt(10.0) * (x1 - x4))
    r[12], J[12, 12] = x[12], 1.0
    return r, J


def deficient(x):
    """Rosenbrock in (x0 + x1, x2): columns 0 and 1 of J are equal everywhere and columns 3.. are
    zero, so J'J is singular at every point; only the damping makes the step's matrix definite."""
    r, J = np.zeros(N), np.zeros((N, N))
    u = x[0] + x[1]
    r[0], r[1] = 10.0 * (x[2] - u * u), 1.0 - u
    J[0, 0] = J[0, 1] = -20.0 * u
    J[0, 2] = 10.0
    J[1, 0] = J[1, 1] = -1.0
    return r, J


def fgh(problem, x):
    r, J = problem(np.asarray(x, dtype=np.float64))
    return float(r @ r) / N, 2.0 * (J.T @ r) / N, 2.0 * (J.T @ J) / N


X0 = {"rosenbrock": np.array([-1.2, 1.0] * 6 + [0.5]),
      "powell": np.array([3.0, -1.0, 0.0, 1.0] * 3 + [2.0]),
      "deficient": np.array([-0.7, -0.5, 1.0] + [0.3] * 10)}
PROBLEMS = {"rosenbrock": rosenbrock, "powell": powell, "deficient": deficient}


def run_both(lib, evaluate, x0, maxiter=200, maxfun=1000, ftol=1e-9, pgtol=1e-6, limit=2000):
    """Drive the CPU build and the restatement with the same answers; every requested point and the
    damping state must agree bit for bit -> (reference machine, result of the CPU build)."""
    st = C.create_string_buffer(lib.lmh_state_size())
    more = lib.lmh_begin(st, p(x0))
    ref = R.Lm(x0, maxiter, maxfun, ftol, pgtol)
    xe, damp = np.empty(N), np.empty(3)
    k = 0
    while more:
        assert ref.more and k < limit
        lib.lmh_point(st, xe.ctypes.data_as(D))
        assert xe.tobytes() == np.array(ref.xe).tobytes(), k
        f, g, H = evaluate(k, xe.copy())
        lib.lmh_set_fgh(st, f, p(g), p(H))
        more = lib.lmh_resume(st, maxiter, maxfun, ftol, pgtol)
        ref.resume(f, g, H)
        lib.lmh_damping(st, damp.ctypes.data_as(D))
        want = np.array([ref.lam, ref.nu, ref.pred])
        nan = np.isnan(want)                     # a NaN's sign and payload are not held
        assert np.array_equal(np.isnan(damp), nan) and damp[~nan].tobytes() == want[~nan].tobytes(), k
        k += 1
    assert not ref.more
    x, fun, best, info = np.empty(N), C.c_double(), C.c_double(), (C.c_int * 5)()
    lib.lmh_result(st, x.ctypes.data_as(D), C.byref(fun), C.byref(best), info)
    assert x.tobytes() == np.array(ref.x).tobytes()
    assert np.array([fun.value]).tobytes() == np.array([ref.f]).tobytes()
    assert list(info) == [ref.nit, ref.nfev, ref.task, ref.warnflag, ref.n_calls]
    assert k == ref.n_calls
    return ref, dict(x=x, fun=fun.value, best=best.value, nit=info[0], nfev=info[1], task=info[2],
                     warnflag=info[3], n_calls=info[4])


@pytest.mark.parametrize("name", ["rosenbrock", "powell", "deficient"])
def test_cpu_build_is_the_restatement_bit_for_bit(lib, name):
    prob = PROBLEMS[name]
    f0 = fgh(prob, X0[name])[0]
    ref, out = run_both(lib, lambda k, x: fgh(prob, x), X0[name], ftol=0.0, pgtol=1e-10)
    print(f"{name}: nit {out['nit']} nfev {out['nfev']} task {out['task']} fun {out['fun']:.3e} "
          f"lambda {ref.lam:.3e}")
    assert out["nfev"] == out["n_calls"] and out["nit"] < out["nfev"]
    assert out["fun"] <= f0 and out["best"] == out["fun"]
    assert out["fun"] == fgh(prob, out["x"])[0]          # fun is the loss AT the returned x
    assert out["task"] in (R.GTOL, R.XTOL_STOP) and out["warnflag"] == 0
    assert out["fun"] < 1e-12


def test_a_pivot_that_is_not_positive_is_retried_without_a_request(lib):
    """An indefinite H from the caller (no J'J is, but a rounded singular one can be): the factor
    fails, lambda grows by nu, 2 nu, ... inside one resume and the next request follows; a diagonal
    the damping cannot lift (D is floored at 1e-12) ends as STALLED."""
    H = np.eye(N)
    H[3, 3] = -1e-9                      # needs lambda 1e-12 > 1e-9: lambda > 1e3

    def evaluate(k, x):
        return float(x @ x), 2.0 * x, H

    ref, out = run_both(lib, evaluate, np.full(N, 0.5), maxiter=1)
    assert out["nfev"] >= 2 and ref.lam > 1e3            # steps were formed after the retries
    H3 = H.copy()
    H3[3, 3] = -1e6                      # lambda 1e-12 > 1e6 is past the ceiling 1e16
    ref, out = run_both(lib, lambda k, x: (float(x @ x), 2.0 * x, H3), np.full(N, 0.5))
    assert out["task"] == R.STALLED and out["warnflag"] == 2 and out["nfev"] == 1
    assert np.array_equal(out["x"], np.full(N, 0.5))


def test_an_invalid_trial_is_rejected_and_the_run_recovers(lib):
    calls = []

    def evaluate(k, x):
        f, g, H = fgh(rosenbrock, x)
        if k in (1, 2):                  # the first two trials are invalid: the 1e10 marker, NaN
            calls.append(k)
            return (1e10 if k == 1 else float("nan")), np.zeros(N), np.zeros((N, N))
        return f, g, H

    ref, out = run_both(lib, evaluate, X0["rosenbrock"], ftol=0.0, pgtol=1e-10)
    assert calls == [1, 2] and out["task"] == R.GTOL and out["fun"] < 1e-12
    assert out["nit"] <= out["nfev"] - 3


@pytest.mark.parametrize("f0", [1e10, float("nan")])
def test_an_invalid_loss_at_x0_ends_at_once(lib, f0):
    x0 = X0["powell"]
    ref, out = run_both(lib, lambda k, x: (f0, np.zeros(N), np.zeros((N, N))), x0)
    assert out["task"] == R.INVALID_X0 and out["warnflag"] == 2
    assert (out["nit"], out["nfev"], out["n_calls"]) == (0, 1, 1)
    assert np.array_equal(out["x"], x0) and (out["fun"] == f0 or f0 != f0 and out["fun"] != out["fun"])
    assert out["best"] == np.inf


def test_each_stop_code(lib):
    ev = lambda k, x: fgh(rosenbrock, x)                                   # noqa: E731
    x0 = X0["rosenbrock"]
    assert run_both(lib, ev, x0, ftol=0.0, pgtol=1e-8)[1]["task"] == R.GTOL
    out = run_both(lib, ev, x0, ftol=1e-3, pgtol=0.0)[1]
    assert out["task"] == R.FTOL and out["warnflag"] == 0
    out = run_both(lib, ev, x0, maxiter=3, ftol=0.0, pgtol=0.0)[1]
    assert (out["task"], out["nit"], out["warnflag"]) == (R.MAXITER, 3, 1)
    out = run_both(lib, ev, x0, maxfun=4, ftol=0.0, pgtol=0.0)[1]
    assert (out["task"], out["nfev"], out["warnflag"]) == (R.MAXFUN, 4, 1)
    out = run_both(lib, ev, x0, ftol=-1.0, pgtol=-1.0)[1]                   # neither can fire
    assert out["task"] in (R.XTOL_STOP, R.STALLED)
    # the minimiser itself: g = 0 at x0
    out = run_both(lib, ev, np.ones(N))[1]
    assert (out["task"], out["nit"], out["nfev"]) == (R.GTOL, 0, 1)
    # every trial invalid: lambda climbs until the step is below xtol, or to its ceiling
    out = run_both(lib, lambda k, x: fgh(rosenbrock, x) if k == 0 else (1e10, 0 * x, np.zeros((N, N))),
                   x0)[1]
    assert out["task"] in (R.XTOL_STOP, R.STALLED) and out["nit"] == 0
    assert np.array_equal(out["x"], x0)
    # a NaN gradient: no step can be formed
    out = run_both(lib, lambda k, x: (1.0, np.full(N, np.nan), np.eye(N)), x0)[1]
    assert out["task"] == R.STALLED


def test_minima_agree_with_scipy_least_squares(lib):
    pgtol = 1e-10
    # Rosenbrock
    out = run_both(lib, lambda k, x: fgh(rosenbrock, x), X0["rosenbrock"], ftol=0.0, pgtol=pgtol)[1]
    sp = least_squares(lambda x: rosenbrock(x)[0], X0["rosenbrock"], jac=lambda x: rosenbrock(x)[1],
                       method="lm", xtol=1e-14, ftol=1e-14, gtol=1e-14)
    lam_min = np.linalg.eigvalsh(fgh(rosenbrock, np.ones(N))[2])[0]
    bar = 2.0 * np.sqrt(N) * pgtol / lam_min + 1e-14 * np.sqrt(N)
    err = np.linalg.norm(out["x"] - sp.x)
    print(f"rosenbrock: |x - scipy x| {err:.3e} bar {bar:.3e} (lambda_min {lam_min:.3e}); nfev "
          f"{out['nfev']} scipy {sp.nfev}")
    assert np.linalg.norm(sp.x - 1.0) <= bar and err <= 2.0 * bar
    # Powell's singular function
    out = run_both(lib, lambda k, x: fgh(powell, x), X0["powell"], ftol=0.0, pgtol=pgtol)[1]
    sp = least_squares(lambda x: powell(x)[0], X0["powell"], jac=lambda x: powell(x)[1],
                       method="lm", xtol=1e-14, ftol=1e-14, gtol=pgtol)
    bar = 3.0 * pgtol ** (1.0 / 3.0)
    print(f"powell: |x| {np.linalg.norm(out['x']):.3e} scipy |x| {np.linalg.norm(sp.x):.3e} bar "
          f"{bar:.3e}; nfev {out['nfev']} scipy {sp.nfev}")
    assert np.linalg.norm(out["x"]) <= bar and np.linalg.norm(sp.x) <= bar
