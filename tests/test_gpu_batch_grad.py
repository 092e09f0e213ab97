"""GPU tests of the analytic-gradient batch calibration (dh_surface_loss_grad_rows*,
dh_calibrate_lbfgs_batch_grad, dhcos.calibrate_batch(gradient="analytic")).

  1. the rows reduction against the NumPy restatement (tests/batch_grad_reference.py) by
     tests/test_gpu_param_grad.py's loss_grad bars -- f to 1e-9 relative, g to 1e-6 |g| + 1e-10
     max |g| -- on the 15-option generator grid and a 70-option one (a lane adds two options), with
     an invalid set; a set's bits do not depend on the call; B = 1 gives Surface.loss_grad's bits;
  2. a market's starts do not depend on the batch, the order of the markets or the chunk size;
  3. every traced request (x, f, g) of a run on the golden market is the restatement at the traced
     x, and the points asked for are the state machine's: bit for bit on its CPU build
     (tests/native/liblbhost.so, tests/test_gpu_device_lbfgs.py's replay and bar) fed the device's
     own (f, g), and SciPy's own setulb (dhcos.calibrator.lbfgsb_steps) fed the same;
  4. the start converges where the FD batch driver does; the start on the Feller kink terminates;
  5. calibrate_batch(gradient="analytic") on three generator markets.

SciPy's replay in 3: setulb takes the subspace step in L-BFGS-B's compact form, the device in the
two-loop recursion -- the same matrix, not the same roundings (tests/test_lbfgs_device_algo.py:
"agreement is in algorithm, not in bits").  Fed the device's (f, g) request by request, setulb must
ask for as many points, and each within that file's bar for a smooth problem, 1e-9 in x; the
bit-for-bit bar is held by the CPU build of the device's own state machine."""
import ctypes as C
import os

import numpy as np
import pytest

import batch_grad_reference as BR
import param_grad_reference as R
from conftest import ROOT
from oracle import dh_oracle as O

pytestmark = pytest.mark.gpu

LO = np.array([0.025, 1.5, 0.025, 0.2, -0.85, 0.02, 0.3, 0.025, 0.1, -0.7, 0.05, -0.08, 0.03])
HI = np.array([0.08, 4.5, 0.065, 0.5, -0.4, 0.07, 1.2, 0.07, 0.35, -0.2, 0.25, -0.01, 0.12])
MAXFUN = 1071
CONVERGED = (4401, 4402)                       # CONVERGENCE: pgtol, factr
TERMINAL = CONVERGED + (5502, 5504, 8000)      # and the maxfun / maxiter stops, ABNORMAL


@pytest.fixture(scope="module")
def native():
    from dhcos import _native
    if _native.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return _native


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_fg(f, g, want_f, want_g, label):
    """tests/test_gpu_param_grad.py's bars for loss_grad."""
    tol = 1e-6 * np.abs(want_g) + 1e-10 * np.max(np.abs(want_g))
    err = np.abs(g - want_g)
    print(f"{label}: f {f:.12e} ref {want_f:.12e} rel {abs(f - want_f) / abs(want_f):.2e}; "
          f"g worst err / bar {np.max(err / tol):.3e}")
    assert abs(f - want_f) <= 1e-9 * abs(want_f), (label, f, want_f)
    assert np.all(err <= tol), (label, [O.PARAM_NAMES[i] for i in np.flatnonzero(err > tol)])


def golden_market(calib_golden):
    market = calib_golden["test_market"]
    K = np.array([o["strike"] for o in market], dtype=np.float64)
    T = np.array([o["maturity"] for o in market], dtype=np.float64)
    mkt = np.array([o["price"] for o in market], dtype=np.float64)
    return market, K, T, mkt


# ---- 1. the reduction stage --------------------------------------------------------------------

@pytest.mark.parametrize("grid", ["pct15", "abs70"])
def test_rows_reduction_matches_the_restatement(native, grid):
    import torch
    from dhcos.generator import MATURITIES, STRIKES_PCT
    ctx = native.default_context()
    if grid == "pct15":
        k = np.asarray(STRIKES_PCT, dtype=np.float64)
        t = np.asarray(MATURITIES, dtype=np.float64)
        mode = native.STRIKE_PCT_SPOT
    else:
        k = np.array([85.0, 90.0, 95.0, 100.0, 105.0, 110.0, 115.0])
        t = np.linspace(0.2, 2.0, 10)
        mode = native.STRIKE_ABSOLUTE
    Kg, Tg = np.tile(k, t.size), np.repeat(t, k.size)
    M, N = Kg.size, 64
    assert M == (15 if grid == "pct15" else 70)
    call = np.ones(M, dtype=bool)
    rs = np.random.RandomState(4)
    S, B = 6, 3
    spots = np.array([96.0, 100.0, 104.5])
    rates = np.array([0.02, 0.03, 0.045])
    row = np.array([0, 1, 2, 2, 1, 0], dtype=np.int32)
    X = np.array([O.from_params(LO + (HI - LO) * rs.rand(13)) for _ in range(S)])
    X[4] = 5.0                                          # NaN prices: an invalid set
    base = np.zeros((B, 16))
    base[:, :13] = LO + (HI - LO) * rs.rand(B, 13)
    base[:, 13], base[:, 14] = spots, rates
    surf = native.Surface(ctx, Kg, Tg, call, strike_mode=mode)        # no market of its own
    own = None
    try:
        mkt = surf.price(base, N) * (1 + 0.02 * rs.randn(B, M))
        f, g, bad = surf.loss_grad_rows(X, mkt, spots, rates, row, N)
        # any place in any call, any S and B: permuted with set 2 twice, and set 3 alone against
        # its market as the only row
        perm = np.array([3, 5, 0, 2, 4, 1, 2])
        fp, gp, bp = surf.loss_grad_rows(X[perm], mkt, spots, rates, row[perm], N)
        f1, g1, b1 = surf.loss_grad_rows(X[3:4], mkt[2:3], spots[2:3], rates[2:3], [0], N)
        with pytest.raises(native.NativeError):
            surf.loss_grad_rows(X, mkt, spots, rates, np.full(S, B, dtype=np.int32), N)
        with pytest.raises(native.NativeError):
            surf.loss_grad_rows(X, mkt, spots, rates, np.full(S, -1, dtype=np.int32), N)
        # the device-pointer form: the same bits
        dev = torch.device("cuda", ctx.device)
        d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (X, mkt, spots, rates, row)]
        d_f = torch.empty(S, dtype=torch.float64, device=dev)
        d_g = torch.empty((S, 13), dtype=torch.float64, device=dev)
        d_bad = torch.empty(S, dtype=torch.int32, device=dev)
        stream = torch.cuda.Stream(device=dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream):
            surf.loss_grad_rows_dev(*(a.data_ptr() for a in d), S, d_f.data_ptr(), d_g.data_ptr(),
                                    d_bad.data_ptr(), N=N, stream=stream.cuda_stream)
        stream.synchronize()
        # B = 1 and the surface's own market: Surface.loss_grad's bits
        own = native.Surface(ctx, Kg, Tg, call, mkt[1], strike_mode=mode)
        want_own = own.loss_grad(X, spots[1], rates[1], N)
        got_own = surf.loss_grad_rows(X, mkt[1:2], spots[1:2], rates[1:2], np.zeros(S, np.int32), N)
    finally:
        surf.close()
        if own is not None:
            own.close()
    assert np.array_equal(bad, [0, 0, 0, 0, M, 0])
    assert f[4] == 1e10 and not g[4].any() and np.signbit(g[4]).sum() == 0
    assert same_bits(fp, f[perm]) and same_bits(gp, g[perm]) and np.array_equal(bp, bad[perm])
    assert f1[0] == f[3] and same_bits(g1[0], g[3]) and b1[0] == 0
    assert same_bits(d_f.cpu().numpy(), f) and same_bits(d_g.cpu().numpy(), g)
    assert np.array_equal(d_bad.cpu().numpy(), bad)
    assert same_bits(got_own[0], want_own[0]) and same_bits(got_own[1], want_own[1])
    assert np.array_equal(got_own[2], want_own[2]) and want_own[2][4] == M
    # the restatement, each set under its own market, spot and rate
    markets = [BR.market_of_row(Kg * spots[b] / 100.0 if mode == native.STRIKE_PCT_SPOT else Kg,
                                Tg, call, mkt[b]) for b in range(B)]
    want_f, want_g = BR.loss_grad_rows(X, markets, spots, rates, row, N)
    assert want_f[4] == 1e10 and not want_g[4].any()
    for s in (0, 1, 2, 3, 5):
        p = O.to_params(X[s])                           # no set within rounding of the Feller kink
        assert min(abs(p[3] ** 2 - 2 * p[1] * p[2]), abs(p[8] ** 2 - 2 * p[6] * p[7])) > 1e-6
        assert_fg(f[s], g[s], want_f[s], want_g[s], f"{grid} set {s} market {row[s]}")
    assert len({f[0], f[5]}) == 2 and f[1] != f[4]      # the rows matter


# ---- 2. isolation -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def markets(native):
    """Five generator markets and two warm starts each (the true parameters under 5% noise)."""
    import dhcos
    from dhcos.generator import MATURITIES, STRIKES_PCT, grid_surface
    np.random.seed(11)
    g = dhcos.generate_synthetic_calibrations(5, None, as_arrays=True, verbose=False)
    mkt = np.ascontiguousarray(g["market_prices"], dtype=np.float64)
    spots = np.ascontiguousarray(g["spot"], dtype=np.float64)
    surf = grid_surface(native.default_context(), STRIKES_PCT, MATURITIES)[0]
    cal = dhcos.DoubleHestonJumpCalibrator(100.0, float(g["risk_free"]), [])
    rs = np.random.RandomState(5)
    X = np.empty((5, 2, 13))
    for b in range(5):
        for s in range(2):
            true = dict(zip(cal.param_names, g["params"][b] * (1 + 0.05 * rs.randn(13))))
            X[b, s] = cal.inverse_transform_params(true)
    return dict(mkt=mkt, spots=spots, rates=np.full(5, float(g["risk_free"])), surf=surf, X=X)


def run(m, sel, starts, maxiter, chunk=8, N=128):
    """The analytic batch driver on markets `sel` with the starts `starts` of each
    -> {market: [LbResult per start]}."""
    sel = list(sel)
    X = m["X"][sel][:, list(starts)]
    S = X.shape[1]
    mof = np.repeat(np.arange(len(sel), dtype=np.int32), S)
    res, _ = m["surf"].calibrate_lbfgs_batch_grad(m["mkt"][sel], m["spots"][sel], m["rates"][sel],
                                                  X.reshape(-1, 13), mof, N, maxiter=maxiter,
                                                  maxfun=MAXFUN, chunk=chunk)
    return {b: res[i * S:(i + 1) * S] for i, b in enumerate(sel)}


def same_start(a, b):
    return (np.array_equal(np.array(a.x[:]), np.array(b.x[:])) and a.fun == b.fun
            and (a.nit, a.nfev, a.task, a.n_calls) == (b.nit, b.nfev, b.task, b.n_calls)
            and a.best_loss == b.best_loss)


def test_a_market_does_not_depend_on_the_batch(markets):
    m = markets
    alone = run(m, [1], (0,), 40)[1][0]
    print(f"market 1 alone: nit {alone.nit} nfev {alone.nfev} task {alone.task} fun {alone.fun:.6e}")
    assert alone.nfev == alone.n_calls > alone.nit > 1 and np.isfinite(alone.fun)
    nfevs = set()
    for chunk in (1, 8):
        # five markets permuted, two starts each: start 0 of market 1 among nine others
        got = run(m, [4, 2, 1, 0, 3], (0, 1), 40, chunk=chunk)
        assert same_start(got[1][0], alone), chunk
        nfevs |= {q.nfev for b in got for q in got[b]}
        again = run(m, [4, 2, 1, 0, 3], (0, 1), 40, chunk=chunk)
        assert all(same_start(a, c) for b in got for a, c in zip(got[b], again[b])), chunk
    three = run(m, [0, 1, 2], (0,), 40)                 # market 1 of 3
    assert same_start(three[1][0], alone)
    print("nfev over the ten starts:", sorted(nfevs))
    assert len(nfevs) > 1                               # starts end apart: compaction ran


# ---- 3. every request shadowed ------------------------------------------------------------------

def lbhost():
    lib = C.CDLL(os.path.join(ROOT, "tests", "native", "liblbhost.so"))
    D = C.POINTER(C.c_double)
    lib.lbh_begin.argtypes = [C.c_void_p, D]
    lib.lbh_point.argtypes = [C.c_void_p, D]
    lib.lbh_set_fg.argtypes = [C.c_void_p, C.c_double, D]
    lib.lbh_resume.argtypes = [C.c_void_p] + [C.c_int] * 3 + [C.c_double] * 2
    lib.lbh_result.argtypes = [C.c_void_p, D, D, C.POINTER(C.c_int)]
    return lib, D


def golden_run(native, calib_golden, start, maxiter, trace=False, gradient="analytic"):
    market, K, T, mkt = golden_market(calib_golden)
    ctx = native.default_context()
    surf = native.Surface(ctx, K, T, np.ones(15, bool))               # no market of its own
    x0 = np.array(calib_golden["guesses_seed0"][start], dtype=np.float64)
    drive = (surf.calibrate_lbfgs_batch_grad if gradient == "analytic"
             else surf.calibrate_lbfgs_batch)
    tr = None
    try:
        if trace:
            ctx.set_lb_trace(4096)
        (res,), _ = drive(mkt[None, :], [100.0], [0.05], x0[None, :], [0], 128, maxiter=maxiter,
                          maxfun=MAXFUN)
        if trace:
            tr = ctx.read_lb_trace()
        f0 = surf.loss_grad_rows(x0[None, :], mkt[None, :], [100.0], [0.05], [0], 128)[0][0]
    finally:
        ctx.set_lb_trace(0)
        surf.close()
    return res, tr, x0, f0


def test_every_request_is_the_restatement_and_the_state_machines_point(native, calib_golden):
    from dhcos.calibrator import lbfgsb_steps
    market = calib_golden["test_market"]
    p0 = O.to_params(np.array(calib_golden["guesses_seed0"][1]))
    slack = [p0[3] ** 2 - 2 * p0[1] * p0[2], p0[8] ** 2 - 2 * p0[6] * p0[7]]
    assert (slack[0] > 1e-3) != (slack[1] > 1e-3) and min(slack) < -1e-3      # off the kink
    maxiter = 40
    res, tr, x0, _ = golden_run(native, calib_golden, 1, maxiter, trace=True)
    assert res.n_calls == res.nfev == len(tr)
    assert np.all(tr[:, 0] == 0) and np.all(tr[:, 29] == 0)          # start 0, market 0
    rows = tr[np.argsort(tr[:, 1])]
    assert np.array_equal(rows[:, 1], np.arange(len(rows)))
    assert np.array_equal(rows[0, 3:16], x0)
    print(f"{len(rows)} requests, nit {res.nit}, task {res.task}, fun {res.fun:.6e}")
    # each traced (x, f, g) against the restatement at the traced x
    for k, q in enumerate(rows):
        want_f, want_g = R.loss_grad(q[3:16], market, 100.0, 0.05, 128)
        assert_fg(q[2], q[16:29], want_f, want_g, f"request {k}")
    # the device's state machine on the CPU: the same points bit for bit, the same end
    lib, D = lbhost()
    eps = np.finfo(float).eps
    st = C.create_string_buffer(lib.lbh_state_size())
    more = lib.lbh_begin(st, np.ascontiguousarray(x0).ctypes.data_as(D))
    xe = np.empty(13)
    k = 0
    while more:
        lib.lbh_point(st, xe.ctypes.data_as(D))
        assert np.array_equal(xe, rows[k, 3:16]), k
        g = np.ascontiguousarray(rows[k, 16:29])
        lib.lbh_set_fg(st, rows[k, 2], g.ctypes.data_as(D))
        more = lib.lbh_resume(st, maxiter, MAXFUN, 20, (1e-9 / eps) * eps, 1e-6)
        k += 1
    assert k == len(rows) == res.nfev
    x = np.empty(13)
    fv = C.c_double()
    info = (C.c_int * 4)()
    lib.lbh_result(st, x.ctypes.data_as(D), C.byref(fv), info)
    assert np.array_equal(x, np.array(res.x[:])) and fv.value == res.fun
    assert list(info) == [res.nit, res.nfev, res.task, res.warnflag]
    # SciPy's setulb fed the same (f, g): as many points, each within 1e-9 of the device's
    gen = lbfgsb_steps(x0, maxiter, MAXFUN)
    pt = next(gen)
    worst, k = 0.0, 0
    try:
        while True:
            assert k < len(rows), "setulb asks for more points than the device evaluated"
            worst = max(worst, float(np.max(np.abs(pt - rows[k, 3:16]))))
            pt = gen.send((float(rows[k, 2]), rows[k, 16:29].copy()))
            k += 1
    except StopIteration as stop:
        out = stop.value
        k += 1
    print(f"setulb replay: {k} points, worst |x - device x| {worst:.3e}, nit {out.nit} "
          f"{out.message!r}")
    assert worst <= 1e-9
    assert (k, out.nit, out.nfev) == (len(rows), res.nit, res.nfev)


# ---- 4. convergence -----------------------------------------------------------------------------

def test_the_start_off_the_kink_converges_where_fd_does(native, calib_golden):
    """guesses_seed0[1], maxiter 300.  Trajectories are chaotic: neither x nor nit is
    compared.  The factor 10 is tests/test_gpu_param_grad.py's analytic-against-FD one."""
    from dhcos.batch import task_message
    an, _, _, f0 = golden_run(native, calib_golden, 1, 300)
    fd, _, _, _ = golden_run(native, calib_golden, 1, 300, gradient="fd")
    for name, q in (("analytic", an), ("fd", fd)):
        print(f"{name}: start loss {f0:.6e} final {q.fun:.6e} nit {q.nit} requests {q.nfev} "
              f"loss evaluations {q.n_calls} {task_message(q.task)!r}")
    assert an.n_calls == an.nfev and fd.n_calls == 14 * fd.nfev
    assert an.task in CONVERGED, task_message(an.task)
    assert np.isfinite(an.fun) and an.fun <= 10.0 * fd.fun


def test_the_start_on_the_kink_terminates(native, calib_golden):
    """guesses_seed0[0] sits on factor 2's Feller kink to an ulp: either one-sided derivative is
    within the contract there, so only the end is held."""
    from dhcos.batch import task_message
    res, _, x0, f0 = golden_run(native, calib_golden, 0, 300)
    print(f"kink start: start loss {f0:.6e} final {res.fun:.6e} best {res.best_loss:.6e} nit "
          f"{res.nit} requests {res.nfev} {task_message(res.task)!r}")
    assert res.task in TERMINAL, res.task
    assert res.n_calls == res.nfev >= 1
    assert np.isfinite(res.fun) and res.fun <= f0


# ---- 5. the public API --------------------------------------------------------------------------

def test_calibrate_batch_with_the_analytic_gradient(native):
    import dhcos
    from dhcos.generator import MATURITIES, STRIKES_PCT, grid_surface
    np.random.seed(23)
    g = dhcos.generate_synthetic_calibrations(3, None, as_arrays=True, verbose=False)
    mkt = np.ascontiguousarray(g["market_prices"], dtype=np.float64)
    spots = np.ascontiguousarray(g["spot"], dtype=np.float64)
    r = float(g["risk_free"])
    cal = dhcos.DoubleHestonJumpCalibrator(100.0, r, [])
    rs = np.random.RandomState(6)
    X = np.array([[cal.inverse_transform_params(
        dict(zip(cal.param_names, g["params"][b] * (1 + 0.05 * rs.randn(13)))))
        for _ in range(2)] for b in range(3)])
    res = dhcos.calibrate_batch(mkt, spots, r, x0s=X, maxiter=40, gradient="analytic")
    assert res.gradient == "analytic" and res.objective == "price"
    assert res.fun.shape == (3, 2) and np.all(res.best_start >= 0)
    assert np.array_equal(res.n_calls, res.nfev)
    assert res.loss_evals == int(res.nfev.sum()) > 0
    surf = grid_surface(native.default_context(), STRIKES_PCT, MATURITIES)[0]
    rec = np.zeros((3, 16))
    rec[:, :13], rec[:, 13], rec[:, 14] = res.parameters, spots, r
    prices = surf.price(rec, 128)
    assert np.array_equal(prices, res.model_prices)
    for b in range(3):
        want = np.mean(((prices[b] - mkt[b]) / mkt[b]) ** 2) + O.feller(res.parameters[b])
        print(f"market {b}: reported {res.final_loss[b]:.12e} repriced {want:.12e} rel "
              f"{abs(res.final_loss[b] - want) / want:.2e} nit {res.iterations[b]}")
        assert abs(res.final_loss[b] - want) <= 1e-9 * want
        assert res.final_loss[b] == res.fun[b, res.best_start[b]]
    fd = dhcos.calibrate_batch(mkt, spots, r, x0s=X, maxiter=3)
    assert fd.gradient == "fd" and fd.loss_evals == int(fd.n_calls.sum()) == 14 * int(fd.nfev.sum())
