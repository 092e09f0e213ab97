"""GPU tests of the batched multi-market calibration (dh_surface_loss_rows,
dh_calibrate_lbfgs_batch, dhcos.calibrate_batch).

Markets: generate_synthetic_calibrations(35, as_arrays=True) under np.random.seed(11) -- the
generator's 15-option grid (strikes in percent of each market's own spot), N = 128, a different
spot per market.  Two starts per market: the reference's robust literature guess (guess 0) and a
warm start (the market's true parameters x (1 + 5% noise), what an FFN would hand over).

What is asserted:
  1. the per-row reduction alone equals, bit for bit, the NumPy restatement of its documented
     order (lane l adds options l, l + 64, ... from 0.0; xor butterfly 1, 2, 4, 8, 16, 32) on the
     prices it returns, for M = 15 and M = 70 (a lane takes two options), with a zero and a NaN
     market price and a set of NaN prices; a set's sse does not depend on its place in the request.
     NaNs are compared as NaNs (the sign and payload of a generated NaN are the hardware's);
  2. every traced request (market, x, f, g) of a 5-market run is the reference's objective there
     (test_gpu_shadow.shadow, its bounds, device_transform=True);
  3. every start's trace replays bit for bit on the CPU build of the state machine;
  4. a market's per-start results do not depend on the batch: one market, five, 35 in reversed
     order (live lists of <= 4, <= 64 and > 64 starts, with compaction), chunk sizes 1, 3, 8; a
     market with a NaN price ends ABNORMAL at nit 0 after 21 requests and moves no bit elsewhere;
  5. against the single-market device driver: the first request's f of every start is
     compute_loss(x0) to 1e-9 relative, and the robust start ends in kind as there.
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

N = 128
NB = 35
MAXFUN = 1071


@pytest.fixture(scope="module")
def dh():
    import dhcos
    from dhcos import _native
    if _native.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return dhcos


@pytest.fixture(scope="module")
def markets(dh):
    """35 generator markets and their [35, 2, 13] starts (robust guess 0, warm start)."""
    from dhcos import _native
    from dhcos.generator import MATURITIES, STRIKES_PCT, grid_surface
    np.random.seed(11)
    g = dh.generate_synthetic_calibrations(NB, None, as_arrays=True, verbose=False)
    mkt = np.ascontiguousarray(g["market_prices"], dtype=np.float64)
    spots = np.ascontiguousarray(g["spot"], dtype=np.float64)
    assert mkt.shape == (NB, 15) and len(set(spots.tolist())) == NB
    r = float(g["risk_free"])
    surf, krel, T = grid_surface(_native.default_context(), STRIKES_PCT, MATURITIES)
    cal = dh.DoubleHestonJumpCalibrator(100.0, r, [])
    rs = np.random.RandomState(5)
    X = np.empty((NB, 2, 13))
    for b in range(NB):
        X[b, 0] = cal.get_initial_guess(0)
        true = dict(zip(cal.param_names, g["params"][b] * (1 + 0.05 * rs.randn(13))))
        X[b, 1] = cal.inverse_transform_params(true)
    return dict(mkt=mkt, spots=spots, r=r, rates=np.full(NB, r), surf=surf, krel=krel, T=T, X=X)


def options_of(m, b):
    return [{"strike": float(k * m["spots"][b] / 100.0), "maturity": float(t),
             "price": float(p), "option_type": "call"}
            for k, t, p in zip(m["krel"], m["T"], m["mkt"][b])]


def run(m, sel, maxiter, chunk=8, starts=(0, 1), mkt=None):
    """The batch driver on the markets `sel` (in that order) -> {market: [LbResult per start]}."""
    sel = list(sel)
    mk = (m["mkt"] if mkt is None else mkt)[sel]
    X = m["X"][sel][:, list(starts)]
    S = X.shape[1]
    mof = np.repeat(np.arange(len(sel), dtype=np.int32), S)
    res, _ = m["surf"].calibrate_lbfgs_batch(mk, m["spots"][sel], m["rates"][sel],
                                            X.reshape(-1, 13), mof, N, maxiter=maxiter,
                                            maxfun=MAXFUN, chunk=chunk)
    return {b: res[i * S:(i + 1) * S] for i, b in enumerate(sel)}


def same_start(a, b):
    return (np.array_equal(np.array(a.x[:]), np.array(b.x[:]), equal_nan=True)
            and (a.fun == b.fun or (a.fun != a.fun and b.fun != b.fun))
            and (a.nit, a.nfev, a.task, a.n_calls) == (b.nit, b.nfev, b.task, b.n_calls)
            and a.best_loss == b.best_loss)


# ---- 1. the reduction alone ------------------------------------------------------------------

def rows_reference(prices, mkt, row):
    """dh_loss_rows.h's documented order, restated: -> (sse [S], n_bad [S])."""
    S, M = prices.shape
    sse, bad = np.empty(S), np.empty(S, dtype=np.int32)
    lane = np.arange(64)
    with np.errstate(all="ignore"):
        for s in range(S):
            m = mkt[row[s]]
            rel = (prices[s] - m) / m
            term = rel * rel
            acc = np.zeros(64)
            for j in range(0, M, 64):
                n = min(64, M - j)
                acc[:n] = acc[:n] + term[j:j + n]
            for off in (1, 2, 4, 8, 16, 32):
                acc = acc + acc[lane ^ off]
            sse[s] = acc[0]
            p = prices[s]
            bad[s] = np.count_nonzero(np.isnan(p) | np.isinf(p) | (p <= 0))
    return sse, bad


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64))


@pytest.mark.parametrize("grid", ["pct15", "abs70"])
def test_rows_reduction_bitwise(dh, grid):
    from dhcos import _native
    from dhcos.generator import MATURITIES, STRIKES_PCT, grid_surface
    ctx = _native.default_context()
    if grid == "pct15":
        surf = grid_surface(ctx, STRIKES_PCT, MATURITIES)[0]
    else:
        k = np.array([85.0, 90.0, 95.0, 100.0, 105.0, 110.0, 115.0])
        t = np.linspace(0.2, 2.0, 10)
        surf = _native.Surface(ctx, np.tile(k, t.size), np.repeat(t, k.size),
                               np.ones(70, dtype=np.int8), strike_mode=_native.STRIKE_ABSOLUTE)
    M = surf.M
    assert M == (15 if grid == "pct15" else 70)
    rs = np.random.RandomState(2)
    lo = np.array([0.025, 1.5, 0.025, 0.2, -0.85, 0.02, 0.3, 0.025, 0.1, -0.7, 0.05, -0.08, 0.03])
    hi = np.array([0.08, 4.5, 0.065, 0.5, -0.4, 0.07, 1.2, 0.07, 0.35, -0.2, 0.25, -0.01, 0.12])
    S, B = 7, 3
    spots = np.array([96.0, 100.0, 104.5])
    row = np.array([0, 1, 2, 0, 1, 2, 1], dtype=np.int32)
    rec = np.zeros((S, 16))
    rec[:, :13] = lo + (hi - lo) * rs.rand(S, 13)
    rec[:, 13], rec[:, 14] = spots[row], 0.03
    rec[5, 0] = np.exp(40.0)                           # v0 = e^40: NaN prices, n_bad = M
    base = np.zeros((B, 16))
    base[:, :13] = lo + (hi - lo) * rs.rand(B, 13)
    base[:, 13], base[:, 14] = spots, 0.03
    mkt = surf.price(base, N) * (1 + 0.02 * rs.randn(B, M))
    mkt[1, 3] = 0.0
    mkt[2, M - 2] = np.nan
    sse, bad, prices = surf.loss_terms_rows(rec, mkt, row, N, want_prices=True)
    assert same_bits(prices, surf.price(rec, N))       # priced as dh_surface_price prices
    want_sse, want_bad = rows_reference(prices, mkt, row)
    assert same_bits(sse, want_sse), (sse, want_sse)
    assert np.array_equal(bad, want_bad) and bad[5] == M and np.all(np.delete(bad, 5) == 0)
    assert np.isinf(sse[1]) and np.isnan(sse[2]) and np.isfinite(sse[0]) and np.isfinite(sse[3])
    # any place in any request: permuted, and set 3 once more at the end
    perm = np.array([4, 6, 0, 3, 5, 2, 1, 3])
    sse_p, bad_p, _ = surf.loss_terms_rows(rec[perm], mkt, row[perm], N)
    assert same_bits(sse_p, sse[perm]) and np.array_equal(bad_p, bad[perm])
    with pytest.raises(_native.NativeError):
        surf.loss_terms_rows(rec, mkt, np.full(S, B, dtype=np.int32), N)


# ---- 2, 3, 5a. one traced run of 5 markets x 2 starts ------------------------------------------

@pytest.fixture(scope="module")
def traced(markets):
    m = markets
    ctx = m["surf"].ctx
    ctx.set_lb_trace(100000)
    try:
        res = run(m, range(5), 25)
        tr = ctx.read_lb_trace()
    finally:
        ctx.set_lb_trace(0)
    assert len(tr) == sum(q.n_calls for b in res for q in res[b]) // 14
    assert np.array_equal(tr[:, 29], tr[:, 0] // 2)    # the spare double holds the market
    return res, tr


@pytest.mark.parametrize("b", range(5))
def test_requests_are_the_reference_objective(markets, traced, b):
    from test_gpu_shadow import shadow
    m = markets
    _, tr = traced
    rows = tr[tr[:, 29] == b]
    trace = [(int(q[0]), int(q[1]), q[3:16].copy(), float(q[2]), q[16:29].copy()) for q in rows]
    trace.sort(key=lambda t: (t[0], t[1]))
    assert {t[0] for t in trace} == {2 * b, 2 * b + 1}
    for s in (0, 1):
        first = next(t for t in trace if t[0] == 2 * b + s and t[1] == 0)
        assert np.array_equal(first[2], m["X"][b, s])
    K = m["krel"] * m["spots"][b] / 100.0
    shadow(trace, m["surf"], K, m["T"], np.ones(15, dtype=bool), m["mkt"][b],
           float(m["spots"][b]), m["r"], N, f"batch market {b}", device_transform=True)


def test_batch_replays_bitwise_on_cpu_build(markets, traced):
    import test_lbfgs_device_algo as T
    lib = C.CDLL(os.path.join(ROOT, "tests", "native", "liblbhost.so"))
    lib.lbh_begin.argtypes = [C.c_void_p, T._D]
    lib.lbh_point.argtypes = [C.c_void_p, T._D]
    lib.lbh_set_fg.argtypes = [C.c_void_p, C.c_double, T._D]
    lib.lbh_resume.argtypes = [C.c_void_p] + [C.c_int] * 3 + [C.c_double] * 2
    lib.lbh_result.argtypes = [C.c_void_p, T._D, T._D, C.POINTER(C.c_int)]
    res, tr = traced
    eps = np.finfo(float).eps
    for b in range(5):
        for s in (0, 1):
            q = res[b][s]
            rows = tr[tr[:, 0] == 2 * b + s]
            rows = rows[np.argsort(rows[:, 1])]
            assert np.array_equal(rows[:, 1], np.arange(len(rows)))
            st = C.create_string_buffer(lib.lbh_state_size())
            x0 = np.ascontiguousarray(markets["X"][b, s])
            more = lib.lbh_begin(st, x0.ctypes.data_as(T._D))
            xe = np.empty(13)
            k = 0
            while more:
                lib.lbh_point(st, xe.ctypes.data_as(T._D))
                assert np.array_equal(xe, rows[k, 3:16]), (b, s, k)
                g = np.ascontiguousarray(rows[k, 16:29])
                lib.lbh_set_fg(st, rows[k, 2], g.ctypes.data_as(T._D))
                more = lib.lbh_resume(st, 25, MAXFUN, 20, (1e-9 / eps) * eps, 1e-6)
                k += 1
            assert k == len(rows) == q.nfev
            x = np.empty(13)
            fv = C.c_double()
            info = (C.c_int * 4)()
            lib.lbh_result(st, x.ctypes.data_as(T._D), C.byref(fv), info)
            assert np.array_equal(x, np.array(q.x[:])) and fv.value == q.fun
            assert list(info) == [q.nit, q.nfev, q.task, q.warnflag]


def test_first_request_is_compute_loss(dh, markets, traced):
    m = markets
    _, tr = traced
    for b in range(5):
        cal = dh.DoubleHestonJumpCalibrator(float(m["spots"][b]), m["r"], options_of(m, b), N=N)
        for s in (0, 1):
            f, = tr[(tr[:, 0] == 2 * b + s) & (tr[:, 1] == 0), 2]
            want = cal.compute_loss(m["X"][b, s])
            print(f"market {b} start {s}: first f {f:.16e} compute_loss {want:.16e}")
            assert abs(f - want) <= 1e-9 * abs(want), (b, s, f, want)


# ---- 4. batch invariance ------------------------------------------------------------------------

def test_batch_invariance_bitwise(markets):
    m = markets
    ref = run(m, range(5), 5, chunk=8)                          # 10 live starts: inline list
    nfevs = {q.nfev for b in ref for q in ref[b]}
    print("nfev over the 10 starts:", sorted(nfevs))
    assert len(nfevs) > 1                                       # starts end apart: compaction
    for chunk in (1, 3):
        got = run(m, range(5), 5, chunk=chunk)
        assert all(same_start(a, c) for b in ref for a, c in zip(got[b], ref[b])), chunk
    for b in (0, 3):                                            # 2 live starts: preloaded list
        alone = run(m, [b], 5, chunk=8)
        assert all(same_start(a, c) for a, c in zip(alone[b], ref[b])), b
    big = run(m, reversed(range(NB)), 5, chunk=3)               # 70 live starts: list in memory
    for b in range(5):
        assert all(same_start(a, c) for a, c in zip(big[b], ref[b])), b
    big8 = run(m, range(NB), 5, chunk=8)
    for b in range(NB):
        assert all(same_start(a, c) for a, c in zip(big8[b], big[b])), b


def test_nan_market_ends_abnormal_and_moves_no_other_bit(dh, markets):
    from dhcos.calibrator import run_starts_device
    m = markets
    ref = run(m, range(5), 5)
    mkt = m["mkt"].copy()
    mkt[2, 7] = np.nan
    got = run(m, range(5), 5, mkt=mkt)
    for b in (0, 1, 3, 4):
        assert all(same_start(a, c) for a, c in zip(got[b], ref[b])), b
    opts = options_of(m, 2)
    opts[7]["price"] = float("nan")
    for s in (0, 1):
        q = got[2][s]
        cal = dh.DoubleHestonJumpCalibrator(float(m["spots"][2]), m["r"], opts, N=N)
        (one, _), = run_starts_device(cal, [m["X"][2, s]], 5)
        assert (q.nit, q.nfev, q.task) == (0, 21, 8000)
        assert (one.nit, one.nfev, one.message) == (0, 21, "ABNORMAL: ")
        assert np.array_equal(np.array(q.x[:]), m["X"][2, s])


# ---- 5b. the robust start, in kind as the single-market driver ----------------------------------

def test_robust_start_ends_as_single_market_driver(dh, markets):
    from dhcos.batch import task_message
    from dhcos.calibrator import run_starts_device
    m = markets
    got = run(m, range(5), 300, starts=(0,))
    for b in range(5):
        cal = dh.DoubleHestonJumpCalibrator(float(m["spots"][b]), m["r"], options_of(m, b), N=N)
        (one, _), = run_starts_device(cal, [m["X"][b, 0]], 300)
        q = got[b][0]
        print(f"market {b}: batch nit {q.nit} nfev {q.nfev} {task_message(q.task)!r}; "
              f"single nit {one.nit} nfev {one.nfev} {one.message!r}")
        assert (q.nit, q.nfev, task_message(q.task)) == (one.nit, one.nfev, one.message)


# ---- the public API ------------------------------------------------------------------------------

def test_calibrate_batch_api(dh, markets):
    m = markets
    B = 4
    res = dh.calibrate_batch(m["mkt"][:B], m["spots"][:B], m["r"], x0s=m["X"][:B], maxiter=5)
    direct = run(m, range(B), 5)
    for b in range(B):
        funs = [q.fun for q in direct[b]]
        assert np.array_equal(res.fun[b], funs)
        w = int(res.best_start[b])
        assert w == int(np.argmin(funs)) and res.final_loss[b] == funs[w]
        assert np.array_equal(res.x[b], np.array(direct[b][w].x[:]))
        one = res.result(b)
        assert one.spot == m["spots"][b] and one.final_loss == funs[w]
        assert one.iterations == direct[b][w].nit and len(one.market_options) == 15
        rec = np.zeros((1, 16))
        rec[0, :13], rec[0, 13], rec[0, 14] = res.parameters[b], m["spots"][b], m["r"]
        assert np.array_equal(res.model_prices[b], m["surf"].price(rec, N)[0])
    # a market whose every start fails (NaN prices: fun NaN or 1e10 ... here all NaN) and dicts
    mkt = m["mkt"][:2].copy()
    mkt[1] = np.nan
    names = dh.DoubleHestonJumpCalibrator(100.0, 0.03, []).param_names
    from dhcos.calibrator import x_to_model
    dicts = [[dict(zip(names, x_to_model(m["X"][b, s]))) for s in (1,)] for b in range(2)]
    res = dh.calibrate_batch(mkt, m["spots"][:2], np.full(2, m["r"]), x0s=dicts, maxiter=3)
    assert res.best_start[0] == 0 and np.isfinite(res.final_loss[0])
    if res.best_start[1] < 0:
        bad = res.result(1)
        assert bad.message == "All optimization starts failed" and not bad.success
        assert bad.final_loss == np.inf and not np.any(bad.model_prices)
        assert all(v == 0.0 for v in bad.parameters.values()) and bad.iterations == 0
    else:                                   # the last trial's loss was 1e10: it wins, as there
        assert res.final_loss[1] == 1e10
