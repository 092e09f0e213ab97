"""GPU tests of the batched multi-market calibration in implied-vol space
(csrc/dh_loss_rows.h: dh_surface_iv_sse_rows_dev, dh_surface_loss_iv_rows,
dh_calibrate_lbfgs_batch_iv; dhcos.calibrate_batch(objective="iv")).  DESIGN.md 3.13.

Markets: those of test_gpu_calibrate_batch.py -- generate_synthetic_calibrations(35,
as_arrays=True, implied_vols=True) under np.random.seed(11), the generator's 15-option grid, N =
128, two starts per market (guess 0 and a 5 % warm start).  Market vols are the generator's
``market_iv``; a noisy market price without a vol gets weight 0 (the path a user takes), every
other weight is 1.

What is asserted:
  1. the reduction alone equals, bit for bit, the NumPy restatement of its documented order (lane l
     takes the surface's sorted options l, l + 64, ... from 0.0; xor butterfly 1, 2, 4, 8, 16, 32)
     on the vols it returns, for M = 15, 64 and 70, S = 7 sets over B = 3 markets with different
     spots, with a set of NaN prices, a zero weight on a NaN market vol and, through the
     device-pointer entry, a price one ulp below its lower bound and an infinite one;
  2. for M = 15 and 64 it has the bits of dh_surface_set_iv_market + dh_surface_loss_iv;
  3. every traced request (market, x, f, g) of a 5-market run is the host-formed vol objective
     (DoubleHestonJumpCalibrator(objective="iv").compute_loss_and_grad) there: f to 1e-9
     relative, g to the derived bar of `grad_bar`;
  4. every start's trace replays bit for bit on the CPU build of the state machine;
  5. a market's per-start results do not depend on the batch (one market, five, 35 reversed; chunk
     1, 3, 8); a market whose loss is not finite ends ABNORMAL at nit 0 and moves no bit elsewhere;
     a zero-weight option in one market moves no bit elsewhere and equals that market run alone;
  6. a noise-free market is fitted below its start's loss, and model_ivs are the vols of
     model_prices;
  7. objective="price" gives the bits of a call without the argument;
  8. the public API against the native call, result(b), and the ValueError before any RNG draw.
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
N = 128
NB = 35
MAXFUN = 1071
IV_YARDSTICK = 5493.0     # the bar implied_vol is held to, in units of u


@pytest.fixture(scope="module")
def dh():
    import dhcos
    from dhcos import _native
    if _native.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return dhcos


@pytest.fixture(scope="module")
def markets(dh):
    """35 generator markets, their vols and weights and their [35, 2, 13] starts."""
    from dhcos import _native
    from dhcos.generator import MATURITIES, STRIKES_PCT, grid_surface
    np.random.seed(11)
    g = dh.generate_synthetic_calibrations(NB, None, as_arrays=True, verbose=False,
                                           implied_vols=True)
    mkt = np.ascontiguousarray(g["market_prices"], dtype=np.float64)
    spots = np.ascontiguousarray(g["spot"], dtype=np.float64)
    ivs = np.ascontiguousarray(g["market_iv"], dtype=np.float64)
    assert mkt.shape == ivs.shape == (NB, 15) and len(set(spots.tolist())) == NB
    wts = (np.isfinite(ivs) & (ivs >= 0)).astype(np.float64)
    assert np.all(wts.sum(axis=1) > 0)
    print(f"market vols: {int((wts == 0).sum())} of {wts.size} noisy prices have none (weight 0)")
    r = float(g["risk_free"])
    surf, krel, T = grid_surface(_native.default_context(), STRIKES_PCT, MATURITIES)
    cal = dh.DoubleHestonJumpCalibrator(100.0, r, [])
    rs = np.random.RandomState(5)
    X = np.empty((NB, 2, 13))
    for b in range(NB):
        X[b, 0] = cal.get_initial_guess(0)
        true = dict(zip(cal.param_names, g["params"][b] * (1 + 0.05 * rs.randn(13))))
        X[b, 1] = cal.inverse_transform_params(true)
    return dict(mkt=mkt, ivs=ivs, wts=wts, spots=spots, r=r, rates=np.full(NB, r), surf=surf,
                krel=krel, T=T, X=X)


def options_of(m, b):
    return [{"strike": float(k * m["spots"][b] / 100.0), "maturity": float(t),
             "price": float(p), "option_type": "call"}
            for k, t, p in zip(m["krel"], m["T"], m["mkt"][b])]


def run(m, sel, maxiter, chunk=8, starts=(0, 1), ivs=None, wts=None):
    """The vol-space batch driver on the markets `sel` (in that order)
    -> {market: [LbResult per start]}."""
    sel = list(sel)
    iv = (m["ivs"] if ivs is None else ivs)[sel]
    w = (m["wts"] if wts is None else wts)[sel]
    X = m["X"][sel][:, list(starts)]
    S = X.shape[1]
    mof = np.repeat(np.arange(len(sel), dtype=np.int32), S)
    res, _ = m["surf"].calibrate_lbfgs_batch_iv(iv, w, m["spots"][sel], m["rates"][sel],
                                               X.reshape(-1, 13), mof, N, maxiter=maxiter,
                                               maxfun=MAXFUN, chunk=chunk)
    return {b: res[i * S:(i + 1) * S] for i, b in enumerate(sel)}


def same_start(a, b):
    return (np.array_equal(np.array(a.x[:]), np.array(b.x[:]), equal_nan=True)
            and (a.fun == b.fun or (a.fun != a.fun and b.fun != b.fun))
            and (a.nit, a.nfev, a.task, a.n_calls) == (b.nit, b.nfev, b.task, b.n_calls)
            and a.best_loss == b.best_loss)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return (a.shape == b.shape and np.array_equal(na, nb)
            and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64)))


# ---- 1. the reduction alone ------------------------------------------------------------------

def iv_rows_reference(iv, mkt_iv, w, row, T):
    """dh_loss_rows.h's documented vol order, restated on the vols as used: the surface sorts its
    options by maturity (stable), lane l takes sorted options l, l + 64, ... -> (sse, n_bad)."""
    S, M = iv.shape
    perm = np.argsort(T, kind="stable")                  # sorted place -> caller's place
    sse, bad = np.empty(S), np.empty(S, dtype=np.int32)
    lane = np.arange(64)
    with np.errstate(all="ignore"):
        for s in range(S):
            b = row[s]
            acc = np.zeros(64)
            nb = 0
            for i in range(M):
                c = perm[i]
                ww = w[b, c]
                if ww > 0:
                    v = iv[s, c]
                    if v != v:
                        nb += 1
                    else:
                        d = v - mkt_iv[b, c]
                        acc[i % 64] = acc[i % 64] + ww * (d * d)
            for off in (1, 2, 4, 8, 16, 32):
                acc = acc + acc[lane ^ off]
            sse[s], bad[s] = acc[0], nb
    return sse, bad


LO = np.array([0.025, 1.5, 0.025, 0.2, -0.85, 0.02, 0.3, 0.025, 0.1, -0.7, 0.05, -0.08, 0.03])
HI = np.array([0.08, 4.5, 0.065, 0.5, -0.4, 0.07, 1.2, 0.07, 0.35, -0.2, 0.25, -0.01, 0.12])


def grid_of(name):
    """-> (K, T, is_call, strike mode): pct15 is the generator's grid; abs64 has unsorted
    maturities, so the surface's order is not the caller's; abs70 is test_gpu_calibrate_batch's."""
    from dhcos import _native
    from dhcos.generator import MATURITIES, STRIKES_PCT
    if name == "pct15":
        k, t = np.asarray(STRIKES_PCT, dtype=float), np.asarray(MATURITIES, dtype=float)
        mode = _native.STRIKE_PCT_SPOT
    elif name == "abs64":
        k = np.array([84.0, 88.0, 92.0, 97.0, 100.0, 104.0, 109.0, 114.0])
        t = np.array([1.0, 0.25, 0.75, 0.5, 2.0, 0.2, 1.5, 0.35])
        mode = _native.STRIKE_ABSOLUTE
    else:
        k = np.array([85.0, 90.0, 95.0, 100.0, 105.0, 110.0, 115.0])
        t = np.linspace(0.2, 2.0, 10)
        mode = _native.STRIKE_ABSOLUTE
    K, T = np.tile(k, t.size), np.repeat(t, k.size)
    call = np.ones(K.size, dtype=np.int8)
    if name == "abs64":
        call[K > 104.0] = 0                               # puts above, calls below
    return K, T, call, mode


def rows_case(surf, T):
    """S = 7 sets over B = 3 markets with different spots; r = 0, so that the discounted legs are
    the spot and the strike themselves and a lower bound is exact."""
    M = surf.M
    rs = np.random.RandomState(2)
    S, B = 7, 3
    spots = np.array([96.0, 100.0, 104.5])
    row = np.array([0, 1, 2, 0, 1, 2, 1], dtype=np.int32)
    rec = np.zeros((S, 16))
    rec[:, :13] = LO + (HI - LO) * rs.rand(S, 13)
    rec[:, 13], rec[:, 14] = spots[row], 0.0
    rec[5, 0] = np.exp(40.0)                           # v0 = e^40: NaN prices, every option bad
    base = np.zeros((B, 16))
    base[:, :13] = LO + (HI - LO) * rs.rand(B, 13)
    base[:, 13], base[:, 14] = spots, 0.0
    mkt_iv = surf.implied_vol(base, N) + rs.uniform(-0.02, 0.02, size=(B, M))
    assert np.all(np.isfinite(mkt_iv)) and np.all(mkt_iv > 0)
    w = rs.uniform(0.25, 4.0, size=(B, M))
    mkt_iv[2, M - 2] = np.nan                          # a NaN market vol under a zero weight
    w[2, M - 2] = 0.0
    w[0, 1] = 0.0
    return rec, row, spots, mkt_iv, w


@pytest.mark.parametrize("grid", ["pct15", "abs64", "abs70"])
def test_rows_reduction_bitwise(dh, grid):
    import torch
    from dhcos import _native
    ctx = _native.default_context()
    K, T, call, mode = grid_of(grid)
    surf = _native.Surface(ctx, K, T, call, strike_mode=mode)
    try:
        M = surf.M
        assert M == {"pct15": 15, "abs64": 64, "abs70": 70}[grid]
        rec, row, spots, mkt_iv, w = rows_case(surf, T)
        S, B = rec.shape[0], mkt_iv.shape[0]
        sse, bad, prices, iv = surf.loss_terms_iv_rows(rec, mkt_iv, row, N, weights=w,
                                                       want_prices=True, want_iv=True)
        assert same_bits(prices, surf.price(rec, N))   # priced as dh_surface_price prices
        want_sse, want_bad = iv_rows_reference(iv, mkt_iv, w, row, T)
        assert same_bits(sse, want_sse), (sse, want_sse)
        assert np.array_equal(bad, want_bad)
        # set 5: every call's price is NaN (a put's may come out finite through parity)
        dead = ~((prices[5] > 0) & np.isfinite(prices[5]))
        assert np.all(dead[call != 0]) and np.all(np.isnan(iv[5][dead]))
        assert bad[5] >= np.count_nonzero((w[row[5]] > 0) & dead) > 0
        assert np.all(np.delete(bad, 5) == 0)
        assert np.all(np.isfinite(np.delete(iv, 5, axis=0))) and np.all(np.delete(sse, 5) > 0)
        # the vols are dh_surface_implied_vol's (each set under its own spot), but for the clamp
        used = iv != 0.0
        assert np.all(used[np.arange(S) != 5])
        assert same_bits(iv[used], surf.implied_vol(rec, N)[used])
        sse2, bad2 = surf.loss_terms_iv_rows(rec, mkt_iv, row, N, weights=w)
        assert same_bits(sse2, sse) and np.array_equal(bad2, bad)
        # any place in any request: permuted, and set 3 once more at the end
        perm = np.array([4, 6, 0, 3, 5, 2, 1, 3])
        sse_p, bad_p = surf.loss_terms_iv_rows(rec[perm], mkt_iv, row[perm], N, weights=w)
        assert same_bits(sse_p, sse[perm]) and np.array_equal(bad_p, bad[perm])
        # weights None: all 1 (the NaN market vol then enters set 2's and 5's rows)
        one = mkt_iv.copy()
        one[2, M - 2] = 0.3
        sse_1, bad_1, iv_1 = surf.loss_terms_iv_rows(rec, one, row, N, want_iv=True)
        w1_sse, w1_bad = iv_rows_reference(iv_1, one, np.ones((B, M)), row, T)
        assert same_bits(sse_1, w1_sse) and np.array_equal(bad_1, w1_bad) and bad_1[5] >= bad[5]
        for wrong in (B, -1):
            with pytest.raises(_native.NativeError):
                surf.loss_terms_iv_rows(rec, mkt_iv, np.full(S, wrong, dtype=np.int32), N,
                                        weights=w)
        # crafted prices through the device-pointer entry: set 0's deepest in-the-money call one
        # ulp below its lower bound (vol 0.0, not bad), an infinite price in set 3 (bad)
        kabs = K * spots[0] / 100.0 if mode == _native.STRIKE_PCT_SPOT else K
        c0 = int(np.flatnonzero((call != 0) & (kabs < spots[0]) & (w[0] > 0))[0])
        lower = spots[0] - kabs[c0]
        assert lower > 0
        crafted = prices.copy()
        crafted[0, c0] = np.nextafter(lower, 0.0)
        c3 = int(np.flatnonzero(w[row[3]] > 0)[2])
        crafted[3, c3] = np.inf
        dev = torch.device("cuda", ctx.device)
        d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
             for k, v in dict(rec=rec, prices=crafted, iv=mkt_iv, w=w, row=row).items()}
        d_sse = torch.full((S,), -1.0, dtype=torch.float64, device=dev)
        d_bad = torch.full((S,), -7, dtype=torch.int32, device=dev)
        d_iv = torch.full((S, M), -1.0, dtype=torch.float64, device=dev)
        stream = torch.cuda.Stream(device=dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream):
            surf.iv_sse_rows_dev(d["rec"].data_ptr(), d["prices"].data_ptr(), d["iv"].data_ptr(),
                                 d["w"].data_ptr(), d["row"].data_ptr(), S, d_sse.data_ptr(),
                                 d_bad.data_ptr(), d_iv.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        c_sse, c_bad, c_iv = d_sse.cpu().numpy(), d_bad.cpu().numpy(), d_iv.cpu().numpy()
    finally:
        surf.close()
    assert c_iv[0, c0] == 0.0 and not np.signbit(c_iv[0, c0]) and np.isnan(c_iv[3, c3])
    keep = np.ones((S, M), dtype=bool)
    keep[0, c0] = keep[3, c3] = False
    assert same_bits(c_iv[keep], iv[keep])
    want_sse, want_bad = iv_rows_reference(c_iv, mkt_iv, w, row, T)
    assert same_bits(c_sse, want_sse) and np.array_equal(c_bad, want_bad)
    assert c_bad[0] == 0 and c_bad[3] == 1 and c_sse[0] != sse[0]
    rest = [1, 2, 4, 5, 6]
    assert same_bits(c_sse[rest], sse[rest]) and np.array_equal(c_bad[rest], bad[rest])


# ---- 2. identity with the single-market stage ---------------------------------------------------

@pytest.mark.parametrize("grid", ["pct15", "abs64"])
def test_rows_equal_the_single_market_stage(dh, grid):
    from dhcos import _native
    ctx = _native.default_context()
    K, T, call, mode = grid_of(grid)
    surf = _native.Surface(ctx, K, T, call, strike_mode=mode)
    try:
        rec, row, spots, mkt_iv, w = rows_case(surf, T)
        S = rec.shape[0]
        for b in (0, 2):                               # market 2 holds the NaN vol at weight 0
            sse, bad, iv = surf.loss_terms_iv_rows(rec, mkt_iv[b:b + 1], np.zeros(S, np.int32), N,
                                                   weights=w[b:b + 1], want_iv=True)
            surf.set_iv_market(mkt_iv[b], w[b])
            one_sse, one_bad, one_iv = surf.loss_terms_iv(rec, N, want_iv=True)
            assert same_bits(sse, one_sse), (b, sse, one_sse)
            assert np.array_equal(bad, one_bad) and same_bits(iv, one_iv)
            assert bad[5] > 0 and np.all(bad[:5] == 0) and np.all(sse[:5] > 0)
    finally:
        surf.close()


# ---- 3, 4. one traced run of 5 markets x 2 starts --------------------------------------------------

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


def bs_vega_and_scale(price, v, S0, K, T, r):
    """Black-Scholes vega of calls at vol v (q = 0) and test_gpu_iv.py's price scale: the price
    where the lower bound is 0, else the largest of price and the two discounted legs."""
    A, Bd = S0, K * np.exp(-r * T)
    sq = v * np.sqrt(T)
    with np.errstate(all="ignore"):                    # a clamped vol (0.0): vega 0, no bar
        d1 = np.log(A / Bd) / sq + 0.5 * sq
        vega = A * np.exp(-0.5 * d1 * d1) / np.sqrt(2.0 * np.pi) * np.sqrt(T)
    scale = np.where(A - Bd > 0.0, np.maximum(price, np.maximum(A, Bd)), price)
    return vega, scale


def grad_bar(x, f_ref, g_ref, dx, v, prices, mkt_iv, w, S0, K, T, r, yard=IV_YARDSTICK):
    """The bar on |g - g_ref|, derived: each of the two losses of a forward difference may move by
      E = transform_bound(x, g_ref)            the device's exp / tanh against NumPy's (2 ulp)
        + (log2 M + 4) spacing(f)              the two summation orders
        + sum_m 2 w_m |v_m - v_mkt,m| dv_m / sum(w)
    with dv_m = yard (eps v_m + eps scale_m / vega_m) the accuracy DESIGN.md 3.10 holds
    implied_vol to (the yardstick times the unit u: what one ulp of the price or of the bounds
    does to the vol), so |g_i - g_ref,i| <= 2 E / dx_i."""
    from test_gpu_shadow import transform_bound
    sel = w > 0
    vega, scale = bs_vega_and_scale(prices[sel], v[sel], S0, K[sel], T[sel], r)
    with np.errstate(all="ignore"):
        dv = yard * (EPS * v[sel] + EPS * scale / vega)
    e_iv = float(np.sum(2.0 * w[sel] * np.abs(v[sel] - mkt_iv[sel]) * dv) / w.sum())
    e = transform_bound(x, g_ref) + (np.log2(w.size) + 4) * np.spacing(abs(f_ref)) + e_iv
    return 2.0 * e / dx


def test_requests_are_the_vol_objective(dh, markets, traced):
    from dhcos.calibrator import fd_request_points
    m = markets
    _, tr = traced
    worst_f = worst_g = worst_g117 = 0.0
    n_invalid = 0
    lines = []
    for b in range(5):
        rows = tr[tr[:, 29] == b]
        assert {int(s) for s in rows[:, 0]} == {2 * b, 2 * b + 1}
        S0 = float(m["spots"][b])
        K = m["krel"] * S0 / 100.0
        cal = dh.DoubleHestonJumpCalibrator(S0, m["r"], options_of(m, b), N=N, objective="iv",
                                            market_ivs=m["ivs"][b], iv_weights=m["wts"][b])
        surf = cal._get_surface()
        for s in (0, 1):
            first, = rows[(rows[:, 0] == 2 * b + s) & (rows[:, 1] == 0)]
            assert np.array_equal(first[3:16], m["X"][b, s])
        for q in rows:                                  # every request: none is skipped
            x, f, g = q[3:16].copy(), float(q[2]), q[16:29].copy()
            f_ref, g_ref = cal.compute_loss_and_grad(x)
            dx = fd_request_points(x)[1]
            if f_ref == 1e10:
                n_invalid += 1
                assert f == 1e10, (b, q[0], q[1], f)
                assert np.all(np.abs(g - g_ref) <= 1e-9 * np.abs(g_ref)), (b, q[0], q[1], g, g_ref)
                continue
            assert abs(f - f_ref) <= 1e-9 * abs(f_ref), (b, q[0], q[1], f, f_ref)
            worst_f = max(worst_f, abs(f - f_ref) / (1e-9 * abs(f_ref)))
            _, rec = cal._records(x[None, :])
            _, bad, prices, v = surf.loss_terms_iv(rec, N, want_prices=True, want_iv=True)
            assert bad[0] == 0
            args = (x, f_ref, g_ref, dx, v[0], prices[0], m["ivs"][b], m["wts"][b], S0, K, m["T"],
                    m["r"])
            bar = grad_bar(*args)
            ratio = float(np.max(np.abs(g - g_ref) / bar))
            worst_g = max(worst_g, ratio)
            worst_g117 = max(worst_g117,
                             float(np.max(np.abs(g - g_ref) / grad_bar(*args, yard=117.0))))
            assert np.all(np.abs(g - g_ref) <= bar), (b, q[0], q[1], np.abs(g - g_ref) / bar)
        lines.append(f"market {b}: {len(rows)} requests")
    lines.append(f"{len(tr)} requests, {n_invalid} invalid (1e10 on both sides); worst "
                 f"|df| / (1e-9 |f|) = {worst_f:.3e}; worst |dg| / bar = {worst_g:.3e} with the "
                 f"vol term at the {IV_YARDSTICK:.0f} u implied_vol is held to "
                 f"({worst_g117:.3e} at the 117 u measured for it, DESIGN.md 3.10)")
    print("\n".join(lines))
    log = os.environ.get("DHCOS_SHADOW_LOG")
    if log:
        with open(log, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def test_batch_replays_bitwise_on_cpu_build(markets, traced):
    import test_lbfgs_device_algo as T
    lib = C.CDLL(os.path.join(ROOT, "tests", "native", "liblbhost.so"))
    lib.lbh_begin.argtypes = [C.c_void_p, T._D]
    lib.lbh_point.argtypes = [C.c_void_p, T._D]
    lib.lbh_set_fg.argtypes = [C.c_void_p, C.c_double, T._D]
    lib.lbh_resume.argtypes = [C.c_void_p] + [C.c_int] * 3 + [C.c_double] * 2
    lib.lbh_result.argtypes = [C.c_void_p, T._D, T._D, C.POINTER(C.c_int)]
    res, tr = traced
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
                more = lib.lbh_resume(st, 25, MAXFUN, 20, (1e-9 / EPS) * EPS, 1e-6)
                k += 1
            assert k == len(rows) == q.nfev
            x = np.empty(13)
            fv = C.c_double()
            info = (C.c_int * 4)()
            lib.lbh_result(st, x.ctypes.data_as(T._D), C.byref(fv), info)
            assert np.array_equal(x, np.array(q.x[:])) and fv.value == q.fun
            assert list(info) == [q.nit, q.nfev, q.task, q.warnflag]


# ---- 5. batch invariance ------------------------------------------------------------------------

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


def test_non_finite_market_ends_abnormal_and_moves_no_other_bit(markets):
    """The price objective's case is a NaN market price.  In vol space a NaN market vol at a
    positive weight never reaches the driver (DH_E_ARG, and ValueError above it), so the market
    whose every loss is not finite is one with a vol whose squared error overflows: sse = inf, f =
    inf, g = inf - inf = NaN -- ABNORMAL at nit 0 after 21 requests, as a NaN loss ends."""
    m = markets
    ref = run(m, range(5), 5)
    ivs = m["ivs"].copy()
    c = int(np.flatnonzero(m["wts"][2] > 0)[3])
    ivs[2, c] = 1e200
    got = run(m, range(5), 5, ivs=ivs)
    for b in (0, 1, 3, 4):
        assert all(same_start(a, q) for a, q in zip(got[b], ref[b])), b
    for s in (0, 1):
        q = got[2][s]
        assert (q.nit, q.nfev, q.task) == (0, 21, 8000)
        # fun is the last trial's loss: inf, or 1e10 once the NaN gradient has made the trial NaN
        assert q.fun in (np.inf, 1e10) and q.best_loss == np.inf
        assert np.array_equal(np.array(q.x[:]), m["X"][2, s])


def test_zero_weight_option_equals_the_market_alone(markets):
    m = markets
    ref = run(m, range(5), 5)
    wts = m["wts"].copy()
    c = int(np.flatnonzero(wts[1] > 0)[6])
    wts[1, c] = 0.0
    ivs = m["ivs"].copy()
    ivs[1, c] = np.nan                                  # anything may stand under a zero weight
    got = run(m, range(5), 5, ivs=ivs, wts=wts)
    alone = run(m, [1], 5, ivs=ivs, wts=wts)
    for a, q in zip(alone[1], got[1]):
        assert np.array_equal(np.array(a.x[:]), np.array(q.x[:])) and a.fun == q.fun
        assert same_start(a, q)
    assert any(a.fun != q.fun for a, q in zip(got[1], ref[1]))   # the weight is read
    for b in (0, 2, 3, 4):
        assert all(same_start(a, q) for a, q in zip(got[b], ref[b])), b


def test_library_checks_vols_and_weights(markets):
    """dh_calibrate_lbfgs_batch_iv's own DH_E_ARG cases (the Python layer checks the same things
    first, so the library is called directly)."""
    from dhcos import _native
    m = markets
    lib = _native.load()
    surf = m["surf"]
    B, S = 2, 2
    x0 = np.ascontiguousarray(m["X"][:B, 1])
    mof = np.arange(B, dtype=np.int32)
    opt = _native.LbOptions(3, MAXFUN, 20, 8, 1e-9, 1e-6)
    out = (_native.LbResult * S)()
    nl = C.c_int32(0)

    def call(iv, w):
        iv = np.ascontiguousarray(iv)
        w = None if w is None else np.ascontiguousarray(w)
        return lib.dh_calibrate_lbfgs_batch_iv(
            surf.ctx.handle, surf.handle, _native._ptr(iv), None if w is None else _native._ptr(w),
            _native._ptr(m["spots"][:B].copy()), _native._ptr(m["rates"][:B].copy()), B,
            _native._ptr(x0), _native._ptr(mof, _native._i32p), S, N, 10.0, C.byref(opt), out,
            C.byref(nl))

    iv = np.full((B, 15), 0.2)
    for v in (-1.0, np.nan, np.inf):
        w = np.ones((B, 15))
        w[1, 4] = v
        assert call(iv, w) == -1
        assert b"market 1 option 4" in lib.dh_last_error()
    w = np.ones((B, 15))
    w[0] = 0.0
    assert call(iv, w) == -1 and b"market 0" in lib.dh_last_error()
    hole = iv.copy()
    hole[1, 9] = np.nan
    assert call(hole, None) == -1 and b"market 1 option 9" in lib.dh_last_error()
    hole[1, 9] = -0.2
    assert call(hole, np.ones((B, 15))) == -1 and b"market 1 option 9" in lib.dh_last_error()
    w = np.ones((B, 15))
    w[1, 9] = 0.0
    assert call(hole, w) == 0 and nl.value > 0          # anything under a zero weight


# ---- 6. it fits vols ------------------------------------------------------------------------------

def test_noise_free_market_is_fitted_in_vol_space(dh, markets):
    from dhcos import batch as Bt
    from dhcos.generator import MATURITIES, STRIKES_PCT
    m = markets
    model = np.array([0.04, 2.5, 0.045, 0.3, -0.7, 0.035, 0.6, 0.05, 0.2, -0.5, 0.15, -0.04, 0.08])
    spot, r = 103.25, 0.03
    rec = np.zeros((1, 16))
    rec[0, :13], rec[0, 13], rec[0, 14] = model, spot, r
    mkt = m["surf"].price(rec, N)                       # [1, 15], no noise
    cal = dh.DoubleHestonJumpCalibrator(spot, r, [])
    rs = np.random.RandomState(9)
    x0 = cal.inverse_transform_params(dict(zip(cal.param_names,
                                               model * (1 + 0.05 * rs.randn(13)))))
    res = dh.calibrate_batch(mkt, [spot], r, x0s=x0[None, None, :], maxiter=50, objective="iv")
    K, T, flags, _ = Bt._grid(STRIKES_PCT, MATURITIES, None, True)
    Kabs = K[None, :] * spot / 100.0
    want_iv = dh.implied_vol(mkt, spot, Kabs, T[None, :], r, 0.0, flags[None, :])
    assert same_bits(res.market_ivs, want_iv) and np.all(res.iv_weights == 1.0)
    opts = [{"strike": float(k), "maturity": float(t), "price": float(p), "option_type": "call"}
            for k, t, p in zip(Kabs[0], T, mkt[0])]
    start = dh.DoubleHestonJumpCalibrator(spot, r, opts, N=N, objective="iv",
                                          market_ivs=want_iv[0]).compute_loss(x0)
    print(f"vol-space loss {start:.6e} -> {res.final_loss[0]:.6e} in {res.iterations[0]} "
          f"iterations ({res.message(0)})")
    assert res.objective == "iv" and res.best_start[0] == 0
    assert np.isfinite(res.final_loss[0]) and res.final_loss[0] < start
    assert res.final_loss[0] == res.fun[0, 0]
    back = dh.implied_vol(res.model_prices, spot, Kabs, T[None, :], r, 0.0, flags[None, :])
    assert same_bits(res.model_ivs, back)
    rec[0, :13] = res.parameters[0]
    assert same_bits(res.model_prices, m["surf"].price(rec, N))


# ---- 7. the price objective is untouched ------------------------------------------------------------

def test_price_objective_is_untouched(dh, markets):
    m = markets
    B = 4
    args = (m["mkt"][:B], m["spots"][:B], m["r"])
    a = dh.calibrate_batch(*args, x0s=m["X"][:B], maxiter=5)
    b = dh.calibrate_batch(*args, x0s=m["X"][:B], maxiter=5, objective="price")
    assert a.objective == b.objective == "price" and b.model_ivs is None and b.market_ivs is None
    for name in ("x", "parameters", "final_loss", "fun", "best_loss", "model_prices", "start_x"):
        assert same_bits(getattr(a, name), getattr(b, name)), name
    for name in ("nit", "nfev", "start_task", "status", "n_calls", "best_start", "iterations",
                 "task", "success"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    direct, _ = m["surf"].calibrate_lbfgs_batch(m["mkt"][:B], m["spots"][:B], m["rates"][:B],
                                               m["X"][:B].reshape(-1, 13),
                                               np.repeat(np.arange(B, dtype=np.int32), 2), N,
                                               maxiter=5, maxfun=MAXFUN)
    assert same_bits(a.fun.reshape(-1), [q.fun for q in direct])


# ---- 8. the public API ------------------------------------------------------------------------------

def test_calibrate_batch_iv_api(dh, markets):
    m = markets
    B = 4
    res = dh.calibrate_batch(m["mkt"][:B], m["spots"][:B], m["r"], x0s=m["X"][:B], maxiter=5,
                             objective="iv", market_ivs=m["ivs"][:B], iv_weights=m["wts"][:B])
    direct = run(m, range(B), 5)
    assert res.objective == "iv" and res.model_ivs.shape == (B, 15)
    assert same_bits(res.market_ivs, m["ivs"][:B]) and np.array_equal(res.iv_weights,
                                                                      m["wts"][:B])
    for b in range(B):
        funs = [q.fun for q in direct[b]]
        assert np.array_equal(res.fun[b], funs)
        w = int(res.best_start[b])
        assert w == int(np.argmin(funs)) and res.final_loss[b] == funs[w]
        assert np.array_equal(res.x[b], np.array(direct[b][w].x[:]))
        one = res.result(b)
        assert one.spot == m["spots"][b] and one.final_loss == funs[w]
        assert one.iterations == direct[b][w].nit and len(one.market_options) == 15
        assert np.array_equal(one.market_prices, m["mkt"][b])
        rec = np.zeros((1, 16))
        rec[0, :13], rec[0, 13], rec[0, 14] = res.parameters[b], m["spots"][b], m["r"]
        iv, prices = m["surf"].implied_vol(rec, N, want_prices=True)
        assert same_bits(res.model_prices[b], prices[0]) and same_bits(res.model_ivs[b], iv[0])
        assert same_bits(one.model_prices, prices[0])
    # the default vols are the inversion of the market prices; [M] weights serve every market
    w15 = np.all(m["wts"][:B] > 0, axis=0).astype(float)
    res2 = dh.calibrate_batch(m["mkt"][:B], m["spots"][:B], m["r"], x0s=m["X"][:B], maxiter=2,
                              objective="iv", iv_weights=w15)
    sel = np.isfinite(m["ivs"][:B])
    assert np.allclose(res2.market_ivs[sel], m["ivs"][:B][sel], rtol=1e-9, atol=0.0)
    assert res2.iv_weights.shape == (B, 15) and np.all(res2.iv_weights == w15)
    # a market without a vol at a positive weight: named, before any RNG draw
    mkt = m["mkt"][:B].copy()
    mkt[2, 0] = 0.5 * (m["spots"][2] - m["krel"][0] * m["spots"][2] / 100.0)   # below intrinsic
    w = m["wts"][:B].copy()                             # 0 where the generator's price has no vol
    w[2, 0] = 1.0
    state = np.random.get_state()
    with pytest.raises(ValueError, match=r"\[\[2, 0\]\]"):
        dh.calibrate_batch(mkt, m["spots"][:B], m["r"], objective="iv", iv_weights=w,
                           multi_start=2)
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
