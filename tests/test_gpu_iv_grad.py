"""GPU tests of the vol objective's exact gradient (csrc/dh_iv_grad.h: dh_surface_iv_grad_rows_dev,
dh_surface_loss_iv_grad_rows*, dh_calibrate_lbfgs_batch_iv_grad; calibrate_batch(objective="iv",
gradient="vega"); DoubleHestonJumpCalibrator(objective="iv", gradient="vega")).  DESIGN.md 3.20.

  1. the reduction alone on crafted planes, S = 7 sets over B = 3 markets with different spots
     (tests/test_gpu_calibrate_batch_iv.py's rows_case) on M = 15, 64 (unsorted maturities, puts and
     calls) and 70 (a lane adds two options), with a set of NaN prices, a single NaN price, an
     infinite one, a price one ulp below its lower bound and a zero weight over a NaN market vol:
     sse, n_bad and iv are dh_surface_iv_sse_rows_dev's bits for plane 0; an invalid set gives f =
     1e10 and g = 0; f is sse / div + pen; g is the restatement's on the same planes and vols;
     permuted, repeated and single-set calls give the same bits;
  2. the full request against the restatement (tests/iv_grad_reference.py) at the device's own vols
     as used: f to 1e-9 relative (DESIGN.md 3.19's bar), g to 3.18's bar 1e-6 |g_i| + 1e-10 max |g|
     plus the inversion term (2 / sum w) sum_m w_m dv_m |plane_i,m| / vega_m |dtheta_i/dx_i| with
     dv_m 3.13's (the 5,493 u implied_vol is held to);
  3. the driver: a market alone and among others at chunk 1 and 8, bit for bit; every traced
     (x, f, g) of a short run is the rows request's bits at the traced x and the restatement within
     the bars of 2; the CPU build of the state machine (tests/native/liblbhost.so) fed the device's
     (f, g) asks for the same points bit for bit; n_calls == nfev;
  4. on test_gpu_calibrate_batch_iv.py's noise-free market, from x* + 0.05, the final vol loss is
     within 10x of gradient="fd"'s (3.19's bar) and loss_evals is the request count;
  5. the SciPy driver's compute_loss_and_grad has the bits of Surface.loss_iv_grad_rows with B = 1.
"""
import ctypes as C
import os

import numpy as np
import pytest

import iv_grad_reference as V
import param_grad_reference as R
from conftest import ROOT
from oracle import dh_oracle as O
from test_gpu_calibrate_batch_iv import (EPS, HI, IV_YARDSTICK, LO, bs_vega_and_scale, grid_of,
                                         rows_case, same_bits)

pytestmark = pytest.mark.gpu

MAXFUN = 1071


@pytest.fixture(scope="module")
def native():
    from dhcos import _native
    if _native.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return _native


def weight_sums(w):
    """Each market's weight sum as the library forms it: option order, sequential, from 0.0."""
    return np.cumsum(np.asarray(w, dtype=np.float64), axis=1)[:, -1]


def feller_of(rec):
    v1 = rec[:, 3] * rec[:, 3] - 2.0 * rec[:, 1] * rec[:, 2]
    v2 = rec[:, 8] * rec[:, 8] - 2.0 * rec[:, 6] * rec[:, 7]
    return 1000.0 * (np.where(v1 > 0.0, v1, 0.0) + np.where(v2 > 0.0, v2, 0.0))


def assert_g(g, want_g, extra, label):
    """3.18's bar plus `extra` [13] (the inversion term, or 0) -> the worst error over the bar."""
    tol = 1e-6 * np.abs(want_g) + 1e-10 * np.max(np.abs(want_g))
    err = np.abs(g - want_g)
    frac, frac_all = float(np.max(err / tol)), float(np.max(err / (tol + extra)))
    print(f"{label}: g worst err / (3.18's bar) {frac:.3e}, / (bar + inversion term) {frac_all:.3e}")
    assert np.all(err <= tol + extra), (label, [O.PARAM_NAMES[i]
                                                for i in np.flatnonzero(err > tol + extra)])
    return frac, frac_all


# ---- 1. the reduction alone --------------------------------------------------------------------

def reduce_on_device(surf, planes, rec, pen, mkt_iv, w, row, div):
    """dh_surface_iv_grad_rows_dev and dh_surface_iv_sse_rows_dev on plane 0, on a stream of their
    own -> (f, g, bad, sse, iv), (sse, bad, iv)."""
    import torch
    S, M = rec.shape[0], surf.M
    dev = torch.device("cuda", surf.ctx.device)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
         for k, v in dict(planes=planes, rec=rec, pen=pen, iv=mkt_iv, w=w, row=row,
                          div=div).items()}

    def outs():
        return (torch.full((S,), -1.0, dtype=torch.float64, device=dev),
                torch.full((S,), -7, dtype=torch.int32, device=dev),
                torch.full((S, M), -1.0, dtype=torch.float64, device=dev))

    f = torch.full((S,), -1.0, dtype=torch.float64, device=dev)
    g = torch.full((S, 13), -1.0, dtype=torch.float64, device=dev)
    sse, bad, iv = outs()
    sse2, bad2, iv2 = outs()
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        surf.iv_grad_rows_dev(d["planes"].data_ptr(), d["rec"].data_ptr(), d["pen"].data_ptr(),
                              d["iv"].data_ptr(), d["w"].data_ptr(), d["row"].data_ptr(),
                              d["div"].data_ptr(), S, f.data_ptr(), g.data_ptr(), bad.data_ptr(),
                              d_sse=sse.data_ptr(), d_iv=iv.data_ptr(), stream=stream.cuda_stream)
        surf.iv_sse_rows_dev(d["rec"].data_ptr(), d["planes"].data_ptr(), d["iv"].data_ptr(),
                             d["w"].data_ptr(), d["row"].data_ptr(), S, sse2.data_ptr(),
                             bad2.data_ptr(), iv2.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    return ([a.cpu().numpy() for a in (f, g, bad, sse, iv)],
            [a.cpu().numpy() for a in (sse2, bad2, iv2)])


@pytest.mark.parametrize("grid", ["pct15", "abs64", "abs70"])
def test_reduction_on_crafted_planes(native, grid):
    ctx = native.default_context()
    K, T, call, mode = grid_of(grid)
    surf = native.Surface(ctx, K, T, call, strike_mode=mode)
    try:
        M = surf.M
        assert M == {"pct15": 15, "abs64": 64, "abs70": 70}[grid]
        rec, row, spots, mkt_iv, w = rows_case(surf, T)
        S = rec.shape[0]
        planes = surf.param_sens(rec, 128)                           # [14, S, M]
        kabs = K * spots[0] / 100.0 if mode == native.STRIKE_PCT_SPOT else K
        # set 0: its deepest in-the-money call one ulp below its lower bound (r = 0: exact);
        # set 3: an infinite price; set 1: a NaN price; set 5 is rows_case's set of NaN prices
        c0 = int(np.flatnonzero((call != 0) & (kabs < spots[0]) & (w[0] > 0))[0])
        lower = spots[0] - kabs[c0]
        assert lower > 0
        planes[0, 0, c0] = np.nextafter(lower, 0.0)
        c3 = int(np.flatnonzero(w[row[3]] > 0)[2])
        planes[0, 3, c3] = np.inf
        c1 = int(np.flatnonzero(w[row[1]] > 0)[4])
        planes[0, 1, c1] = np.nan
        pen = feller_of(rec)
        div = weight_sums(w)[row]
        assert np.isnan(mkt_iv[2, M - 2]) and w[2, M - 2] == 0.0     # rows_case's zero weight
        (f, g, bad, sse, iv), (sse2, bad2, iv2) = reduce_on_device(surf, planes, rec, pen, mkt_iv,
                                                                   w, row, div)
        again, _ = reduce_on_device(surf, planes, rec, pen, mkt_iv, w, row, div)
        perm = np.array([4, 6, 0, 3, 5, 2, 1, 3])
        permuted, _ = reduce_on_device(surf, planes[:, perm], rec[perm], pen[perm], mkt_iv, w,
                                       row[perm], div[perm])
        single, _ = reduce_on_device(surf, planes[:, 2:3], rec[2:3], pen[2:3], mkt_iv, w,
                                     row[2:3], div[2:3])
    finally:
        surf.close()
    # the vol-space reduction's bits on plane 0
    assert same_bits(sse, sse2) and np.array_equal(bad, bad2) and same_bits(iv, iv2)
    assert iv[0, c0] == 0.0 and not np.signbit(iv[0, c0]) and bad[0] == 0
    assert np.isnan(iv[3, c3]) and bad[3] == 1 and np.isnan(iv[1, c1]) and bad[1] == 1
    assert bad[5] > 1 and np.all(bad[[0, 2, 4, 6]] == 0)
    # invalid sets
    for s in (1, 3, 5):
        assert f[s] == 1e10 and not g[s].any() and np.signbit(g[s]).sum() == 0
    # valid sets: f from sse, g the restatement's on the same planes and the vols as used
    for s in (0, 2, 4, 6):
        assert f[s] == sse[s] / div[s] + pen[s]
        b = row[s]
        ks = K * spots[b] / 100.0 if mode == native.STRIKE_PCT_SPOT else K
        want = V.reduce_planes(planes[:, s], rec[s, :13], iv[s], mkt_iv[b], w[b], spots[b], ks, T,
                               0.0)
        assert want[3] == 0 and want[2] == sse[s], (s, want[2], sse[s])
        assert abs(want[0] - f[s]) <= 1e-14 * abs(f[s]), (s, want[0], f[s])
        assert_g(g[s], want[1], 0.0, f"{grid} set {s}")
    # the clamped option moves the loss and no gradient sum: its c_m is 0
    assert np.isfinite(g[0]).all() and g[0].any()
    # any place in any call
    for a, b_ in zip(again, (f, g, bad, sse, iv)):
        assert same_bits(a, b_)
    for a, b_ in zip(permuted, (f, g, bad, sse, iv)):
        assert same_bits(a, b_[perm])
    for a, b_ in zip(single, (f, g, bad, sse, iv)):
        assert same_bits(a, b_[2:3])


# ---- 2. the full request ---------------------------------------------------------------------------

def inversion_term(planes_ref, p, v, w, S0, K, T, r):
    """(2 / sum w) sum_m w_m dv_m |plane_i,m| / vega_m |dtheta_i/dx_i|, dv_m = yard (eps v_m + eps
    scale_m / vega_m): what the accuracy implied_vol is held to does to g."""
    sel = w > 0
    vega, scale = bs_vega_and_scale(planes_ref[0][sel], v[sel], S0, K[sel], T[sel], r)
    dv = IV_YARDSTICK * (EPS * v[sel] + EPS * scale / vega)
    per = (w[sel] * dv / vega)[None, :] * np.abs(planes_ref[1:][:, sel])          # [13, m]
    return (2.0 / w.sum()) * per.sum(axis=1) * np.abs(R.dtheta_dx(p))


@pytest.mark.parametrize("grid", ["pct15", "abs70"])
def test_request_matches_the_restatement_at_the_devices_vols(native, grid):
    import torch
    ctx = native.default_context()
    K, T, call, mode = grid_of(grid)
    M, N = K.size, 64
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
    surf = native.Surface(ctx, K, T, call, strike_mode=mode)
    try:
        mkt_iv = surf.implied_vol(base, N) + rs.uniform(-0.02, 0.02, size=(B, M))
        w = rs.uniform(0.25, 4.0, size=(B, M))
        w[0, 1] = 0.0
        mkt_iv[0, 1] = np.nan
        f, g, bad, iv = surf.loss_iv_grad_rows(X, mkt_iv, w, spots, rates, row, N)
        perm = np.array([3, 5, 0, 2, 4, 1, 2])
        fp, gp, bp, ivp = surf.loss_iv_grad_rows(X[perm], mkt_iv, w, spots, rates, row[perm], N)
        f1, g1, b1, iv1 = surf.loss_iv_grad_rows(X[3:4], mkt_iv[2:3], w[2:3], spots[2:3],
                                                 rates[2:3], [0], N)
        for wrong in (B, -1):
            with pytest.raises(native.NativeError):
                surf.loss_iv_grad_rows(X, mkt_iv, w, spots, rates, np.full(S, wrong, np.int32), N)
        neg = w.copy()
        neg[1, 3] = -1.0
        with pytest.raises(native.NativeError, match="market 1 option 3"):
            surf.loss_iv_grad_rows(X, mkt_iv, neg, spots, rates, row, N)
        hole = mkt_iv.copy()
        hole[2, 5] = np.nan
        with pytest.raises(native.NativeError, match="market 2 option 5"):
            surf.loss_iv_grad_rows(X, hole, w, spots, rates, row, N)
        with pytest.raises(native.NativeError, match="N must be"):
            surf.loss_iv_grad_rows(X, mkt_iv, w, spots, rates, row, 1025)
        # the device-pointer form: the same bits
        dev = torch.device("cuda", ctx.device)
        div = weight_sums(w)[row]
        d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev)
             for a in (X, mkt_iv, w, div, spots, rates, row)]
        d_f = torch.empty(S, dtype=torch.float64, device=dev)
        d_g = torch.empty((S, 13), dtype=torch.float64, device=dev)
        d_bad = torch.empty(S, dtype=torch.int32, device=dev)
        d_iv = torch.empty((S, M), dtype=torch.float64, device=dev)
        stream = torch.cuda.Stream(device=dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream):
            surf.loss_iv_grad_rows_dev(*(a.data_ptr() for a in d), S, d_f.data_ptr(),
                                       d_g.data_ptr(), d_bad.data_ptr(), d_iv.data_ptr(), N=N,
                                       stream=stream.cuda_stream)
        stream.synchronize()
        # the vols as used are the vol-space rows request's
        rec = np.zeros((S, 16))
        rec[:, :13] = [O.to_params(x) for x in X]
        rec[:, 13], rec[:, 14] = spots[row], rates[row]
        _, bad_iv, iv_rows = surf.loss_terms_iv_rows(rec, mkt_iv, row, N, weights=w, want_iv=True)
    finally:
        surf.close()
    assert bad[4] == M and np.all(np.delete(bad, 4) == 0)
    assert f[4] == 1e10 and not g[4].any() and np.signbit(g[4]).sum() == 0
    assert same_bits(fp, f[perm]) and same_bits(gp, g[perm]) and np.array_equal(bp, bad[perm])
    assert same_bits(ivp, iv[perm])
    assert f1[0] == f[3] and same_bits(g1[0], g[3]) and b1[0] == 0 and same_bits(iv1[0], iv[3])
    assert same_bits(d_f.cpu().numpy(), f) and same_bits(d_g.cpu().numpy(), g)
    assert np.array_equal(d_bad.cpu().numpy(), bad) and same_bits(d_iv.cpu().numpy(), iv)
    valid = [0, 1, 2, 3, 5]
    assert np.array_equal(np.isnan(iv), np.isnan(iv_rows))
    assert np.array_equal(bad_iv > 0, bad > 0)
    fracs = []
    for s in valid:
        b = row[s]
        p = O.to_params(X[s])                           # no set within rounding of the Feller kink
        assert min(abs(p[3] ** 2 - 2 * p[1] * p[2]), abs(p[8] ** 2 - 2 * p[6] * p[7])) > 1e-6
        ks = K * spots[b] / 100.0 if mode == native.STRIKE_PCT_SPOT else K
        assert np.all(iv[s] > 0.05)                      # none near the clamp
        planes_ref = V.planes_of(p, spots[b], ks, T, rates[b], call, N)
        want_f, want_g, _, nb = V.reduce_planes(planes_ref, p, iv[s], mkt_iv[b], w[b], spots[b],
                                                ks, T, rates[b])
        assert nb == 0
        print(f"{grid} set {s} market {b}: f {f[s]:.12e} ref {want_f:.12e} rel "
              f"{abs(f[s] - want_f) / abs(want_f):.2e}")
        assert abs(f[s] - want_f) <= 1e-9 * abs(want_f), (s, f[s], want_f)
        extra = inversion_term(planes_ref, p, iv[s], w[b], spots[b], ks, T, rates[b])
        fracs.append(assert_g(g[s], want_g, extra, f"{grid} set {s} market {b}"))
    print(f"{grid}: worst fraction of 3.18's bar {max(a for a, _ in fracs):.3e}, of the bar with "
          f"the inversion term {max(b_ for _, b_ in fracs):.3e}")
    assert len({f[0], f[5]}) == 2                       # the rows matter


# ---- 3. the driver ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def markets(native):
    """Five generator markets with their vols, weight 0 where a noisy price has none, and two warm
    starts each (the true parameters under 5% noise)."""
    import dhcos
    from dhcos.generator import MATURITIES, STRIKES_PCT, grid_surface
    np.random.seed(11)
    g = dhcos.generate_synthetic_calibrations(5, None, as_arrays=True, verbose=False,
                                              implied_vols=True)
    spots = np.ascontiguousarray(g["spot"], dtype=np.float64)
    ivs = np.ascontiguousarray(g["market_iv"], dtype=np.float64)
    wts = (np.isfinite(ivs) & (ivs >= 0)).astype(np.float64)
    assert np.all(wts.sum(axis=1) > 0)
    surf, krel, T = grid_surface(native.default_context(), STRIKES_PCT, MATURITIES)
    r = float(g["risk_free"])
    cal = dhcos.DoubleHestonJumpCalibrator(100.0, r, [])
    rs = np.random.RandomState(5)
    X = np.empty((5, 2, 13))
    for b in range(5):
        for s in range(2):
            true = dict(zip(cal.param_names, g["params"][b] * (1 + 0.05 * rs.randn(13))))
            X[b, s] = cal.inverse_transform_params(true)
    return dict(ivs=ivs, wts=wts, spots=spots, r=r, rates=np.full(5, r), surf=surf,
                krel=np.asarray(krel, dtype=np.float64), T=np.asarray(T, dtype=np.float64), X=X)


def run(m, sel, starts, maxiter, chunk=8, N=128):
    sel = list(sel)
    X = m["X"][sel][:, list(starts)]
    S = X.shape[1]
    mof = np.repeat(np.arange(len(sel), dtype=np.int32), S)
    res, _ = m["surf"].calibrate_lbfgs_batch_iv_grad(
        m["ivs"][sel], m["wts"][sel], m["spots"][sel], m["rates"][sel], X.reshape(-1, 13), mof, N,
        maxiter=maxiter, maxfun=MAXFUN, chunk=chunk)
    return {b: res[i * S:(i + 1) * S] for i, b in enumerate(sel)}


def same_start(a, b):
    return (np.array_equal(np.array(a.x[:]), np.array(b.x[:])) and a.fun == b.fun
            and (a.nit, a.nfev, a.task, a.n_calls) == (b.nit, b.nfev, b.task, b.n_calls)
            and a.best_loss == b.best_loss)


def test_a_market_does_not_depend_on_the_batch(markets):
    m = markets
    alone = run(m, [1], (0,), 30)[1][0]
    print(f"market 1 alone: nit {alone.nit} nfev {alone.nfev} task {alone.task} fun {alone.fun:.6e}")
    assert alone.nfev == alone.n_calls > alone.nit > 1 and np.isfinite(alone.fun)
    for chunk in (1, 8):
        got = run(m, [4, 2, 1, 0, 3], (0, 1), 30, chunk=chunk)
        assert same_start(got[1][0], alone), chunk
        assert all(q.n_calls == q.nfev for b in got for q in got[b])


def test_every_request_is_the_restatement_and_the_state_machines_point(native, markets):
    m = markets
    b, maxiter, N = 2, 12, 128
    surf, ctx = m["surf"], m["surf"].ctx
    x0 = m["X"][b, 1]
    try:
        ctx.set_lb_trace(4096)
        (res,), _ = surf.calibrate_lbfgs_batch_iv_grad(
            m["ivs"][b:b + 1], m["wts"][b:b + 1], m["spots"][b:b + 1], m["rates"][b:b + 1],
            x0[None, :], [0], N, maxiter=maxiter, maxfun=MAXFUN)
        tr = ctx.read_lb_trace()
    finally:
        ctx.set_lb_trace(0)
    assert res.n_calls == res.nfev == len(tr) > 2
    rows = tr[np.argsort(tr[:, 1])]
    assert np.array_equal(rows[:, 1], np.arange(len(rows))) and np.array_equal(rows[0, 3:16], x0)
    print(f"{len(rows)} requests, nit {res.nit}, task {res.task}, fun {res.fun:.6e}")
    S0, r = float(m["spots"][b]), m["r"]
    ks = m["krel"] * S0 / 100.0
    call = np.ones(15, dtype=bool)
    mkt_iv, w = m["ivs"][b], m["wts"][b]
    # each traced (x, f, g): the rows request's bits at the traced x, and the restatement there
    Xt = np.ascontiguousarray(rows[:, 3:16])
    f, g, bad, iv = surf.loss_iv_grad_rows(Xt, mkt_iv[None, :], w[None, :], [S0], [r],
                                           np.zeros(len(Xt), np.int32), N)
    assert same_bits(f, rows[:, 2]) and same_bits(g, rows[:, 16:29])
    fracs = []
    for k, q in enumerate(rows):
        if bad[k]:
            assert q[2] == 1e10 and not q[16:29].any()
            continue
        p = O.to_params(q[3:16])
        planes_ref = V.planes_of(p, S0, ks, m["T"], r, call, N)
        want_f, want_g, _, nb = V.reduce_planes(planes_ref, p, iv[k], mkt_iv, w, S0, ks, m["T"], r)
        assert nb == 0 and abs(q[2] - want_f) <= 1e-9 * abs(want_f), (k, q[2], want_f)
        extra = inversion_term(planes_ref, p, iv[k], w, S0, ks, m["T"], r)
        fracs.append(assert_g(q[16:29], want_g, extra, f"request {k}"))
    print(f"traced run: worst fraction of 3.18's bar {max(a for a, _ in fracs):.3e}, with the "
          f"inversion term {max(c for _, c in fracs):.3e}")
    # the device's state machine on the CPU: the same points bit for bit, the same end
    lib = C.CDLL(os.path.join(ROOT, "tests", "native", "liblbhost.so"))
    D = C.POINTER(C.c_double)
    lib.lbh_begin.argtypes = [C.c_void_p, D]
    lib.lbh_point.argtypes = [C.c_void_p, D]
    lib.lbh_set_fg.argtypes = [C.c_void_p, C.c_double, D]
    lib.lbh_resume.argtypes = [C.c_void_p] + [C.c_int] * 3 + [C.c_double] * 2
    lib.lbh_result.argtypes = [C.c_void_p, D, D, C.POINTER(C.c_int)]
    st = C.create_string_buffer(lib.lbh_state_size())
    more = lib.lbh_begin(st, np.ascontiguousarray(x0).ctypes.data_as(D))
    xe = np.empty(13)
    k = 0
    while more:
        lib.lbh_point(st, xe.ctypes.data_as(D))
        assert np.array_equal(xe, rows[k, 3:16]), k
        gk = np.ascontiguousarray(rows[k, 16:29])
        lib.lbh_set_fg(st, rows[k, 2], gk.ctypes.data_as(D))
        more = lib.lbh_resume(st, maxiter, MAXFUN, 20, (1e-9 / EPS) * EPS, 1e-6)
        k += 1
    assert k == len(rows) == res.nfev
    x = np.empty(13)
    fv = C.c_double()
    info = (C.c_int * 4)()
    lib.lbh_result(st, x.ctypes.data_as(D), C.byref(fv), info)
    assert np.array_equal(x, np.array(res.x[:])) and fv.value == res.fun
    assert list(info) == [res.nit, res.nfev, res.task, res.warnflag]


# ---- 4. convergence ------------------------------------------------------------------------------------

def test_noise_free_market_converges_where_fd_does(native):
    """test_gpu_calibrate_batch_iv.py's noise-free market from x* + 0.05.  Trajectories are chaotic
    (DESIGN.md 2): neither x nor nit is compared; the factor 10 is 3.19's."""
    import dhcos
    from dhcos.generator import MATURITIES, STRIKES_PCT, grid_surface
    model = np.array([0.04, 2.5, 0.045, 0.3, -0.7, 0.035, 0.6, 0.05, 0.2, -0.5, 0.15, -0.04, 0.08])
    spot, r = 103.25, 0.03
    surf = grid_surface(native.default_context(), STRIKES_PCT, MATURITIES)[0]
    rec = np.zeros((1, 16))
    rec[0, :13], rec[0, 13], rec[0, 14] = model, spot, r
    mkt = surf.price(rec, 128)
    cal = dhcos.DoubleHestonJumpCalibrator(spot, r, [])
    x0 = cal.inverse_transform_params(dict(zip(cal.param_names, model))) + 0.05
    out = {}
    for grad in ("vega", "fd"):
        q = dhcos.calibrate_batch(mkt, [spot], r, x0s=x0[None, None, :], maxiter=300,
                                  objective="iv", gradient=grad)
        print(f"{grad}: final vol loss {q.final_loss[0]:.6e} nit {q.iterations[0]} requests "
              f"{int(q.nfev.sum())} loss evaluations {q.loss_evals} {q.message(0)!r}")
        assert q.gradient == grad and q.objective == "iv" and q.best_start[0] == 0
        out[grad] = q
    vg, fd = out["vega"], out["fd"]
    assert np.array_equal(vg.n_calls, vg.nfev) and vg.loss_evals == int(vg.nfev.sum()) > 0
    assert fd.loss_evals == 14 * int(fd.nfev.sum())
    assert same_bits(vg.market_ivs, fd.market_ivs) and vg.model_ivs.shape == (1, 15)
    assert np.isfinite(vg.final_loss[0]) and vg.final_loss[0] <= 10.0 * fd.final_loss[0]


# ---- 5. the SciPy driver ----------------------------------------------------------------------------------

def test_scipy_drivers_request_is_the_rows_request(native, markets):
    import dhcos
    m = markets
    b = 3
    S0, r = float(m["spots"][b]), m["r"]
    ks = m["krel"] * S0 / 100.0
    rec = np.zeros((1, 16))
    rec[0, :13] = O.to_params(m["X"][b, 0])
    rec[0, 13], rec[0, 14] = S0, r
    prices = m["surf"].price(rec, 128)[0]
    opts = [{"strike": float(k), "maturity": float(t), "price": float(p), "option_type": "call"}
            for k, t, p in zip(ks, m["T"], prices)]
    cal = dhcos.DoubleHestonJumpCalibrator(S0, r, opts, N=128, objective="iv", gradient="vega",
                                           market_ivs=m["ivs"][b], iv_weights=m["wts"][b])
    x = m["X"][b, 1]
    f, g = cal.compute_loss_and_grad(x)
    assert cal.n_calls == 1 and cal.loss_evals == 1 and cal.best_loss == f
    surf = native.Surface(native.default_context(), ks, m["T"], np.ones(15, bool))
    try:
        f2, g2, bad, _ = surf.loss_iv_grad_rows(x[None, :], m["ivs"][b][None, :],
                                                m["wts"][b][None, :], [S0], [r], [0], 128)
    finally:
        surf.close()
    assert bad[0] == 0 and f == f2[0] and same_bits(g, g2[0])
    fb, gb, low = cal.fg_batch(np.stack([x, m["X"][b, 0]]))
    assert fb[0] == f and same_bits(gb[0], g) and low[0] == f
    np.random.seed(3)
    res = cal.calibrate(maxiter=3, multi_start=2)               # the lockstep loop
    assert np.isfinite(res.final_loss) and cal.loss_evals > 3
