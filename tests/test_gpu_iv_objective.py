"""GPU tests of the implied-vol calibration objective (csrc/dh_iv_loss.h: dh_surface_set_iv_market,
dh_surface_iv_sse_dev, dh_surface_loss_iv_dev, dh_surface_loss_iv; DoubleHestonJumpCalibrator(
objective="iv")).  DESIGN.md 3.11.

Bars.  The vols and prices are compared bit for bit with dh_surface_implied_vol / dh_surface_price
(the same device functions).  sse is compared with math.fsum of the host's terms w (iv - mkt)^2:
    |sse - fsum| <= (M + 8) eps fsum,
the worst case of summing M non-negative terms in any order plus four roundings per term, with no
margin on top.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
N = 128
# a Feller-satisfying point (sigma^2 < 2 kappa theta on both factors)
MODEL = np.array([0.04, 2.5, 0.045, 0.3, -0.7, 0.035, 0.6, 0.05, 0.2, -0.5, 0.15, -0.04, 0.08])


@pytest.fixture(scope="module")
def dh():
    import dhcos
    from dhcos import _native
    if _native.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return dhcos


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def make_surface(M):
    """M options over 2-3 unsorted maturities (perm is not the identity), calls and puts in and out
    of the money, with random non-uniform weights."""
    rng = np.random.RandomState(1000 + 7 * M)
    T = rng.choice([1.0, 0.5, 0.25] if M % 2 else [0.75, 0.4], size=M)
    if M >= 3:
        T[:3] = [1.0, 0.5, 1.0] if M % 2 else [0.75, 0.4, 0.75]
    K = np.round(rng.uniform(82.0, 118.0, size=M), 3)
    call = (rng.uniform(size=M) < 0.5).astype(np.int8)
    w = rng.uniform(0.25, 4.0, size=M)
    return K, T, call, w


def records(S, pct=False):
    """Records spread as tests/test_gpu_iv.py::test_surface_form spreads them."""
    from dhcos import _native
    rec = np.empty((S, _native.PARAM_STRIDE))
    rec[:, :13] = MODEL * (1.0 + 0.02 * np.arange(S))[:, None]
    rec[:, 13] = 100.0 + (0.5 * np.arange(S) if pct else 0.0)
    rec[:, 14] = 0.03 + 0.001 * np.arange(S)
    rec[:, 15] = 0.001 * np.arange(S)
    return rec


def sse_bound(M, fsum):
    return (M + 8) * EPS * fsum


def host_sse(iv_row, mkt_iv, w):
    sel = w > 0
    return math.fsum((w[sel] * (iv_row[sel] - mkt_iv[sel]) ** 2).tolist())


CASES = [(M, S, False) for M in (1, 64, 65, 257, 600) for S in (1, 15)] + [(65, 15, True)]


@pytest.mark.parametrize("M,S,pct", CASES)
def test_against_the_parts(dh, M, S, pct):
    from dhcos import _native
    K, T, call, w = make_surface(M)
    rec = records(S, pct)
    rng = np.random.RandomState(M + S)
    ctx = _native.default_context()
    surf = _native.Surface(ctx, K, T, call,
                           strike_mode=_native.STRIKE_PCT_SPOT if pct else _native.STRIKE_ABSOLUTE)
    try:
        want_iv, want_prices = surf.implied_vol(rec, N, want_prices=True)
        assert np.all(np.isfinite(want_iv)) and np.all(want_iv > 0.01)
        assert same_bits(want_prices, surf.price(rec, N))
        mkt_iv = want_iv[0] + rng.uniform(-0.03, 0.03, size=M)
        assert np.all(mkt_iv > 0)
        surf.set_iv_market(mkt_iv, w)
        sse, bad, prices, iv = surf.loss_terms_iv(rec, N, want_prices=True, want_iv=True)
        sse2, bad2 = surf.loss_terms_iv(rec, N)
    finally:
        surf.close()
    assert sse.shape == (S,) and bad.shape == (S,) and bad.dtype == np.int32
    assert same_bits(iv, want_iv)
    assert same_bits(prices, want_prices)
    assert np.all(bad == 0) and np.all(bad2 == 0)
    assert same_bits(sse, sse2)
    fs = np.array([host_sse(want_iv[s], mkt_iv, w) for s in range(S)])
    print(f"M {M} S {S}: worst |sse - fsum| / (eps fsum) = "
          f"{np.max(np.abs(sse - fs) / (EPS * fs)):.3g} (bar {M + 8})")
    for s in range(S):
        assert fs[s] > 0 and abs(sse[s] - fs[s]) <= sse_bound(M, fs[s]), (s, sse[s], fs[s])


def test_stage_on_crafted_prices(dh):
    """dh_surface_iv_sse_dev alone, on torch tensors and a non-default stream.  r = q = 0: the
    discounted legs are S0 and K themselves, so the bounds are exact."""
    import torch
    from dhcos import _native, implied_vol
    M, S, S0 = 70, 2, 100.0
    rng = np.random.RandomState(70)
    T = rng.choice([0.5, 1.0, 0.25], size=M)
    T[:3] = [1.0, 0.5, 1.0]
    K = np.round(rng.uniform(85.0, 115.0, size=M), 2)
    call = (rng.uniform(size=M) < 0.5).astype(np.int8)
    w = rng.uniform(0.25, 4.0, size=M)
    rec = records(S)
    rec[:, 13], rec[:, 14], rec[:, 15] = S0, 0.0, 0.0
    # columns 0..7 of set 0 are crafted: in-the-money calls at K = 80, puts at K = 120
    K[:8] = [80.0, 80.0, 120.0, 100.0, 100.0, 100.0, 100.0, 100.0]
    call[:8] = [1, 1, 0, 1, 0, 1, 0, 1]
    w[7] = 0.0
    ctx = _native.default_context()
    surf = _native.Surface(ctx, K, T, call)
    try:
        good = surf.price(rec, N)
        good_iv = implied_vol(good, S0, K[None, :], T[None, :], 0.0, 0.0, call[None, :] != 0)
        assert np.all(np.isfinite(good_iv)) and np.all(good_iv > 0.01)
        prices = good.copy()
        prices[0, 0] = np.nextafter(20.0, 0.0)     # one ulp below intrinsic: iv 0.0, not bad
        prices[0, 1] = 100.0                       # call: == upper (S0)           bad
        prices[0, 2] = 125.0                       # put: > upper (K = 120)        bad
        prices[0, 3] = np.nan                      #                                bad
        prices[0, 4] = np.inf                      #                                bad
        prices[0, 5] = -1.0                        #                                bad
        prices[0, 6] = 0.0                         #                                bad
        prices[0, 7] = np.nan                      # weight 0: not counted
        n_bad_cols = 6
        mkt_iv = good_iv[1] + rng.uniform(-0.02, 0.02, size=M)
        surf.set_iv_market(mkt_iv, w)
        dev = torch.device("cuda", ctx.device)
        d_rec = torch.from_numpy(rec).to(dev)
        d_prices = torch.from_numpy(prices).to(dev)
        d_sse = torch.full((S,), -1.0, dtype=torch.float64, device=dev)
        d_bad = torch.full((S,), -7, dtype=torch.int32, device=dev)
        d_iv = torch.full((S, M), -1.0, dtype=torch.float64, device=dev)
        stream = torch.cuda.Stream(device=dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        assert stream.cuda_stream != 0
        with torch.cuda.stream(stream):
            surf.iv_sse_dev(d_rec.data_ptr(), d_prices.data_ptr(), S, d_sse.data_ptr(),
                            d_bad.data_ptr(), d_iv.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        sse, bad, iv = d_sse.cpu().numpy(), d_bad.cpu().numpy(), d_iv.cpu().numpy()
        # the same request without the vols
        with torch.cuda.stream(stream):
            surf.iv_sse_dev(d_rec.data_ptr(), d_prices.data_ptr(), S, d_sse.data_ptr(),
                            d_bad.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        assert same_bits(d_sse.cpu().numpy(), sse) and np.array_equal(d_bad.cpu().numpy(), bad)
    finally:
        surf.close()
    assert bad.tolist() == [n_bad_cols, 0]
    assert iv[0, 0] == 0.0 and not np.signbit(iv[0, 0])
    assert np.all(np.isnan(iv[0, 1:8]))
    assert same_bits(iv[0, 8:], good_iv[0, 8:]) and same_bits(iv[1], good_iv[1])
    used = np.zeros(M)
    used[0] = 0.0
    used[8:] = good_iv[0, 8:]
    w0 = w.copy()
    w0[1:8] = 0.0                                    # the bad columns leave the sum
    for s, (row, ww) in enumerate(((used, w0), (good_iv[1], w))):
        f = host_sse(row, mkt_iv, ww)
        print(f"set {s}: sse {sse[s]:.17g} fsum {f:.17g} |diff| / (eps fsum) = "
              f"{abs(sse[s] - f) / (EPS * f):.3g} (bar {M + 8})")
        assert np.isfinite(sse[s]) and abs(sse[s] - f) <= sse_bound(M, f), (s, sse[s], f)


def test_invariance(dh):
    from dhcos import _native
    M = 600
    K, T, call, w = make_surface(M)
    w[::7] = 0.0
    rec = records(42)
    ctx = _native.default_context()
    surf = _native.Surface(ctx, K, T, call)
    try:
        mkt_iv = surf.implied_vol(rec[:1], N)[0] + 0.01
        surf.set_iv_market(mkt_iv, w)
        batch = [surf.loss_terms_iv(rec, N) for _ in range(3)]
        alone = {s: surf.loss_terms_iv(rec[s:s + 1], N) for s in (0, 5, 41)}
        moved = surf.loss_terms_iv(np.roll(rec, 9, axis=0), N)
        broken = rec.copy()
        broken[17, 3] = np.nan
        hurt = surf.loss_terms_iv(broken, N)
        # the device-pointer form, pricing into the context's scratch
        import torch
        dev = torch.device("cuda", ctx.device)
        d_rec = torch.from_numpy(rec).to(dev)
        d_sse = torch.empty(42, dtype=torch.float64, device=dev)
        d_bad = torch.empty(42, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        surf.loss_iv_dev(d_rec.data_ptr(), 42, d_sse.data_ptr(), d_bad.data_ptr(), N=N)
        ctx.synchronize()
        dev_form = d_sse.cpu().numpy(), d_bad.cpu().numpy()
    finally:
        surf.close()
    sse, bad = batch[0]
    assert np.all(bad == 0) and np.all(sse > 0)
    for other in batch[1:]:                                  # three back-to-back calls
        assert same_bits(other[0], sse) and np.array_equal(other[1], bad)
    for s, (a_sse, a_bad) in alone.items():                  # alone against in a batch of 42
        assert same_bits(a_sse, sse[s:s + 1]) and np.array_equal(a_bad, bad[s:s + 1]), s
    assert same_bits(dev_form[0], sse) and np.array_equal(dev_form[1], bad)
    assert same_bits(moved[0], np.roll(sse, 9)) and np.array_equal(moved[1], np.roll(bad, 9))
    # a NaN parameter: every weighted option of that record is bad, its neighbours are unchanged
    keep = np.arange(42) != 17
    assert hurt[1][17] == int(np.count_nonzero(w > 0))
    assert same_bits(hurt[0][keep], sse[keep]) and np.array_equal(hurt[1][keep], bad[keep])


def test_validation(dh):
    from dhcos import _native
    K, T, call, w = make_surface(9)
    rec = records(2)
    ctx = _native.default_context()
    surf = _native.Surface(ctx, K, T, call)
    try:
        with pytest.raises(_native.NativeError, match="market vols"):
            surf.loss_terms_iv(rec, N)
        iv = np.full(9, 0.2)
        neg = w.copy()
        neg[4] = -1.0
        with pytest.raises(_native.NativeError):
            surf.set_iv_market(iv, neg)
        with pytest.raises(_native.NativeError):
            surf.set_iv_market(iv, np.zeros(9))
        hole = iv.copy()
        hole[2] = np.nan
        with pytest.raises(_native.NativeError):
            surf.set_iv_market(hole, w)
        with pytest.raises(_native.NativeError, match="market vols"):     # still none accepted
            surf.loss_terms_iv(rec, N)
        w0 = w.copy()
        w0[2] = 0.0
        surf.set_iv_market(hole, w0)                       # NaN at weight 0 is accepted
        sse, bad = surf.loss_terms_iv(rec, N)
        assert np.all(bad == 0) and np.all(np.isfinite(sse))
        surf.set_iv_market(iv)                             # replaces; weights default to 1
        sse1, bad1, got_iv = surf.loss_terms_iv(rec, N, want_iv=True)
        f = host_sse(got_iv[0], iv, np.ones(9))
        assert np.all(bad1 == 0) and abs(sse1[0] - f) <= sse_bound(9, f)
    finally:
        surf.close()


# ---- calibrator ----------------------------------------------------------------------------
def calib_market(dh, x_star, spot=100.0, r=0.03):
    """5 strikes x 3 maturities priced by the surface itself at x_star's records."""
    from dhcos import _native
    strikes = [90.0, 95.0, 100.0, 105.0, 110.0]
    opts = [{"strike": k, "maturity": t, "option_type": "call" if k >= 100.0 else "put",
             "price": 0.0} for t in (1.0, 0.25, 0.5) for k in strikes]
    probe = dh.DoubleHestonJumpCalibrator(spot, r, opts)
    _, rec = probe._records(x_star[None, :])
    surf = _native.Surface(_native.default_context(), [o["strike"] for o in opts],
                           [o["maturity"] for o in opts],
                           [o["option_type"] == "call" for o in opts])
    try:
        prices = surf.price(rec, N)[0]
    finally:
        surf.close()
    for o, p in zip(opts, prices):
        o["price"] = float(p)
    return opts


@pytest.fixture(scope="module")
def x_star(dh):
    cal = dh.DoubleHestonJumpCalibrator(100.0, 0.03, [])
    x = cal.inverse_transform_params(dict(zip(cal.param_names, MODEL)))
    from dhcos import calibrator as C
    assert C.feller_penalty(C.x_to_model(x[None, :]))[0] == 0.0
    return x


def test_calibrator_loss(dh, x_star):
    from dhcos import calibrator as C
    opts = calib_market(dh, x_star)
    w = np.linspace(0.5, 2.0, 15)
    cal = dh.DoubleHestonJumpCalibrator(100.0, 0.03, opts, objective="iv", iv_weights=w)
    assert cal.compute_loss(x_star) == 0.0
    assert np.array_equal(cal.loss_batch(np.tile(x_star, (14, 1))), np.zeros(14))
    assert cal.market_ivs.shape == (15,) and np.all(np.isfinite(cal.market_ivs))
    K, T = cal._option_arrays()
    want = dh.implied_vol(cal.market_prices, 100.0, K, T, 0.03, 0.0,
                          [o["option_type"] for o in opts])
    assert same_bits(cal.market_ivs, want)
    # fg_batch is fg_from_losses
    X0 = np.stack([x_star + 0.05, x_star - 0.02])
    f, g, low = cal.fg_batch(X0)
    wf, wg, wlow = C.fg_from_losses(cal, X0)
    assert same_bits(f, wf) and same_bits(g, wg) and same_bits(low, wlow)
    # a perturbed point against the host formula over Surface.implied_vol
    x = x_star + 0.05
    got = cal.compute_loss(x)
    P, rec = cal._records(x[None, :])
    iv = cal._get_surface().implied_vol(rec, N)[0]
    assert np.all(np.isfinite(iv))
    fs = host_sse(iv, cal.market_ivs, w)
    assert C.feller_penalty(P)[0] == 0.0
    print(f"loss {got:.17g} host {fs / w.sum():.17g}")
    assert got > 0 and abs(got - fs / w.sum()) <= sse_bound(15, fs) / w.sum()


def test_calibrator_runs_the_same_in_lockstep_and_in_sequence(dh, x_star):
    opts = calib_market(dh, x_star)
    x0s = [x_star + 0.05, x_star - 0.04]
    out = {}
    for lockstep in (True, False):
        cal = dh.DoubleHestonJumpCalibrator(100.0, 0.03, opts, objective="iv")
        start = cal.compute_loss(x0s[0])
        res = cal.calibrate(maxiter=30, multi_start=2, x0s=[x.copy() for x in x0s],
                            lockstep=lockstep)
        out[lockstep] = res
        assert np.isfinite(res.final_loss)
        assert res.final_loss < start, (res.final_loss, start)
        assert res.model_prices.shape == (15,)
    a, b = out[True], out[False]
    print(f"final loss {a.final_loss:.6e} after {a.iterations} iterations ({a.message})")
    assert same_bits([a.parameters[k] for k in a.parameters], [b.parameters[k] for k in b.parameters])
    assert same_bits(a.final_loss, b.final_loss) and a.iterations == b.iterations


def test_calibrator_market_vols(dh, x_star):
    opts = calib_market(dh, x_star)
    given = np.linspace(0.15, 0.3, 15)
    cal = dh.DoubleHestonJumpCalibrator(100.0, 0.03, opts, objective="iv", market_ivs=given)
    assert cal.compute_loss(x_star) > 0.0                  # not the inverted prices' zero
    assert same_bits(cal.market_ivs, given)
    # a market price below intrinsic: no vol, the option is named; weight 0 admits it
    broken = [dict(o) for o in opts]
    assert broken[0]["strike"] == 90.0 and broken[0]["option_type"] == "put"
    broken[10] = dict(broken[10], strike=60.0, option_type="call", price=39.0)   # S0 - K e^{-rT} > 39
    cal = dh.DoubleHestonJumpCalibrator(100.0, 0.03, broken, objective="iv")
    with pytest.raises(ValueError, match=r"\[10\]"):
        cal.compute_loss(x_star)
    with pytest.raises(ValueError, match=r"\[10\]"):       # and again: nothing was cached
        cal.compute_loss(x_star)
    w = np.ones(15)
    w[10] = 0.0
    cal = dh.DoubleHestonJumpCalibrator(100.0, 0.03, broken, objective="iv", iv_weights=w)
    assert np.isfinite(cal.compute_loss(x_star))
    assert np.isnan(cal.market_ivs[10])
