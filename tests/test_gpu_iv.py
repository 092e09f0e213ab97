"""GPU tests of the Black-Scholes implied volatility (csrc/dh_iv.h; dh_implied_vol,
dh_implied_vol_dev, dh_surface_implied_vol and the Python layer over them).

Truth: tests/golden/iv_truth.npz (tests/golden/make_iv_truth.py: 1,250 quotes priced in 60-digit
arithmetic from a known sigma).  Error unit per quote u = eps sigma_true + eps scale / vega: the
change of sigma that one ulp of the input price, or of the discounted bounds, already causes.
Bar: |sigma - sigma_true| <= yardstick u on every kept quote, where yardstick (5.5e3, stored in the
fixture) is the worst error, in the same unit on the same quotes, of SciPy brentq on the textbook
formula -- the host route a user has without the library.  No extra margin.
"""
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
KAT_PARITY = 4.87e-10        # the KAT's own call/put parity residual
COLS = ("price", "S0", "K", "T", "r", "q")


@pytest.fixture(scope="module")
def dh():
    import dhcos
    from dhcos import _native
    if _native.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return dhcos


@pytest.fixture(scope="module")
def truth():
    with np.load(os.path.join(GOLDEN, "iv_truth.npz")) as z:
        t = {k: z[k] for k in z.files}
    t["u"] = EPS * t["sigma_true"] + EPS * t["scale"] / t["vega"]
    t["bar"] = float(t["yardstick"]) * t["u"]
    return t


@pytest.fixture(scope="module")
def full(dh, truth):
    """The vols of the whole fixture, computed once (the other tests compare with its bits)."""
    t = truth
    out = dh.implied_vol(*(t[k] for k in COLS), option_type=t["is_call"] != 0)
    out.setflags(write=False)
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def bs_price(sigma, S0, K, T, r, q, call):
    """Textbook Black-Scholes on the CPU (math.erfc)."""
    sq = sigma * math.sqrt(T)
    d1 = (math.log(S0 / K) + (r - q + 0.5 * sigma * sigma) * T) / sq
    d2 = d1 - sq
    cdf = lambda x: 0.5 * math.erfc(-x / math.sqrt(2.0))     # noqa: E731
    A, B = S0 * math.exp(-q * T), K * math.exp(-r * T)
    vega = A * math.exp(-0.5 * d1 * d1) / math.sqrt(2.0 * math.pi) * math.sqrt(T)
    price = A * cdf(d1) - B * cdf(d2) if call else B * cdf(-d2) - A * cdf(-d1)
    return price, vega, A, B


def test_fixture_round_trip(truth, full):
    t, k = truth, truth["keep"]
    err = np.abs(full - t["sigma_true"])
    ratio = err / t["u"]
    w = int(np.argmax(np.where(k, ratio, 0.0)))
    print(f"kept {int(k.sum())}: worst |err| / u = {ratio[w]:.4g} at quote {w} (yardstick "
          f"{float(t['yardstick']):.4g}); median {np.median(ratio[k]):.3g}, 99% "
          f"{np.percentile(ratio[k], 99):.3g}")
    assert np.all(np.isfinite(full[k]))
    assert np.all(err[k] <= t["bar"][k]), (w, ratio[w])
    rest = full[~k]               # time value below the fp64 price's resolution: any of these
    assert np.all(np.isnan(rest) | (np.isfinite(rest) & (rest >= 0.0)))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 1000])
def test_tail_and_position(dh, truth, full, n):
    t = truth
    ic = t["is_call"] != 0
    got = dh.implied_vol(*(t[k][:n] for k in COLS), option_type=ic[:n])
    assert got.shape == (n,)
    assert same_bits(got, full[:n])
    perm = np.random.RandomState(n).permutation(n)
    got = dh.implied_vol(*(t[k][:n][perm] for k in COLS), option_type=ic[:n][perm])
    assert same_bits(got, full[:n][perm])


def test_edges(dh):
    S0, r, q, T = 100.0, 0.03, 0.01, 0.5
    A = S0 * np.exp(-q * T)

    def B(K):
        return K * np.exp(-r * T)
    nan, inf = float("nan"), float("inf")
    good = dict(price=6.0, S0=S0, K=100.0, T=T, r=r, q=q, call=True)
    # rows that sit exactly on a bound take r = q = 0, so that the discounted legs are S0 and K in
    # any exp's rounding and the comparison with the bound is exact
    z = dict(r=0.0, q=0.0)
    rows = [
        # price == lower -> 0.0
        (dict(z, price=20.0, K=80.0, call=True), 0.0),              # in-the-money call, intrinsic
        (dict(z, price=20.0, K=120.0, call=False), 0.0),            # in-the-money put
        (dict(price=0.0, K=120.0, call=True), 0.0),                 # price 0 out of the money
        (dict(price=0.0, K=80.0, call=False), 0.0),
        # NaN
        (dict(price=-1.0), nan), (dict(price=-0.5, K=120.0), nan),
        (dict(z, price=np.nextafter(20.0, 0.0), K=80.0), nan),      # just below intrinsic
        (dict(z, price=100.0), nan), (dict(z, price=200.0), nan),   # call: upper = S0 e^{-qT}
        (dict(z, price=100.0, call=False), nan), (dict(z, price=200.0, call=False), nan),
        (dict(price=1.5 * A), nan), (dict(price=1.5 * B(100.0), call=False), nan),
        (dict(price=nan), nan), (dict(price=inf), nan), (dict(price=-inf), nan),
        (dict(T=0.0), nan), (dict(T=-1.0), nan), (dict(K=0.0), nan), (dict(K=-5.0), nan),
        (dict(S0=0.0), nan), (dict(S0=nan), nan), (dict(r=nan), nan), (dict(q=nan), nan),
        (dict(T=nan), nan), (dict(K=nan), nan),
    ]
    alone = dh.implied_vol(good["price"], S0, 100.0, T, r, q, "C")
    assert isinstance(alone, np.float64) and 0.15 < alone < 0.3
    # every edge row between finite neighbours, all in one wave
    quotes, want = [], []
    for over, w in rows:
        quotes += [dict(good, **over), good]
        want += [w, float(alone)]
    cols = {k: np.array([x[k] for x in quotes], dtype=np.float64) for k in COLS}
    got = dh.implied_vol(*(cols[k] for k in COLS), option_type=[x["call"] for x in quotes])
    assert len(quotes) <= 64
    for i, (g, w) in enumerate(zip(got, want)):
        if math.isnan(w):
            assert math.isnan(g), (i, quotes[i], g)
        else:
            assert same_bits(g, w), (i, quotes[i], g, w)


def test_call_put_agreement(truth, full):
    t = truth
    c, p = np.arange(0, t["price"].size, 2), np.arange(1, t["price"].size, 2)
    both = t["keep"][c] & t["keep"][p]
    assert both.sum() > 400
    diff = np.abs(full[c] - full[p])[both]
    bar = (t["bar"][c] + t["bar"][p])[both]
    print(f"{int(both.sum())} kept pairs: worst |call vol - put vol| / (sum of bars) = "
          f"{np.max(diff / bar):.3g}")
    assert np.all(diff <= bar)


def test_model_vols(dh, kat, truth):
    e = kat["prices"][0]
    assert e["T"] == 1.0 and e["S0"] == 100.0
    yard = float(truth["yardstick"])
    for K in (90.0, 95.0, 100.0, 105.0, 110.0):
        vols, bars, vegas = {}, {}, {}
        for ot in ("C", "P"):
            m = dh.DoubleHeston(e["S0"], K, e["T"], e["r"], *e["params"], option_type=ot, q=e["q"])
            price, sigma = m.pricing(128), m.implied_vol(128)
            assert isinstance(sigma, np.float64) and 0.05 < sigma < 1.0, (K, ot, sigma)
            call = ot == "C"
            back, vega, A, B = bs_price(float(sigma), e["S0"], K, e["T"], e["r"], e["q"], call)
            lower = max(A - B, 0.0) if call else max(B - A, 0.0)
            scale = price if lower == 0.0 else max(price, A, B)
            print(f"K {K} {ot}: price {price:.12f} vol {sigma:.15f} reprice error "
                  f"{abs(back - price):.3e} (bar {yard * EPS * scale:.3e})")
            assert abs(back - price) <= yard * EPS * scale, (K, ot, back, price)
            vols[ot], vegas[ot] = float(sigma), vega
            bars[ot] = yard * (EPS * float(sigma) + EPS * scale / vega)
        assert abs(vols["C"] - vols["P"]) <= bars["C"] + bars["P"] + KAT_PARITY / vegas["C"], \
            (K, vols)
    # the batch form: price_batch's prices, inverted
    Ks = np.array([90.0, 100.0, 110.0, 95.0])
    ots = ["C", "P", "C", "P"]
    vb = dh.DoubleHeston.implied_vol_batch(e["params"], e["S0"], Ks, e["T"], e["r"], ots, q=e["q"])
    pb = dh.DoubleHeston.price_batch(e["params"], e["S0"], Ks, e["T"], e["r"], ots, q=e["q"])
    assert same_bits(vb, dh.implied_vol(pb, e["S0"], Ks, e["T"], e["r"], e["q"], ots))


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("mode", ["absolute", "pct_spot"])
def test_surface_form(dh, kat, P, mode):
    from dhcos import _native
    e = kat["prices"][0]
    # M = 7 over 2 maturities, unsorted: the surface's maturity sort (perm) is not the identity
    T = np.array([1.0, 0.5, 1.0, 0.5, 0.5, 1.0, 0.5])
    K = np.array([105.0, 90.0, 95.0, 110.0, 100.0, 85.0, 97.5])
    call = np.array([1, 0, 1, 1, 0, 0, 1], dtype=np.int8)
    pct = mode == "pct_spot"
    rec = np.empty((P, _native.PARAM_STRIDE))
    rec[:, :13] = np.asarray(e["params"]) * (1.0 + 0.05 * np.arange(P))[:, None]
    rec[:, 13] = 100.0 + 7.0 * np.arange(P) if pct else 100.0     # distinct S0 under PCT_SPOT
    rec[:, 14] = 0.03 + 0.01 * np.arange(P)
    rec[:, 15] = 0.01 * np.arange(P)
    ctx = _native.default_context()
    surf = _native.Surface(ctx, K, T, call,
                           strike_mode=_native.STRIKE_PCT_SPOT if pct else _native.STRIKE_ABSOLUTE)
    try:
        want_prices = surf.price(rec, 128)
        iv, prices = surf.implied_vol(rec, 128, want_prices=True)
        iv_only = surf.implied_vol(rec, 128)
    finally:
        surf.close()
    assert same_bits(prices, want_prices)
    S0 = rec[:, 13][:, None]
    strikes = K[None, :] * S0 / 100.0 if pct else np.broadcast_to(K, (P, 7))
    want = dh.implied_vol(want_prices, S0, strikes, T[None, :], rec[:, 14][:, None],
                          rec[:, 15][:, None], call[None, :] != 0)
    assert want.shape == (P, 7) and np.all(np.isfinite(want)) and np.all(want > 0.05)
    assert same_bits(iv, want)
    assert same_bits(iv_only, want)


def test_device_pointer_form(dh, truth, full):
    import torch
    from dhcos import _native
    t = truth
    ctx = _native.default_context()
    dev = torch.device("cuda", ctx.device)
    cols = [torch.from_numpy(np.ascontiguousarray(t[k])).to(dev) for k in COLS]
    ic = torch.from_numpy(np.ascontiguousarray(t["is_call"], dtype=np.int8)).to(dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    assert stream.cuda_stream != 0
    with torch.cuda.stream(stream):
        out = ctx.implied_vol_dev(*cols, ic, stream=stream)
        out2 = torch.empty_like(out)
        ctx.implied_vol_dev(*cols, ic, out=out2, stream=stream.cuda_stream)   # the raw handle
    stream.synchronize()
    assert same_bits(out.cpu().numpy(), full)
    assert same_bits(out2.cpu().numpy(), full)
    out3 = ctx.implied_vol_dev(*cols, ic)                      # the context's own stream
    ctx.synchronize()
    assert same_bits(out3.cpu().numpy(), full)
    with pytest.raises(ValueError):                            # the null stream cannot be named
        ctx.implied_vol_dev(*cols, ic, stream=torch.cuda.default_stream(dev))


def test_generator_columns(dh):
    from dhcos import generator as G
    np.random.seed(11)
    st = np.random.get_state()
    base = G.generate_synthetic_calibrations(7, None, as_arrays=True, verbose=False)
    after_base = np.random.random(3)
    np.random.set_state(st)
    got = G.generate_synthetic_calibrations(7, None, as_arrays=True, verbose=False,
                                            implied_vols=True)
    assert np.array_equal(np.random.random(3), after_base)
    assert set(got) == set(base) | {"market_iv", "model_iv"}
    for k, v in base.items():
        if isinstance(v, np.ndarray) and v.dtype == np.float64:
            assert same_bits(got[k], v), k
        else:
            assert np.array_equal(got[k], v), k
    spot = got["spot"][:, None]
    for name in ("market", "model"):
        want = dh.implied_vol(got[name + "_prices"], spot, got["strikes"], got["maturities"],
                              got["risk_free"], 0.0, "C")
        assert got[name + "_iv"].shape == (7, 15)
        assert same_bits(got[name + "_iv"], want), name
    assert np.all(np.isfinite(got["model_iv"])) and np.all(got["model_iv"] > 0.05)
    with pytest.raises(ValueError):
        G.generate_synthetic_calibrations(7, None, as_arrays=False, verbose=False,
                                          implied_vols=True)
