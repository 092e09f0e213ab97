"""Wrapper-level behaviour of the ctypes binding (dhcos/_native.py) that its shared marshalling
helpers own: the ``out=`` check, the loss wrappers' return tuples, the L-BFGS-B scaffold at zero
and one start, the stream argument, the FD ``model`` check and np.random's state across
gen_device.  The smallest shapes that reach each: 3 options over 2 maturities (two tiles), N = 64,
two param records from the golden one of tests/golden/kat.json.  Nothing here is timed."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 64
K = np.array([95.0, 100.0, 105.0])
T = np.array([0.5, 0.5, 1.0])
IS_CALL = np.array([1, 0, 1], dtype=np.int8)
LB = dict(maxiter=1)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.fixture(scope="module")
def nat():
    from dhcos import _native
    if _native.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return _native


@pytest.fixture(scope="module")
def case(nat, kat):
    """The golden record and a neighbour (spot 102) as records [2, 16], their model params [2, 13]
    and spots; a surface of the three options whose market is the golden record's prices 1% up,
    with that market's vols set; a second market for the row-wise wrappers."""
    e = kat["prices"][0]
    rec = np.array([e["params"] + [e["S0"], e["r"], e["q"]],
                    e["params"] + [102.0, e["r"], e["q"]]])
    ctx = nat.default_context()
    plain = nat.Surface(ctx, K, T, IS_CALL)
    prices = plain.price(rec, N)
    plain.close()
    mkt = np.stack([1.01 * prices[0], 0.99 * prices[1]])            # [B = 2, M = 3]
    surf = nat.Surface(ctx, K, T, IS_CALL, mkt=mkt[0])
    assert surf.M == 3 and surf.n_tiles == 2
    spots = rec[:, 13].copy()
    mkt_iv = ctx.implied_vol(mkt.ravel(), np.repeat(spots, 3), np.tile(K, 2), np.tile(T, 2),
                             np.full(6, e["r"]), np.zeros(6), np.tile(IS_CALL, 2)).reshape(2, 3)
    assert np.all(np.isfinite(mkt_iv))
    surf.set_iv_market(mkt_iv[0])
    x0 = np.zeros((1, 13))                                           # an unconstrained start
    yield dict(ctx=ctx, surf=surf, rec=rec, prices=prices, mkt=mkt, mkt_iv=mkt_iv, spots=spots,
               r=e["r"], x0=x0)
    surf.close()


def bad_outs():
    return {"dtype": np.full((2, 3), -1.0, dtype=np.float32),
            "shape": np.full((3, 2), -1.0),
            "non-contiguous": np.full((2, 6), -1.0)[:, ::2],
            "read-only": np.full((2, 3), -1.0)}


@pytest.mark.parametrize("method", ["price", "price_cols"])
def test_out_argument(nat, case, method):
    """A valid ``out`` comes back as the same object with the bits of the out=None call; a wrong
    dtype, a wrong shape, a non-contiguous or a read-only array is a ValueError with the
    wrapper's message before any call (``out`` unchanged)."""
    surf, rec = case["surf"], case["rec"]
    if method == "price":
        def call(out=None):
            return surf.price(rec, N, out=out)
    else:
        def call(out=None):
            return surf.price_cols(rec[:, :13], case["spots"], case["r"], N, out=out)
    want = call()
    assert want.shape == (2, 3) and np.all(np.isfinite(want))
    out = np.full((2, 3), -1.0)
    assert call(out) is out and same_bits(out, want)
    for what, bad in bad_outs().items():
        if what == "read-only":
            bad.setflags(write=False)
        with pytest.raises(ValueError, match=r"out must be a writeable C-contiguous float64 "
                                             r"\[2, 3\]"):
            call(bad)
        assert np.all(bad == -1.0), what


@pytest.mark.parametrize("rows", [False, True])
def test_vol_space_loss_return_tuples(case, rows):
    """loss_terms_iv / loss_terms_iv_rows return (sse, n_bad[, prices][, iv]): 2, 3, 3 and 4
    members over the want_prices / want_iv combinations, every member the same bits in each."""
    surf, rec = case["surf"], case["rec"]

    def call(**kw):
        if rows:
            return surf.loss_terms_iv_rows(rec, case["mkt_iv"], [1, 0], N, **kw)
        return surf.loss_terms_iv(rec, N, **kw)
    both = call(want_prices=True, want_iv=True)
    assert len(both) == 4
    sse, bad, prices, iv = both
    assert sse.shape == (2,) and bad.dtype == np.int32 and bad.shape == (2,)
    assert prices.shape == iv.shape == (2, 3)
    none = call()
    only_p = call(want_prices=True)
    only_iv = call(want_iv=True)
    assert (len(none), len(only_p), len(only_iv)) == (2, 3, 3)
    for got in (none, only_p, only_iv):
        assert same_bits(got[0], sse) and np.array_equal(got[1], bad)
    assert same_bits(only_p[2], prices) and same_bits(only_iv[2], iv)


def test_price_space_loss_return_tuples(case):
    """loss_terms / loss_terms_rows return three members, prices None unless asked for."""
    surf, rec = case["surf"], case["rec"]
    for call in (lambda **kw: surf.loss_terms(rec, N, **kw),
                 lambda **kw: surf.loss_terms_rows(rec, case["mkt"], [1, 0], N, **kw)):
        sse, bad, prices = call()
        assert prices is None and sse.shape == (2,) and bad.dtype == np.int32
        sse2, bad2, prices = call(want_prices=True)
        assert prices.shape == (2, 3) and np.all(np.isfinite(prices))
        assert same_bits(sse2, sse) and np.array_equal(bad2, bad)


def lbfgs_calls(case):
    """The three L-BFGS-B wrappers as functions of the start points x0s [S, 13] (start i on
    market 0)."""
    surf, c = case["surf"], case
    zeros = lambda x0s: np.zeros(len(x0s), dtype=np.int32)          # noqa: E731
    return {
        "calibrate_lbfgs": lambda x0s: surf.calibrate_lbfgs(x0s, c["spots"][0], c["r"], N, **LB),
        "calibrate_lbfgs_batch": lambda x0s: surf.calibrate_lbfgs_batch(
            c["mkt"], c["spots"], [c["r"]] * 2, x0s, zeros(x0s), N, **LB),
        "calibrate_lbfgs_batch_iv": lambda x0s: surf.calibrate_lbfgs_batch_iv(
            c["mkt_iv"], None, c["spots"], [c["r"]] * 2, x0s, zeros(x0s), N, **LB),
    }


@pytest.mark.parametrize("name", ["calibrate_lbfgs", "calibrate_lbfgs_batch",
                                  "calibrate_lbfgs_batch_iv"])
def test_lbfgs_zero_and_one_start(nat, case, name):
    """No start: ([], n) without error (the result array still has one element to point at).  One
    start, maxiter = 1: one LbResult that evaluated x0 at least."""
    call = lbfgs_calls(case)[name]
    res, n = call(np.empty((0, 13)))
    assert res == [] and isinstance(n, int)
    res, n = call(case["x0"])
    assert len(res) == 1 and isinstance(res[0], nat.LbResult) and res[0].nfev >= 1
    assert n >= 1


def test_mc_price_dev_stream_argument(nat, case):
    """mc_price_dev refuses torch's default (null) stream, as implied_vol_dev does; on the
    context's own stream (None) its prices are mc_price's, bit for bit."""
    import torch
    ctx, rec = case["ctx"], case["rec"][:1]
    opts = (nat.McOption * 1)(nat.McOption(nat.MC_KINDS["european"], 1, 100.0, 0.5, 0.0))
    dev = torch.device("cuda", ctx.device)
    d_rec = torch.from_numpy(rec).to(dev)
    with pytest.raises(ValueError, match=r"mc_price_dev: the default \(null\) stream cannot be "
                                         r"named"):
        ctx.mc_price_dev(d_rec, opts, 1024, 8, 7, stream=torch.cuda.default_stream(dev))
    d_price, d_err = ctx.mc_price_dev(d_rec, opts, 1024, 8, 7)
    ctx.synchronize()
    price, err = ctx.mc_price(rec, opts, 1024, 8, 7)
    assert same_bits(d_price.cpu().numpy(), price) and same_bits(d_err.cpu().numpy(), err)


def test_fd_model_shape(nat, case):
    """A ``model`` that is not [2, S, 13] is a ValueError from fg and from fg_begin, and the
    refused fg_begin leaves its slot idle: fg_end on it is the library's error."""
    surf, x0 = case["surf"], case["x0"]
    wrong = np.zeros((2, 2, 13))
    with pytest.raises(ValueError, match=r"model must be \[2, 1, 13\], got \(2, 2, 13\)"):
        surf.fg(x0, case["spots"][0], case["r"], N, model=wrong)
    with pytest.raises(ValueError, match=r"model must be \[2, 1, 13\], got \(2, 2, 13\)"):
        surf.fg_begin(x0, case["spots"][0], case["r"], N, model=wrong, slot=1)
    assert case["ctx"]._fg_s[1] is None
    with pytest.raises(nat.NativeError):
        surf.fg_end(1)


def test_gen_device_leaves_the_host_draws_rng_state(nat, case):
    """gen_device, 4 samples on a 3-option grid in percent of spot: np.random's next five doubles
    are those that follow the generator's host draw (dh_gen_draw) from the same seed, and the
    drawn params and spots are that draw's."""
    from dhcos import generator as G
    pct, mat = np.array([95.0, 100.0, 105.0]), np.array([0.5])
    np.random.seed(12)
    params, spots, _ = G.draw_paths(4, strikes=pct, maturities=mat)
    want = np.random.random_sample(5)
    grid = nat.Surface(case["ctx"], pct, np.repeat(mat, 3), np.ones(3, dtype=np.int8),
                       strike_mode=nat.STRIKE_PCT_SPOT)
    try:
        lo, hi = G._ranges()
        np.random.seed(12)
        out = nat.gen_device(grid, 4, lo, hi, G.ALPHA, G.SPOT_BASE, 0.0003, 0.01, 0.02,
                             G.RISK_FREE, pct, N=N)
        got = np.random.random_sample(5)
    finally:
        grid.close()
    assert np.array_equal(got, want)
    assert same_bits(out["params"], params) and same_bits(out["spots"], spots)
    assert out["dates"] is None and out["market"].shape == (4, 3)
