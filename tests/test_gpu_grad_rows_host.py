"""GPU tests of the analytic rows request's shared host path (csrc/dh_param_grad.h:
rows_round_trip, rows_request_dev) behind dh_surface_loss_grad_rows*,
dh_surface_gauss_newton_rows* and dh_surface_loss_iv_grad_rows*:

  1. the host form's f, g, bad and extra output (H, or the vols as used) are the _dev form's bits
     on the same inputs -- S = 5 sets on B = 3 markets, row = [2, 0, 2, 1, 0] (S != B, unsorted,
     repeated, a second 4-set block), M = 65 (a 13 x 5 grid: a second pass with one live lane),
     N = 32; the vol family without weights and with a [B, M] weight array holding one zero;
  2. every pointer an entry point needs, set to NULL one at a time, fails with "<name> is null",
     and a bad row, spot or rate with its message; several wrong arguments fail in the order of
     the checks: N, the pointers, the rows, spot and rate market by market, then the weights."""
import numpy as np
import pytest

from oracle import dh_oracle as O

pytestmark = pytest.mark.gpu

LO = np.array([0.025, 1.5, 0.025, 0.2, -0.85, 0.02, 0.3, 0.025, 0.1, -0.7, 0.05, -0.08, 0.03])
HI = np.array([0.08, 4.5, 0.065, 0.5, -0.4, 0.07, 1.2, 0.07, 0.35, -0.2, 0.25, -0.01, 0.12])
N, M, S, B = 32, 65, 5, 3
ROW = np.array([2, 0, 2, 1, 0], dtype=np.int32)


@pytest.fixture(scope="module")
def native():
    from dhcos import _native
    if _native.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return _native


@pytest.fixture(scope="module")
def case(native):
    """The surface, the shared inputs (prices and their vols as the markets) and device copies."""
    import torch
    ctx = native.default_context()
    k, t = np.linspace(82.0, 118.0, 13), np.linspace(0.2, 2.0, 5)
    surf = native.Surface(ctx, np.tile(k, t.size), np.repeat(t, k.size), np.ones(M, dtype=bool),
                          strike_mode=native.STRIKE_ABSOLUTE)
    rs = np.random.RandomState(65)
    spots, rates = np.array([97.0, 103.5, 100.0]), np.array([0.02, 0.04, 0.03])
    X = np.stack([O.from_params(LO + (HI - LO) * rs.rand(13)) for _ in range(S)])
    base = np.zeros((B, 16))
    base[:, :13] = LO + (HI - LO) * rs.rand(B, 13)
    base[:, 13], base[:, 14] = spots, rates
    mkt = surf.price(base, 128) * (1 + 0.02 * rs.randn(B, M))
    mkt_iv = surf.implied_vol(base, 128) * (1 + 0.02 * rs.randn(B, M))
    assert np.all(np.isfinite(mkt_iv)) and np.all(mkt_iv > 0)
    dev = torch.device("cuda", ctx.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = {"f": torch.empty(S, dtype=torch.float64, device=dev),
           "g": torch.empty((S, 13), dtype=torch.float64, device=dev),
           "bad": torch.empty(S, dtype=torch.int32, device=dev),
           "H": torch.empty((S, 13, 13), dtype=torch.float64, device=dev),
           "iv": torch.empty((S, M), dtype=torch.float64, device=dev)}
    yield dict(surf=surf, ctx=ctx, X=X, mkt=mkt, mkt_iv=mkt_iv, spots=spots, rates=rates,
               d={n: up(a) for n, a in (("X", X), ("mkt", mkt), ("mkt_iv", mkt_iv),
                                        ("spots", spots), ("rates", rates), ("row", ROW))},
               out=out, up=up)
    surf.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def on_stream(case, call):
    import torch
    dev = torch.device("cuda", case["ctx"].device)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        call(stream.cuda_stream)
    stream.synchronize()
    return {n: a.cpu().numpy() for n, a in case["out"].items()}


def test_price_host_form_is_dev_form(case):
    c, d, o = case, case["d"], case["out"]
    f, g, bad = c["surf"].loss_grad_rows(c["X"], c["mkt"], c["spots"], c["rates"], ROW, N)
    got = on_stream(c, lambda st: c["surf"].loss_grad_rows_dev(
        d["X"].data_ptr(), d["mkt"].data_ptr(), d["spots"].data_ptr(), d["rates"].data_ptr(),
        d["row"].data_ptr(), S, o["f"].data_ptr(), o["g"].data_ptr(), o["bad"].data_ptr(), N=N,
        stream=st))
    assert np.all(np.isfinite(f)) and np.all(np.isfinite(g)) and not bad.any()
    assert same_bits(got["f"], f) and same_bits(got["g"], g) and np.array_equal(got["bad"], bad)


def test_gauss_newton_host_form_is_dev_form(case):
    c, d, o = case, case["d"], case["out"]
    f, g, bad, H = c["surf"].gauss_newton_rows(c["X"], c["mkt"], c["spots"], c["rates"], ROW, N)
    got = on_stream(c, lambda st: c["surf"].gauss_newton_rows_dev(
        d["X"].data_ptr(), d["mkt"].data_ptr(), d["spots"].data_ptr(), d["rates"].data_ptr(),
        d["row"].data_ptr(), S, o["f"].data_ptr(), o["g"].data_ptr(), o["bad"].data_ptr(),
        o["H"].data_ptr(), N=N, stream=st))
    assert np.all(np.isfinite(H)) and H.any() and not bad.any()
    assert same_bits(got["f"], f) and same_bits(got["g"], g) and np.array_equal(got["bad"], bad)
    assert same_bits(got["H"], H)


@pytest.mark.parametrize("weighted", [False, True])
def test_vol_host_form_is_dev_form(case, weighted):
    c, d, o = case, case["d"], case["out"]
    w = np.ones((B, M))
    if weighted:
        w = 0.5 + np.random.RandomState(7).rand(B, M)
        w[2, 31] = 0.0
    f, g, bad, iv = c["surf"].loss_iv_grad_rows(c["X"], c["mkt_iv"], w if weighted else None,
                                               c["spots"], c["rates"], ROW, N)
    # the divisor as the host form makes it: each market's weights summed in option order from 0.0
    wsum = np.zeros(B)
    for m in range(M):
        wsum = wsum + w[:, m]
    d_w, d_div = c["up"](w), c["up"](wsum[ROW])
    got = on_stream(c, lambda st: c["surf"].loss_iv_grad_rows_dev(
        d["X"].data_ptr(), d["mkt_iv"].data_ptr(), d_w.data_ptr(), d_div.data_ptr(),
        d["spots"].data_ptr(), d["rates"].data_ptr(), d["row"].data_ptr(), S, o["f"].data_ptr(),
        o["g"].data_ptr(), o["bad"].data_ptr(), o["iv"].data_ptr(), N=N, stream=st))
    assert np.all(np.isfinite(f)) and np.all(np.isfinite(g)) and not bad.any()
    assert same_bits(got["f"], f) and same_bits(got["g"], g) and np.array_equal(got["bad"], bad)
    assert same_bits(got["iv"], iv)


# ---- error messages: the families' host and _dev symbols through the raw library ------------------
HOST_PRICE = ["x", "mkt", "spot", "rate", "row", "f", "g", "bad"]
FAMILIES = {
    # symbol: (pointer names in argument order, host or _dev form, pointers that may be NULL)
    "dh_surface_loss_grad_rows": (HOST_PRICE, "host", ()),
    "dh_surface_loss_grad_rows_dev": (HOST_PRICE, "dev", ()),
    "dh_surface_gauss_newton_rows": (HOST_PRICE + ["H"], "host", ()),
    "dh_surface_gauss_newton_rows_dev": (HOST_PRICE + ["H"], "dev", ()),
    "dh_surface_loss_iv_grad_rows": (["x", "mkt_iv", "wgt", "spot", "rate", "row", "f", "g",
                                      "bad", "iv"], "host", ("wgt", "iv")),
    "dh_surface_loss_iv_grad_rows_dev": (["x", "mkt_iv", "wgt", "div", "spot", "rate", "row", "f",
                                          "g", "bad", "iv"], "dev", ("iv",)),
}
INPUTS = {"x", "mkt", "mkt_iv", "wgt", "div", "spot", "rate", "row"}


def raw_call(native, case, symbol, null=(), n=N, **replace):
    """Call `symbol` with valid arguments but the pointers named in `null` NULL and the host
    arrays in `replace` in place of the valid ones -> the NativeError's text ("" on success)."""
    names, form, _ = FAMILIES[symbol]
    host = {"x": case["X"], "mkt": case["mkt"], "mkt_iv": case["mkt_iv"], "wgt": np.ones((B, M)),
            "div": np.full(S, float(M)), "spot": case["spots"], "rate": case["rates"], "row": ROW,
            "f": np.empty(S), "g": np.empty((S, 13)), "bad": np.empty(S, dtype=np.int32),
            "H": np.empty((S, 13, 13)), "iv": np.empty((S, M))}
    host.update(replace)
    if form == "host":
        keep = {k: np.ascontiguousarray(v) for k, v in host.items()}
        addr = {k: v.ctypes.data for k, v in keep.items()}
    else:
        keep = {k: case["up"](v) for k, v in host.items()}
        addr = {k: v.data_ptr() for k, v in keep.items()}
    ptrs = [None if k in null else addr[k] for k in names]
    n_in = sum(k in INPUTS for k in names)
    ints = [S, B, n, 10.0] if form == "host" else [S, n, 10.0]
    args = ptrs[:n_in] + ints + ptrs[n_in:] + ([None] if form == "dev" else [])
    try:
        native._check(getattr(native.load(), symbol)(case["ctx"].handle, case["surf"].handle,
                                                     *args))
    except native.NativeError as e:
        return str(e)
    if form == "dev":                                  # a valid call enqueued work on `keep`
        import torch
        torch.cuda.synchronize()
    return ""


@pytest.mark.parametrize("symbol", sorted(FAMILIES))
def test_null_pointer_names_the_argument(native, case, symbol):
    names, _, optional = FAMILIES[symbol]
    for k in names:
        msg = raw_call(native, case, symbol, null=(k,))
        if k in optional:
            assert msg == "", (symbol, k, msg)
        else:
            assert msg.endswith(f": {k} is null"), (symbol, k, msg)
    # the first NULL in the entry point's order is the one reported, after N's check
    assert raw_call(native, case, symbol, null=("bad", names[1], "f")).endswith(
        f": {names[1]} is null")
    assert "N must be in [1, " in raw_call(native, case, symbol, null=("x",), n=0)


@pytest.mark.parametrize("symbol", [s for s in sorted(FAMILIES) if not s.endswith("_dev")])
def test_row_spot_rate_messages_and_order(native, case, symbol):
    row = ROW.copy()
    row[3] = B
    spot, rate = case["spots"].copy(), case["rates"].copy()
    spot[1], rate[2] = np.nan, np.inf
    assert raw_call(native, case, symbol, row=row).endswith(": row 3 is outside [0, B)")
    assert raw_call(native, case, symbol, spot=spot).endswith(": spot 1 is not finite or not > 0")
    assert raw_call(native, case, symbol, rate=rate).endswith(": rate 2 is not finite")
    # pointers, then rows, then spot and rate market by market, then the objective's own checks
    assert raw_call(native, case, symbol, null=("g",), row=row).endswith(": g is null")
    assert raw_call(native, case, symbol, row=row, spot=spot).endswith(
        ": row 3 is outside [0, B)")
    rate0 = case["rates"].copy()
    rate0[0] = -np.inf
    assert raw_call(native, case, symbol, spot=spot, rate=rate0).endswith(
        ": rate 0 is not finite")
    assert raw_call(native, case, symbol, spot=spot, rate=rate).endswith(
        ": spot 1 is not finite or not > 0")
    if "iv" in symbol:
        assert raw_call(native, case, symbol, rate=rate, wgt=np.zeros((B, M))).endswith(
            ": rate 2 is not finite")
        assert "sum to zero" in raw_call(native, case, symbol, wgt=np.zeros((B, M)))
