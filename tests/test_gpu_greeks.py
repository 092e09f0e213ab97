"""GPU checks of the analytic COS Greeks (dh_surface_greeks*, dh_greeks_pairs, dhcos.greeks): the
device against the NumPy restatement (tests/greeks_reference.py) per plane, against Surface.price,
Euler's identity, bit-reproducibility across the call forms, NaN parameters and the refusals.

Parity bar per plane: conftest.rel_close(rtol=1e-6) with the absolute floor 1e-10 in the plane's
natural unit (price and vegas 1e-10 S0, delta and dual delta 1e-10, gamma 1e-10 / S0)."""
import ctypes as C
import functools

import numpy as np
import pytest

import greeks_reference as G
from conftest import rel_close

pytestmark = pytest.mark.gpu

S0, R = 100.0, 0.03
LO = np.array([0.025, 1.5, 0.025, 0.2, -0.85, 0.02, 0.3, 0.025, 0.1, -0.7, 0.05, -0.08, 0.03])
HI = np.array([0.08, 4.5, 0.065, 0.5, -0.4, 0.07, 1.2, 0.07, 0.35, -0.2, 0.25, -0.01, 0.12])
NS = [1, 2, 64, 65, 128, 2048]


@pytest.fixture(scope="module")
def native():
    from dhcos import _native
    if _native.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return _native


def records(seed, P, spot=S0, q=0.0):
    rs = np.random.RandomState(seed)
    rec = np.empty((P, 16))
    rec[:, :13] = LO + (HI - LO) * rs.rand(P, 13)
    rec[:, 13], rec[:, 14], rec[:, 15] = spot, R, q
    return rec


def floors(spot):
    """[6, 1, 1] absolute floors in PLANES' order: price, delta, gamma, dual delta, vega1, vega2."""
    s = np.atleast_1d(np.asarray(spot, dtype=np.float64))            # [1], or [P]: a spot per set
    one = np.ones_like(s)
    return np.stack([1e-10 * s, 1e-10 * one, 1e-10 / s, 1e-10 * one, 1e-10 * s,
                     1e-10 * s])[:, :, None]


def assert_planes(got, want, spot, label):
    ok = rel_close(got, want, 1e-6, floors(spot))
    for g, name in enumerate(G.PLANES):
        err = np.abs(got[g] - want[g])
        print(f"{label} {name}: max abs {err.max():.3e} max rel "
              f"{np.max(err / np.maximum(np.abs(want[g]), 1e-300)):.3e}")
    assert ok.all(), (label, [G.PLANES[g] for g in np.unique(np.argwhere(~ok)[:, 0])])


def same_bits(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a).tobytes() == \
        np.ascontiguousarray(b).tobytes()


# ---- the cases, and their references (computed once) -------------------------------------------
def mixed_case():
    """Five maturities of 7 options, calls and puts mixed, in the caller's (unsorted) order."""
    rs = np.random.RandomState(5)
    T = np.repeat([0.1, 0.35, 0.8, 1.25, 2.0], 7)
    K = S0 * rs.uniform(0.85, 1.15, 35)
    call = rs.rand(35) < 0.5
    order = rs.permutation(35)
    return records(11, 3), K[order], T[order], call[order]


def tile_case():
    """One maturity, 257 options: tiles of 256 and 1; its prefixes give M = 1, 255, 256."""
    rs = np.random.RandomState(6)
    return records(12, 1), S0 * rs.uniform(0.8, 1.2, 257), np.full(257, 0.7), rs.rand(257) < 0.5


def clamp_case():
    """The six clamp-active strikes of test_fast_path_matches_exact_mode_full_size (T = 0.1) in
    one tile with 14 unclamped neighbours."""
    rs = np.random.RandomState(7)
    K = np.concatenate([[5.0, 40.0, 60.0, 250.0, 500.0, 3000.0], S0 * rs.uniform(0.9, 1.1, 14)])
    call = rs.rand(20) < 0.5
    order = rs.permutation(20)
    return records(13, 3), K[order], np.full(20, 0.1), call[order]


@functools.lru_cache(maxsize=None)
def reference(name, N):
    rec, K, T, call = {"mixed": mixed_case, "tile": tile_case, "clamp": clamp_case}[name]()
    return G.greeks_surface(rec, K, T, call, N)


# ---- device against the restatement ---------------------------------------------------------------
@pytest.mark.parametrize("N", NS)
def test_mixed_surface_matches_restatement(native, N):
    """N in {1, 2, 64, 65, 128, 2048} x P in {1, 3}: five maturities of 7 options; a set priced alone
    gives the bits it has inside P = 3, and two calls give the same bits."""
    rec, K, T, call = mixed_case()
    want = reference("mixed", N)
    ctx = native.default_context()
    surf = native.Surface(ctx, K, T, call)
    try:
        got = surf.greeks(rec, N)
        again = surf.greeks(rec, N)
        alone = surf.greeks(rec[:1], N)
    finally:
        surf.close()
    assert got.shape == (6, 3, 35) and alone.shape == (6, 1, 35)
    assert_planes(got, want, S0, f"mixed N={N} P=3")
    assert_planes(alone, want[:, :1], S0, f"mixed N={N} P=1")
    assert same_bits(got, again)
    assert same_bits(alone, got[:, :1])


@pytest.mark.parametrize("M", [1, 255, 256, 257])
def test_tile_edges(native, M):
    rec, K, T, call = tile_case()
    want = reference("tile", 128)[:, :, :M]
    surf = native.Surface(native.default_context(), K[:M], T[:M], call[:M])
    try:
        got = surf.greeks(rec, 128)
        assert surf.n_tiles == (2 if M > 256 else 1)
    finally:
        surf.close()
    assert_planes(got, want, S0, f"tile M={M}")


def test_clamped_options_among_unclamped_neighbours(native):
    """The six strikes of test_fast_path_matches_exact_mode_full_size at T = 0.1 among 14 neighbours
    near the money.  Which of the six the clamp widens depends on the set's cumulant range (its
    half-width at T = 0.1 is 0.7 to 1.0 for parameters in the generator's bounds): K = 5, 500 and
    3000 under every set, K = 40 and 250 under the two sets with the narrower range, K = 60
    (log(0.6) - 0.1 = -0.61) under none.  The pattern is asserted, so that both branches are known
    to run: 13 (set, option) pairs the per-term way, 47 on the tile's table, in one tile."""
    rec, K, T, call = clamp_case()
    active = np.array([[G.clamp_active(r[:13], S0, k, 0.1, R) for k in K] for r in rec])
    strikes = [sorted(K[a].tolist()) for a in active]
    print("clamp-active strikes per set:", strikes)
    assert strikes == [[5.0, 500.0, 3000.0], [5.0, 40.0, 250.0, 500.0, 3000.0],
                       [5.0, 40.0, 250.0, 500.0, 3000.0]]
    want = reference("clamp", 256)
    ctx = native.default_context()
    surf = native.Surface(ctx, K, T, call)
    try:
        got = surf.greeks(rec, 256)
        prices = surf.price(rec, 256)
    finally:
        surf.close()
    assert_planes(got, want, S0, "clamp N=256")
    assert rel_close(got[0], prices, 1e-11, 1e-11).all(), np.max(np.abs(got[0] - prices))


def test_pct_spot_surface_and_dividend_yield(native):
    """A DH_STRIKE_PCT_SPOT surface under three spots, and q = 0.02."""
    rec = records(14, 3, spot=np.array([80.0, 100.0, 125.0]), q=0.02)
    rs = np.random.RandomState(8)
    K_rel = rs.uniform(85.0, 115.0, 12)
    T = np.repeat([0.25, 1.0, 1.75], 4)
    call = rs.rand(12) < 0.5
    want = G.greeks_surface(rec, K_rel, T, call, 128, pct_spot=True)
    ctx = native.default_context()
    surf = native.Surface(ctx, K_rel, T, call, strike_mode=native.STRIKE_PCT_SPOT)
    try:
        got = surf.greeks(rec, 128)
        prices = surf.price(rec, 128)
    finally:
        surf.close()
    assert_planes(got, want, rec[:, 13], "pct-spot q=0.02")
    assert rel_close(got[0], prices, 1e-11, 1e-11).all()
    # the absolute-strike surface of each set gives the same bits: the strike is resolved, then held
    for p in range(3):
        s2 = native.Surface(ctx, K_rel * rec[p, 13] / 100.0, T, call)
        try:
            assert same_bits(s2.greeks(rec[p:p + 1], 128), got[:, p:p + 1]), p
        finally:
            s2.close()


# ---- further checks -----------------------------------------------------------------------------
@pytest.mark.parametrize("N", [128, 2048])
def test_price_plane_matches_surface_price(native, N):
    rec, K, T, call = mixed_case()
    surf = native.Surface(native.default_context(), K, T, call)
    try:
        got = surf.greeks(rec, N)[0]
        prices = surf.price(rec, N)
    finally:
        surf.close()
    print(f"N={N}: max |greeks price - Surface.price| {np.max(np.abs(got - prices)):.3e}")
    assert rel_close(got, prices, 1e-11, 1e-11).all()


def _euler_residual(native, case, N):
    rec, K, T, call = {"mixed": mixed_case, "clamp": clamp_case}[case]()
    surf = native.Surface(native.default_context(), K, T, call)
    try:
        g = surf.greeks(rec, N)
    finally:
        surf.close()
    sd, kd = S0 * g[1], K[None, :] * g[3]
    return g[0], sd, kd, np.abs(sd + kd - g[0])


@pytest.mark.parametrize("N", [128, 2048])
def test_euler_identity_on_the_device_planes(native, N):
    """price = S0 delta + K dual_delta on the device's own planes to 1e-12 relative to the price, on
    the mixed surface (prices from a few cents up).  Measured on an MI355X: 2.5e-14."""
    price, _, _, resid = _euler_residual(native, "mixed", N)
    print(f"mixed N={N}: euler max residual {resid.max():.3e}, max rel to the price "
          f"{np.max(resid / np.abs(price)):.3e}")
    assert np.all(resid <= 1e-12 * np.abs(price))


def test_euler_identity_among_clamped_strikes(native):
    """The same identity on the clamp surface, a case the issue does not list.  Its clamped options
    have prices down to 1e-13 (K = 3000), of the size of the rounding of the three N-term sums whose
    terms are of the size of S0 however far out of the money the option is; a bar relative to such
    a price means nothing.  So here the residual is held to 1e-12 of max(|price|, |S0 delta|,
    |K dual_delta|, S0): the identity's addends, and where all are smaller than the spot, S0, the
    price plane's natural unit.  Measured on an MI355X: residuals <= 1.8e-13, 6.7e-16 of that unit."""
    price, sd, kd, resid = _euler_residual(native, "clamp", 256)
    scale = np.maximum(np.maximum(np.abs(price), S0), np.maximum(np.abs(sd), np.abs(kd)))
    print(f"clamp N=256: euler max residual {resid.max():.3e}, max rel to max(addends, S0) "
          f"{np.max(resid / scale):.3e}")
    assert np.all(resid <= 1e-12 * scale)


def test_call_forms_give_the_same_bits(native):
    """dh_surface_greeks against _dev on a caller's stream, against greeks_pairs on the same
    (set, option) pairs, and against DoubleHeston.greeks / greeks_batch / dhcos.greeks."""
    import torch
    import dhcos
    rec, K, T, call = clamp_case()                     # clamped and unclamped options
    P, M, N = 3, K.size, 256
    ctx = native.default_context()
    surf = native.Surface(ctx, K, T, call)
    try:
        host = surf.greeks(rec, N)
        dev = torch.device("cuda", ctx.device)
        d_rec = torch.from_numpy(rec).to(dev)
        d_out = torch.full((6, P, M), -1.0, dtype=torch.float64, device=dev)
        stream = torch.cuda.Stream(device=dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        assert stream.cuda_stream != 0
        with torch.cuda.stream(stream):
            surf.greeks_dev(d_rec.data_ptr(), P, d_out.data_ptr(), N=N, stream=stream.cuda_stream)
        stream.synchronize()
        assert same_bits(d_out.cpu().numpy(), host)
    finally:
        surf.close()
    pairs = ctx.greeks_pairs(np.repeat(rec, M, axis=0), np.tile(K, P), np.tile(T, P),
                             np.tile(call, P), N)
    assert same_bits(pairs.reshape(6, P, M), host)
    batch = dhcos.DoubleHeston.greeks_batch(np.repeat(rec[:, :13], M, axis=0), S0, np.tile(K, P),
                                            np.tile(T, P), R, np.tile(call, P), N=N)
    opts = [{"strike": k, "maturity": t, "option_type": "call" if c else "put"}
            for k, t, c in zip(K, T, call)]
    top = dhcos.greeks(rec[:, :13], S0, R, opts, N=N)
    one = dhcos.greeks(dict(zip(dhcos.calibrator.PARAM_NAMES, rec[1, :13])), S0, R, opts, N=N)
    m = 3
    kw = dict(zip(dhcos.pricer.MODEL_FIELDS, rec[2, :13]))
    single = dhcos.DoubleHeston(S0=S0, K=K[m], T=T[m], r=R, option_type=opts[m]["option_type"],
                                **kw).greeks(N)
    for g, name in enumerate(G.PLANES):
        assert same_bits(getattr(batch, name).reshape(P, M), host[g]), name
        assert same_bits(getattr(top, name), host[g]), name
        assert same_bits(getattr(one, name), host[g, 1]), name
        assert np.float64(getattr(single, name)).tobytes() == host[g, 2, m].tobytes(), name


def test_nan_parameters_give_nan_planes_and_leave_the_context_usable(native):
    rec, K, T, call = mixed_case()
    bad = rec.copy()
    bad[1, 3] = np.nan                                 # sigma1 of the middle set
    surf = native.Surface(native.default_context(), K, T, call)
    try:
        got = surf.greeks(bad, 128)
        after = surf.greeks(rec, 128)
    finally:
        surf.close()
    assert np.isnan(got[:, 1]).all()
    assert same_bits(got[:, [0, 2]], after[:, [0, 2]])
    assert np.isfinite(after).all()


def test_refusals_name_the_argument(native):
    lib = native.load()
    rec, K, T, call = mixed_case()
    ctx = native.default_context()
    surf = native.Surface(ctx, K, T, call)
    out = np.empty((6, 3, 35))
    ic = np.ascontiguousarray(call, dtype=np.int8)

    def surface(ctx_h=ctx.handle, s=surf.handle, prm=rec.ctypes.data, P=3, N=128, L=10.0,
                o=out.ctypes.data):
        return lib.dh_surface_greeks(ctx_h, s, prm, P, N, L, o)

    def surface_dev(**kw):
        a = dict(ctx_h=ctx.handle, s=surf.handle, prm=rec.ctypes.data, P=3, N=128, L=10.0,
                 o=out.ctypes.data)
        a.update(kw)
        return lib.dh_surface_greeks_dev(a["ctx_h"], a["s"], a["prm"], a["P"], a["N"], a["L"],
                                         a["o"], None)

    def pairs(ctx_h=ctx.handle, prm=rec.ctypes.data, k=K.ctypes.data, t=T.ctypes.data,
              c=ic.ctypes.data, n=3, N=128, L=10.0, o=out.ctypes.data):
        return lib.dh_greeks_pairs(ctx_h, prm, k, t, c, n, N, L, o)

    try:
        for call_, kw, word in [
                (surface, dict(N=0), b"N"), (surface, dict(N=native.MAX_N + 1), b"N"),
                (surface, dict(P=0), b"P"), (surface, dict(L=0.0), b"L"),
                (surface, dict(L=float("inf")), b"L"), (surface, dict(L=float("nan")), b"L"),
                (surface, dict(ctx_h=None), b"ctx"), (surface, dict(s=None), b"surface"),
                (surface, dict(prm=None), b"params"), (surface, dict(o=None), b"out"),
                (surface_dev, dict(N=4096), b"N"), (surface_dev, dict(P=-1), b"P"),
                (surface_dev, dict(L=-1.0), b"L"), (surface_dev, dict(prm=None), b"params"),
                (surface_dev, dict(o=None), b"out"),
                (pairs, dict(N=0), b"N"), (pairs, dict(n=0), b"n"), (pairs, dict(L=0.0), b"L"),
                (pairs, dict(k=None), b"K"), (pairs, dict(t=None), b"T"),
                (pairs, dict(c=None), b"is_call"), (pairs, dict(prm=None), b"params"),
                (pairs, dict(o=None), b"out")]:
            assert call_(**kw) == -1, (call_.__name__, kw)               # DH_E_ARG
            assert lib.dh_last_error().startswith(word + b" "), (kw, lib.dh_last_error())
        assert surface() == 0 and np.isfinite(out).all()                 # and still usable
    finally:
        surf.close()
