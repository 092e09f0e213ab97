"""GPU checks of the full Greeks (csrc/dh_greeks_full.h): the three new summed planes
against the 50+-digit truth of tests/golden/greeks_full_truth.json, the six old planes against
dh_surface_greeks bit for bit, the bits' independence of the call, the dynamic-LDS cap on fresh
contexts, Dupire's quotient, dhcos.local_vol, and the refusals.

Unit and bar are tests/test_gpu_greeks_truth.py's: every bar is in the fixture's `unit` of the case
and plane (the plane's absolute term sum), and the device gets 16x the NumPy restatement's own
recorded error for that plane and N, never less than 16 * 2^-52.  Nothing here is set from the
device's output.  Measured on an MI355X (worst |device - truth| / unit over the cases of each N):

    N            1        2        17       128      256      772, 773, 2048
    dprice_dT    2.1e-16  5.1e-16  1.3e-15  2.1e-15  2.2e-15  1.2e-15
    rho          2.4e-16  2.0e-16  1.8e-16  1.4e-15  2.2e-15  2.5e-16
    dual_gamma   1.2e-16  2.0e-16  7.5e-16  1.2e-15  2.3e-15  7.3e-16

against bars of 3.6e-15 (the floor) to 1.1e-13: the device is inside every one by a factor of 4 or
more, and no bar was moved.  local_var equals the documented quotient of the device's own planes
with 0 ulp on every entry checked here (the bar is 4 ulp).
"""
import functools
import json
import os

import numpy as np
import pytest

import greeks_full_reference as GF

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
MARGIN = 16.0
NEW = [GF.PLANES.index(n) for n in GF.NEW_PLANES]          # 6, 7, 8
LV = GF.PLANES.index("local_var")


@pytest.fixture(scope="module")
def native():
    from dhcos import _native
    if _native.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    assert _native.GREEKS_FULL == GF.PLANES
    return _native


@functools.lru_cache(maxsize=None)
def fixture():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                           "greeks_full_truth.json")) as fh:
        return json.load(fh)


def device_bar(N):
    worst = fixture()["restatement_worst"]
    return np.array([max(MARGIN * worst[name][str(N)], MARGIN * EPS) for name in GF.NEW_PLANES])


def select(pred):
    """(cases, records [n, 16], K, T, is_call, truth [3, n], unit [3, n]) of the cases pred picks."""
    fix = fixture()
    cs = [c for c in fix["cases"] if pred(c)]
    rec = np.array([fix["sets"][c["set"]] + [c["S0"], c["r"], c["q"]] for c in cs])
    return (cs, rec, np.array([c["K"] for c in cs]), np.array([c["T"] for c in cs]),
            np.array([c["is_call"] for c in cs]), np.array([c["truth"] for c in cs]).T,
            np.array([c["unit"] for c in cs]).T)


def same_bits(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a).tobytes() == \
        np.ascontiguousarray(b).tobytes()


def assert_truth(got, truth, unit, N, label):
    """got [10, n]; truth, unit [3, n]: |got[NEW] - truth| <= device_bar(N) * unit."""
    bar = device_bar(N)
    err = np.abs(got[NEW] - truth)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(unit > 0, err / unit, np.where(err == 0, 0.0, np.inf))
    print(f"{label} N={N}: worst |device - truth| / unit  " + "  ".join(
        f"{name} {rel[g].max():.2e} (bar {bar[g]:.2e})" for g, name in enumerate(GF.NEW_PLANES)))
    ok = err <= bar[:, None] * unit
    assert ok.all(), (label, N, [(GF.NEW_PLANES[g], int(i), got[NEW][g, i], truth[g, i], unit[g, i])
                                 for g, i in np.argwhere(~ok)])


def assert_quotient(got, K, r, q, label):
    """local_var against the documented quotient of the device's own planes: NaN exactly where the
    host rule says, <= 4 ulp elsewhere (the issue's bar; 0 ulp is what the repeated order gives)."""
    ix = GF.PLANES.index
    want = GF.local_var_from_planes(got[ix("dprice_dT")], got[ix("price")], got[ix("dual_delta")],
                                    got[ix("dual_gamma")], K, r, q)
    lv = got[LV]
    assert np.array_equal(np.isnan(lv), np.isnan(want)), label
    m = ~np.isnan(want)
    ulps = np.abs(lv[m] - want[m]) / np.spacing(np.abs(want[m]))
    print(f"{label}: local_var against the host quotient, {m.sum()} finite of {m.size}, "
          f"worst {ulps.max() if m.any() else 0:.0f} ulp")
    assert (ulps <= 4).all(), (label, ulps.max())
    return m


_PAIRS = {}


def pairs_of(native, N):
    """The device's planes [10, n] of every fixture case of series length N: one call per N."""
    if N not in _PAIRS:
        _, rec, K, T, call, _, _ = select(lambda c: c["N"] == N)
        _PAIRS[N] = native.default_context().greeks_full_pairs(rec, K, T, call, N)
    return _PAIRS[N]


# ---- the LDS cap (first in the file, as in tests/test_gpu_greeks_truth.py) -----------------------
def test_lds_cap_is_raised_on_a_fresh_context_in_either_order(native):
    """greeks_full_lds_bytes is 49,136 B at N = 772 and 49,248 B at N = 773: the launch crosses the
    48 KiB default cap between them and the first request past it raises the kernel's cap, once per
    context.  772 then 773 on one fresh Context, 773 then 772 on another; all four against truth,
    and the same bits in either order."""
    sel = {N: select(lambda c, N=N: c["N"] == N) for N in (772, 773)}
    results = []
    for order in ((772, 773), (773, 772)):
        ctx = native.Context(native.default_context().device)
        try:
            results.append({N: ctx.greeks_full_pairs(*sel[N][1:5], N) for N in order})
        finally:
            ctx.close()
    for which, res in enumerate(results):
        for N in (772, 773):
            assert_truth(res[N], sel[N][5], sel[N][6], N, f"fresh context {which}")
    for N in (772, 773):
        assert same_bits(results[0][N], results[1][N]), N


# ---- device against truth ------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 17, 128, 256, 772, 773, 2048])
def test_pairs_match_truth_on_every_case_and_new_plane(native, N):
    cs, rec, K, _, _, truth, unit = select(lambda c: c["N"] == N)
    assert len(cs) == {128: 64, 256: 12}.get(N, 4)
    got = pairs_of(native, N)
    assert_truth(got, truth, unit, N, "pairs")
    assert_quotient(got, K, rec[:, 14], rec[:, 15], f"pairs N={N}")


# ---- the six old planes are dh_surface_greeks' ---------------------------------------------------
@pytest.mark.parametrize("N", [1, 17, 128, 256, 2048])
def test_first_six_planes_are_the_bits_of_greeks_pairs(native, N):
    """Groups A and B (N = 128), the clamp strikes (256) and N in {1, 17, 2048}, paired form."""
    _, rec, K, T, call, _, _ = select(lambda c: c["N"] == N)
    assert same_bits(pairs_of(native, N)[:6], native.default_context().greeks_pairs(
        rec, K, T, call, N))


@pytest.mark.parametrize("N", [17, 128, 256, 2048])
def test_surface_planes_are_the_bits_of_surface_greeks_and_of_pairs(native, N):
    """One surface of set 0's A and C options (three maturities, clamp-widened strikes among the
    T = 0.1 tile) under P = 3 records (the sets 0, 1, 2): its first six planes are
    dh_surface_greeks' bits, all ten are the paired form's, and a P = 1 request gives record 0's
    bits."""
    fix = fixture()
    cs, _, K, T, call, _, _ = select(lambda c: c["set"] == 0 and c["group"] in "AC")
    assert len(cs) == 24 and any(c["clamp"] for c in cs)
    rec = np.array([fix["sets"][s] + [100.0, 0.03, 0.0] for s in range(3)])
    ctx = native.default_context()
    surf = native.Surface(ctx, K, T, call)
    try:
        assert surf.n_tiles == 3
        full = surf.greeks_full(rec, N)
        assert full.shape == (10, 3, 24)
        assert same_bits(full[:6], surf.greeks(rec, N))
        assert same_bits(full[:, :1], surf.greeks_full(rec[:1], N))
    finally:
        surf.close()
    for p in range(3):
        pair = ctx.greeks_full_pairs(np.repeat(rec[p:p + 1], 24, axis=0), K, T, call, N)
        assert same_bits(full[:, p], pair), p
        assert_quotient(full[:, p], K, 0.03, 0.0, f"surface N={N} set {p}")


def test_a_maturity_of_300_options_in_two_tiles_has_the_bits_of_one_option_each(native):
    """300 strikes at T = 1 split into two tiles; every option's ten planes are the bits it has
    alone in a paired request, and a second maturity's tile does not move them."""
    fix = fixture()
    rec = np.array([fix["sets"][1] + [100.0, 0.03, 0.01]])
    K = np.concatenate([np.linspace(60.0, 160.0, 300), [90.0, 110.0]])
    T = np.concatenate([np.full(300, 1.0), [0.25, 0.25]])
    call = np.arange(302) % 2 == 0
    ctx = native.default_context()
    surf = native.Surface(ctx, K, T, call)
    try:
        assert surf.n_tiles == 3
        got = surf.greeks_full(rec, 64)[:, 0]
    finally:
        surf.close()
    assert same_bits(got, ctx.greeks_full_pairs(np.repeat(rec, 302, axis=0), K, T, call, 64))
    assert_quotient(got, K, 0.03, 0.01, "two tiles")


# ---- local_var -----------------------------------------------------------------------------------
BS_SET = [0.04, 2.0, 0.04, 1e-3, 0.0, 0.04, 1.5, 0.04, 1e-3, 0.0, 0.0, -0.05, 0.10]


def test_local_var_in_the_black_scholes_limit(native):
    """tests/test_greeks_full_truth.py's Black-Scholes-limit case on the device: sigma_j = 1e-3,
    rho_j = 0, lambda = 0, N = 512, T in {0.5, 1} x K / S0 in {0.9, 1, 1.1}, calls and puts, q =
    0.01: local_var = sum_j [theta_j + (v0_j - theta_j) e^{-kappa_j T}] to 1e-4 relative."""
    S0, r, q = 100.0, 0.03, 0.01
    grid = [(T, S0 * m, c) for T in (0.5, 1.0) for m in (0.9, 1.0, 1.1) for c in (True, False)]
    T, K, call = (np.array(x) for x in zip(*grid))
    rec = np.repeat(np.array([BS_SET + [S0, r, q]]), len(grid), axis=0)
    got = native.default_context().greeks_full_pairs(rec, K, T, call, 512)
    v01, k1, t1, _, _, v02, k2, t2 = BS_SET[:8]
    want = (t1 + (v01 - t1) * np.exp(-k1 * T)) + (t2 + (v02 - t2) * np.exp(-k2 * T))
    rel = np.abs(got[LV] / want - 1)
    print("Black-Scholes limit: local_var relative to the closed form, worst", rel.max())
    assert (np.abs(got[LV] - want) <= 1e-4 * want).all(), (got[LV], want)
    assert_quotient(got, K, r, q, "Black-Scholes limit")


def test_far_wing_strike_is_nan_or_finite_as_the_host_rule_says(native):
    """K = 3000 at T = 0.1 under the demo set (S0 = 100, clamp active, dual gamma at rounding
    level), call and put, N = 256: local_var is NaN exactly where the host quotient rule gives NaN
    and the quotient's bits elsewhere."""
    cs, rec, K, T, call, _, _ = select(lambda c: c["group"] == "C" and c["K"] == 3000.0)
    assert len(cs) == 2 and all(c["clamp"] for c in cs)
    got = native.default_context().greeks_full_pairs(rec, K, T, call, 256)
    print("far wing: dual_gamma", got[8], "local_var", got[LV])
    assert_quotient(got, K, rec[:, 14], rec[:, 15], "far wing")


# ---- the Python surface --------------------------------------------------------------------------
def test_local_vol_grid_is_greeks_full_of_each_option(native):
    import dhcos
    fix = fixture()
    prm = np.array([fix["sets"][0], fix["sets"][2]])
    strikes, mats = np.array([70.0, 85.0, 100.0, 115.0, 130.0]), np.array([0.25, 1.0, 2.0])
    lv = dhcos.local_vol(prm, 100.0, [0.03, 0.05], strikes, mats, N=256, q=[0.0, 0.01])
    assert np.array_equal(lv.strikes, strikes) and np.array_equal(lv.maturities, mats)
    for f in (lv.local_vol, lv.local_var, lv.density, lv.price, lv.valid):
        assert f.shape == (2, 3, 5)
    assert lv.valid.dtype == bool
    with np.errstate(invalid="ignore"):
        assert np.array_equal(lv.valid, np.isfinite(lv.local_var) & (lv.local_var >= 0))
    assert lv.valid.all()              # this grid is inside the range at every maturity
    assert np.array_equal(lv.local_vol, np.sqrt(lv.local_var))
    for p, (r, q) in enumerate(((0.03, 0.0), (0.05, 0.01))):
        for i, T in enumerate(mats):
            for j, K in enumerate(strikes):
                one = dhcos.greeks_full(prm[p], 100.0, r, [{"strike": K, "maturity": T,
                                                             "option_type": "call"}], N=256, q=q)
                assert same_bits(one.local_var, lv.local_var[p, i, j:j + 1]), (p, i, j)
                assert same_bits(one.price, lv.price[p, i, j:j + 1]), (p, i, j)
                assert same_bits(one.density, lv.density[p, i, j:j + 1]), (p, i, j)
    single = dhcos.local_vol(prm[0], 100.0, 0.03, strikes, mats, N=256)
    assert single.local_var.shape == (3, 5) and same_bits(single.local_var, lv.local_var[0])
    dh = dhcos.DoubleHeston(100.0, 115.0, 1.0, 0.03, *prm[0])
    g = dh.greeks_full(256)
    assert g.local_var.tobytes() == lv.local_var[0, 1, 3].tobytes()
    assert g.theta == -g.dprice_dT and g.epsilon == -(g.rho + 1.0 * g.price)
    b = dhcos.DoubleHeston.greeks_full_batch(prm[:1], 100.0, [115.0], [1.0], 0.03, N=256)
    assert same_bits(b.local_var, np.atleast_1d(g.local_var))


# ---- refusals ------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments(native):
    lib = native.load()
    ctx = native.default_context()
    rec = np.array([fixture()["sets"][0] + [100.0, 0.03, 0.0]])
    K, T, call = np.array([100.0]), np.array([1.0]), np.array([1], dtype=np.int8)
    out = np.zeros(10)
    surf = native.Surface(ctx, K, T, call)
    empty = native.Surface(ctx, np.empty(0), np.empty(0), np.empty(0, dtype=np.int8))
    a = lambda x: x.ctypes.data                                                    # noqa: E731
    try:
        def surface(h=ctx.handle, s=surf.handle, p=a(rec), P=1, N=128, L=10.0, o=a(out)):
            return lib.dh_surface_greeks_full(h, s, p, P, N, L, o)

        def surface_dev(h=ctx.handle, s=surf.handle, p=a(rec), P=1, N=128, L=10.0, o=a(out)):
            return lib.dh_surface_greeks_full_dev(h, s, p, P, N, L, o, None)

        def pairs(h=ctx.handle, p=a(rec), k=a(K), t=a(T), c=a(call), n=1, N=128, L=10.0, o=a(out)):
            return lib.dh_greeks_full_pairs(h, p, k, t, c, n, N, L, o)

        bad = [dict(N=0), dict(N=2049), dict(L=0.0), dict(L=-1.0), dict(L=float("nan")),
               dict(h=None), dict(p=None), dict(o=None)]
        for f, extra in ((surface, [dict(P=0), dict(s=None)]),
                         (surface_dev, [dict(P=0), dict(s=None)]),
                         (pairs, [dict(n=0), dict(k=None), dict(t=None), dict(c=None)])):
            for kw in bad + extra:
                assert f(**kw) == -1, (f.__name__, kw)             # DH_E_ARG
                assert len(lib.dh_last_error()) > 0
        assert surface(s=empty.handle) == 0 and surface_dev(s=empty.handle) == 0   # M = 0: DH_OK
        assert surface() == 0 and np.isfinite(out).all()
    finally:
        surf.close()
        empty.close()
