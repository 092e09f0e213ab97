"""GPU checks of the analytic parameter sensitivities (param_grad_kernel, csrc/dh_param_grad.h;
DESIGN.md 3.18) and of the two reductions on its planes (loss_grad_rows, gauss_newton_rows; 3.19,
3.21) against the 50-digit truth of tests/golden/param_sens_truth.json: every case and plane through
dh_param_sens_pairs, N = 1, the clamp group through a surface tile that mixes the table pass with
the per-term way, every series length of group D through a surface, the dynamic-LDS cap on fresh
contexts in both orders, per-record market data in both strike modes, and the loss gradient and
Gauss-Newton Hessian against values composed from the truth planes alone.

Unit.  Every bar is in the fixture's `unit` of the case and plane: the series' absolute term sum
e^{-rT} sum_k |term_k| (tests/golden/make_param_sens_truth.py), so a value at rounding level is held
to the rounding of the sum that made it.

Bar (device_bar).  The reference is the NumPy restatement's own fp64 error against the truth,
restatement_worst[plane][key] of the fixture (key: the group for A, B, C, E; N for D), measured by
the generator.  The device gets MARGIN = 16 times that: its primitives are held to 2 ulp where libm
gives <= 1, and cdiv_rcp to 6 ulp where IEEE division gives 0.5 -- at most 12 times as much,
rounded up to the next power of two (tests/test_gpu_greeks_truth.py uses the same
factor) -- and never less than 16 * 2^-52 of the unit.  The bars are per plane because the
restatement's error is: the kappa/sigma/rho chain cancels inside each term, and kappa2's bar comes
out three orders above the price's.  Nothing here is set from the device's output.  Measured on an
MI355X (worst |device - truth| / unit over the cases of each key, dh_param_sens_pairs):

    key         A        B        C        E        2        17       65       336, 337, 1024
    price       8.4e-16  1.5e-15  4.3e-15  6.9e-16  5.7e-16  2.7e-16  3.4e-16  3.2e-16
    v1_0        3.7e-15  1.4e-14  5.5e-15  1.4e-15  8.6e-16  9.2e-16  9.9e-16  1.0e-15
    kappa1      8.2e-13  1.3e-13  4.5e-12  1.8e-12  3.5e-13  4.4e-14  4.1e-14  4.1e-14
    theta1      6.8e-14  2.5e-14  3.4e-13  5.9e-15  4.8e-15  4.1e-15  4.0e-15  4.0e-15
    sigma1      3.4e-13  8.8e-13  1.2e-12  1.5e-13  3.8e-14  3.7e-14  3.3e-14  3.3e-14
    rho1        6.2e-14  1.1e-14  3.1e-14  6.6e-15  1.3e-13  8.0e-15  7.3e-15  7.2e-15
    v2_0        2.5e-15  1.4e-15  3.2e-15  1.4e-15  1.4e-15  1.6e-15  1.8e-15  1.6e-15
    kappa2      6.5e-12  1.7e-13  1.9e-11  1.8e-12  1.5e-12  6.8e-13  5.9e-13  5.9e-13
    theta2      1.1e-13  3.0e-14  2.2e-13  5.9e-15  5.4e-15  5.6e-15  5.4e-15  5.4e-15
    sigma2      2.8e-13  8.1e-14  1.2e-12  1.5e-13  5.7e-13  1.3e-13  1.2e-13  1.2e-13
    rho2        5.3e-14  1.5e-14  4.0e-14  6.6e-15  2.1e-13  6.4e-15  5.7e-15  5.7e-15
    lambda_j    1.6e-14  4.0e-15  4.7e-15  1.4e-15  5.3e-14  9.3e-15  9.0e-15  9.0e-15
    mu_j        3.4e-15  2.6e-15  1.5e-15  1.3e-15  3.8e-15  5.4e-16  5.5e-16  5.6e-16
    sigma_j     1.6e-15  1.1e-15  3.9e-15  1.2e-15  1.2e-15  8.7e-16  8.3e-16  9.0e-16

(N = 1: price 3.8e-16, every parameter plane exactly 0.)  The bars run from 3.6e-15 (the floor) to
1.3e-10 (kappa2 on the grid); the device's worst share of its bar is 0.46 (sigma1, group B), then
0.27 (sigma2, N = 65) and 0.26 (theta1, group C); the price plane uses at most 0.11 of its bar.  No
bar was moved.  The run that first measured this found one defect: at N = 1 the kernel's D_p(0) was
a rounding residue (up to 1.3e-12 of unit_price plane_ratio on sigma2, against the 3.6e-15 of test
b), not 0; term 0's parameter weights are now exactly 0 in csrc/dh_param_grad.h.

The reductions (group E) are held to bars propagated from the plane bars: see
test_loss_gradient_and_gauss_newton_hessian_against_truth.  Measured: f, g and H within 0.4 % to
3.6 % of those bars.  The bars themselves are wide on this group: its calls at T = 1 and 2 have a
price unit of 1.3e8 and 8.7e10 beside prices of 60 to 80 (the call payoff's e^b on a range of +-25),
so the propagated bar of g is 7e-5 to 2e-2 of its absolute sum; the device's g is within 4e-5
relative of the truth on every component.
"""
import functools
import json
import math
import os

import numpy as np
import pytest

import greeks_reference as G
import param_grad_reference as R

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
MARGIN = 16.0
NS_D = (1, 2, 17, 65, 336, 337, 1024)


@pytest.fixture(scope="module")
def native():
    from dhcos import _native
    if _native.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return _native


@functools.lru_cache(maxsize=None)
def fixture():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                           "param_sens_truth.json")) as fh:
        return json.load(fh)


def key_of(c):
    return str(c["N"]) if c["group"] == "D" else c["group"]


def device_bar(plane, key):
    """The bar of a plane (its name) under a key, in units of the case's `unit`; nan where the
    fixture has no entry: the parameter planes at N = 1, whose unit is 0 (test b holds them)."""
    worst = fixture()["restatement_worst"][plane]
    return max(MARGIN * worst[key], MARGIN * EPS) if key in worst else math.nan


class Cases:
    """The fixture's cases pred picks, in the fixture's order: idx, cases, records [n, 16], K, T,
    call, truth [14, n], unit [14, n], bar [14, n] and keys [n]."""

    def __init__(self, pred):
        fix = fixture()
        self.idx = [i for i, c in enumerate(fix["cases"]) if pred(c)]
        self.cases = cs = [fix["cases"][i] for i in self.idx]
        self.rec = np.array([fix["sets"][c["set"]] + [c["S0"], c["r"], c["q"]] for c in cs])
        self.K = np.array([c["K"] for c in cs])
        self.T = np.array([c["T"] for c in cs])
        self.call = np.array([c["is_call"] for c in cs])
        self.truth = np.array([c["truth"] for c in cs]).T
        self.unit = np.array([c["unit"] for c in cs]).T
        self.keys = np.array([key_of(c) for c in cs])
        self.bar = np.array([[device_bar(name, k) for k in self.keys] for name in R.PLANES])

    def __len__(self):
        return len(self.idx)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_truth(got, sel, label, cols=None):
    """got [14, n] against sel's truth (cols: the columns of sel that got holds):
    |got - truth| <= bar * unit wherever the plane has a bar, the worst per plane and key printed
    first."""
    cols = np.arange(len(sel)) if cols is None else np.asarray(cols)
    truth, unit, bar, keys = sel.truth[:, cols], sel.unit[:, cols], sel.bar[:, cols], sel.keys[cols]
    assert got.shape == truth.shape, (label, got.shape, truth.shape)
    err = np.abs(got - truth)
    held = ~np.isnan(bar)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(held, err / unit, 0.0)
    for key in dict.fromkeys(keys):
        m = keys == key
        print(f"{label} key {key}: worst |device - truth| / unit (bar)  " + "  ".join(
            f"{name} {rel[g, m].max():.1e} ({bar[g, m][0]:.1e})" for g, name in enumerate(R.PLANES)))
    with np.errstate(invalid="ignore"):
        ok = ~held | (err <= bar * unit)
    assert ok.all(), (label, [(R.PLANES[g], int(i), keys[i], got[g, i], truth[g, i], unit[g, i])
                              for g, i in np.argwhere(~ok)])


_PAIRS = {}


def pairs_of(native, N):
    """(the device's planes [14, n], the cases) of every fixture case of series length N, in the
    fixture's order: one Context.param_sens_pairs call per N, shared among the tests."""
    if N not in _PAIRS:
        sel = Cases(lambda c: c["N"] == N)
        _PAIRS[N] = (native.default_context().param_sens_pairs(sel.rec, sel.K, sel.T, sel.call, N),
                     sel)
    return _PAIRS[N]


# ---- e. the LDS cap (first in the file: see the docstring) ---------------------------------------
def test_lds_cap_is_raised_on_a_fresh_context_in_either_order(native):
    """lds_bytes(N) = 5,904 + 128 Np is 48,912 B at N = 336 and 49,168 B at N = 337 (Np = 338): the
    launch crosses the 48 KiB default cap of dynamic LDS between them, and the first request past it
    raises the kernel's cap, once per context.  On a fresh Context the first request is N = 337,
    then 336, then 128; on a second fresh Context the order is reversed.  Each result is held to the
    truth, and N = 128 and N = 336 give the same bits on both.  The kernel's attribute belongs to
    the process, so the raise itself is new only in the first such request of a process; this test
    stands first in its file so that it makes that request when the file runs alone or first.  The
    N = 336 and 337 requests are group D's eight pairs, the N = 128 request is the 124 pairs of
    groups A, B and E."""
    sel = {N: Cases(lambda c, N=N: c["N"] == N) for N in (128, 336, 337)}
    assert [len(sel[N]) for N in (128, 336, 337)] == [124, 8, 8]
    results = []
    for order in ((337, 336, 128), (128, 336, 337)):
        ctx = native.Context(native.default_context().device)
        try:
            results.append({N: ctx.param_sens_pairs(sel[N].rec, sel[N].K, sel[N].T, sel[N].call, N)
                            for N in order})
        finally:
            ctx.close()
    for which, res in enumerate(results):
        for N in (128, 336, 337):
            assert_truth(res[N], sel[N], f"fresh context {which} N={N}")
    for N in (128, 336):
        assert same_bits(results[0][N], results[1][N]), N


# ---- a. every case through the pairs form ---------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 17, 65, 128, 256, 336, 337, 1024])
def test_pairs_match_truth_on_every_case_and_plane(native, N):
    """Groups A, B and E at N = 128 (124 pairs, per-pair market data among them), C at 256 (36,
    clamped and not), D at each of its seven lengths (8 each)."""
    got, sel = pairs_of(native, N)
    assert len(sel) == {128: 124, 256: 36}.get(N, 8)
    assert got.shape == (14, len(sel))
    assert_truth(got, sel, f"pairs N={N}")


# ---- b. N = 1 ---------------------------------------------------------------------------------------
def test_a_series_of_one_term_has_no_parameter_sensitivity(native):
    """At N = 1 the series is term 0 alone, where u = 0 and every D_p(0) is exactly 0: the truth of
    the thirteen parameter planes is 0 and so is their unit.  The device's are finite (no 0 / 0 in
    the chain at u = 0: d = kappa, bm = 0, D = 2 kappa) and no larger than 16 * 2^-52 of the price's
    unit times plane_ratio[i], the plane's natural size beside the price (the fixture's median of
    unit_i / unit_price over group D's N = 2 cases): the rounding residue of D_p(0).  The price plane
    is held to its bar."""
    got, sel = pairs_of(native, 1)
    ratio = np.array(fixture()["plane_ratio"])
    assert len(sel) == 8 and not sel.truth[1:].any() and not sel.unit[1:].any()
    assert np.all(ratio[1:] > 0) and ratio[0] == 1.0
    err0 = np.abs(got[0] - sel.truth[0])
    assert np.all(err0 <= device_bar("price", "1") * sel.unit[0]), (got[0], sel.truth[0])
    assert np.isfinite(got).all(), got
    bound = MARGIN * EPS * sel.unit[0][None, :] * ratio[1:, None]
    print("N=1: worst |plane| / (unit_price plane_ratio):  " + "  ".join(
        f"{name} {np.max(np.abs(got[1 + i]) / (sel.unit[0] * ratio[1 + i])):.1e}"
        for i, name in enumerate(R.PLANES[1:])))
    assert np.all(np.abs(got[1:]) <= bound), [R.PLANES[1 + i] for i in
                                              np.unique(np.argwhere(np.abs(got[1:]) > bound)[:, 0])]


# ---- c. the clamp group in a mixed tile -------------------------------------------------------------
@pytest.mark.parametrize("s", [0, 1, 2])
def test_clamp_group_in_a_tile_with_near_the_money_neighbours(native, s):
    """Group C's twelve options of one set (T = 0.1, N = 256) on one surface among the 14
    near-the-money neighbours of tests/test_gpu_param_grad.py's clamp_case: one tile, of which the
    table pass takes the options on the tile's range and the per-term way the clamp-widened ones
    (flags asserted mixed, the neighbours all unclamped).  The twelve are held to truth, and have the
    bits of the pairs call: a set's values do not depend on P, tile or stream, and a clamped option
    takes the per-term path on the same range either way."""
    import test_gpu_param_grad as PG
    _, K20, _, call20 = PG.clamp_case()
    near = ~np.isin(K20, [5.0, 40.0, 60.0, 250.0, 500.0, 3000.0])
    assert near.sum() == 14
    pairs, sel256 = pairs_of(native, 256)
    cols = [j for j, c in enumerate(sel256.cases) if c["set"] == s]
    flags = [sel256.cases[j]["clamp"] for j in cols]
    assert len(cols) == 12 and any(flags) and not all(flags)
    prm = fixture()["sets"][s]
    assert not any(G.clamp_active(prm, 100.0, k, 0.1, 0.03) for k in K20[near])
    K = np.concatenate([sel256.K[cols], K20[near]])
    call = np.concatenate([sel256.call[cols], call20[near]])
    rec = np.array([prm + [100.0, 0.03, 0.0]])
    surf = native.Surface(native.default_context(), K, np.full(26, 0.1), call)
    try:
        assert surf.n_tiles == 1
        got = surf.param_sens(rec, 256)
    finally:
        surf.close()
    assert got.shape == (14, 1, 26) and np.isfinite(got).all()
    assert_truth(got[:, 0, :12], sel256, f"surface tile set {s}", cols)
    differ = [(sel256.cases[j]["K"], sel256.cases[j]["is_call"], sel256.cases[j]["clamp"])
              for n, j in enumerate(cols) if not same_bits(got[:, 0, n], pairs[:, j])]
    assert not differ, differ


# ---- d. every series length through a surface ------------------------------------------------------
def test_series_lengths_through_a_surface(native):
    """Group D's four options (T = 0.7) on one surface under its two sets, at every N of the group:
    M = 4, one block per set.  At N = 17 and 65 the last round of the 16-lane pass has one live lane
    (k = 16, 64); at N = 337 the LDS stride is Np = 338 and the padding slot stays unread; N = 1024
    is the longest series the request takes, and 1025 is refused with DH_E_ARG naming N."""
    fix = fixture()
    four = Cases(lambda c: c["group"] == "D" and c["N"] == 2 and c["set"] == 0)
    assert len(four) == 4
    rec = np.array([fix["sets"][s] + [100.0, 0.03, 0.0] for s in (0, 6)])
    surf = native.Surface(native.default_context(), four.K, four.T, four.call)
    try:
        got = {N: surf.param_sens(rec, N) for N in NS_D}
        with pytest.raises(native.NativeError, match=r"error -1: N must be in \[1, 1024\]"):
            surf.param_sens(rec, 1025)
        again = surf.param_sens(rec, 337)                      # and still usable
    finally:
        surf.close()
    assert same_bits(again, got[337])
    for N in NS_D:
        sel = Cases(lambda c, N=N: c["group"] == "D" and c["N"] == N)
        # the fixture's order within an N: set 0's four options, then set 6's, each in four's order
        assert [c["set"] for c in sel.cases] == [0] * 4 + [6] * 4
        assert np.array_equal(sel.K, np.tile(four.K, 2)) and \
            np.array_equal(sel.call, np.tile(four.call, 2))
        assert got[N].shape == (14, 2, 4)
        flat = got[N].reshape(14, 8)
        assert np.isfinite(flat).all()
        assert_truth(flat, sel, f"surface N={N}")
        if N == 1:
            ratio = np.array(fix["plane_ratio"])
            assert np.all(np.abs(flat[1:]) <= MARGIN * EPS * sel.unit[0][None, :] * ratio[1:, None])


# ---- f. market data per record, both strike modes --------------------------------------------------
@pytest.mark.parametrize("s", [1, 2])
def test_market_data_of_the_record_in_both_strike_modes(native, s):
    """Group B: S0 != 100, and under set 1 q != 0 (record column 15), through Surface.param_sens
    with absolute strikes; then the same options as percentages of spot, K 100 / S0, which the
    kernel turns back by K_pct S0 / 100: held to truth, and where that round trip returns K's bits
    the planes have the bits of the absolute form."""
    sel = Cases(lambda c: c["group"] == "B" and c["set"] == s)
    assert len(sel) == 8 and len({tuple(r) for r in sel.rec}) == 1
    if s == 1:
        assert sel.rec[0, 15] == 0.02
    S0 = sel.rec[0, 13]
    pct = sel.K * 100.0 / S0
    exact = pct * S0 / 100.0 == sel.K
    print(f"set {s}: K 100 / S0 round trip exact for {int(exact.sum())} of 8 options")
    ctx = native.default_context()
    absolute = native.Surface(ctx, sel.K, sel.T, sel.call, strike_mode=native.STRIKE_ABSOLUTE)
    percent = native.Surface(ctx, pct, sel.T, sel.call, strike_mode=native.STRIKE_PCT_SPOT)
    try:
        got_abs = absolute.param_sens(sel.rec[:1], 128)
        got_pct = percent.param_sens(sel.rec[:1], 128)
    finally:
        absolute.close()
        percent.close()
    assert got_abs.shape == got_pct.shape == (14, 1, 8)
    assert_truth(got_abs[:, 0], sel, f"group B set {s} absolute")
    assert_truth(got_pct[:, 0], sel, f"group B set {s} percent of spot")
    assert same_bits(got_pct[:, 0, exact], got_abs[:, 0, exact])
    pairs, sel128 = pairs_of(native, 128)
    cols = [sel128.idx.index(i) for i in sel.idx]
    assert same_bits(got_abs[:, 0], pairs[:, cols])


# ---- g. the loss gradient and the Gauss-Newton Hessian ---------------------------------------------
@pytest.mark.parametrize("s", [8, 9])
def test_loss_gradient_and_gauss_newton_hessian_against_truth(native, s):
    """Group E: one surface of a set's 18 options with the fixture's market prices, loss_grad_rows
    and gauss_newton_rows at X = 0 but x[11] = mu_j -- the optimiser's point whose record is (1, 1,
    1, 1, 0, 1, 1, 1, 1, 0, 1, mu_j, 1) on any libm (exp(0) = 1, tanh(0) = 0), the fixture's set.
    The reference is composed from the fixture's truth planes s_im and prices p_m with math.fsum and
    nothing else:

        f    = (1 / M) sum_m ((p_m - mkt_m) / mkt_m)^2             (Feller: sigma^2 - 2 kappa theta
        g_i  = (2 / M) dt_i sum_m (p_m - mkt_m) / mkt_m^2 s_im      = -1 on both factors, asserted:
        H_ij = (2 / M) dt_i dt_j sum_m s_im s_jm / mkt_m^2          no penalty, no kink)

    dt = d theta / d x.  The bars are propagated from the plane bars: with dp_m, ds_im the
    device_bar * unit of each value,

        |df|    <= (1 / M) sum_m (2 |p_m - mkt_m| dp_m + dp_m^2) / mkt_m^2 + R
        |dg_i|  <= (2 / M) |dt_i| sum_m (dp_m |s_im| + |p_m - mkt_m| ds_im) / mkt_m^2 + R
        |dH_ij| <= (2 / M) |dt_i dt_j| sum_m (ds_im |s_jm| + |s_im| ds_jm + ds_im ds_jm) / mkt_m^2
                   + R

    R = 2 (ceil(M / 64) + 6 + 4) 2^-53 of the reduction's absolute sum, the rounding term of
    tests/test_gpu_gauss_newton.py.  H is exactly symmetric, and f, g of the two calls have equal
    bits."""
    sel = Cases(lambda c: c["group"] == "E" and c["set"] == s)
    M = len(sel)
    assert M == 18
    prm = np.array(fixture()["sets"][s])
    S0, r = sel.rec[0, 13], sel.rec[0, 14]
    mkt = np.array([c["mkt"] for c in sel.cases])
    assert np.all(mkt > 0)
    assert prm[3] ** 2 - 2 * prm[1] * prm[2] == -1.0 and prm[8] ** 2 - 2 * prm[6] * prm[7] == -1.0
    X = np.zeros((1, 13))
    X[0, 11] = prm[11]
    assert np.array_equal(R.O.to_params(X[0]), prm)
    dt = R.dtheta_dx(prm)
    assert np.array_equal(dt, np.ones(13))
    surf = native.Surface(native.default_context(), sel.K, sel.T, sel.call, mkt)
    try:
        f, g, bad = surf.loss_grad_rows(X, mkt[None, :], [S0], [r], [0], 128)
        f2, g2, bad2, H = surf.gauss_newton_rows(X, mkt[None, :], [S0], [r], [0], 128)
        own = surf.loss_grad(X, S0, r, 128)                     # the surface's own market prices
    finally:
        surf.close()
    assert bad[0] == 0 and bad2[0] == 0 and own[2][0] == 0
    assert same_bits(f, f2) and same_bits(g, g2)
    assert same_bits(own[0], f) and same_bits(own[1], g)
    assert same_bits(H, np.transpose(H, (0, 2, 1)))

    p, sens = sel.truth[0], sel.truth[1:]                       # [M], [13, M]
    dp, ds = sel.bar[0] * sel.unit[0], sel.bar[1:] * sel.unit[1:]
    assert np.all(np.isfinite(dp)) and np.all(np.isfinite(ds))
    rnd = 2.0 * (math.ceil(M / 64) + 6 + 4) * 2.0 ** -53
    w = (p - mkt) / mkt ** 2
    # the loss
    f_ref = math.fsum(((p - mkt) / mkt) ** 2) / M
    f_bar = math.fsum((2 * np.abs(p - mkt) * dp + dp ** 2) / mkt ** 2) / M + rnd * f_ref
    print(f"set {s}: f {f[0]:.17e} truth {f_ref:.17e} err / bar {abs(f[0] - f_ref) / f_bar:.3f}")
    assert abs(f[0] - f_ref) <= f_bar
    # the gradient
    worst_g = 0.0
    for i in range(13):
        ref = (2.0 / M) * dt[i] * math.fsum(w * sens[i])
        mag = (2.0 / M) * abs(dt[i]) * math.fsum(np.abs(w * sens[i]))
        bar = (2.0 / M) * abs(dt[i]) * math.fsum(
            (dp * np.abs(sens[i]) + np.abs(p - mkt) * ds[i]) / mkt ** 2) + rnd * mag
        print(f"set {s}: g[{R.PLANES[1 + i]}] {g[0, i]: .12e} truth {ref: .12e} "
              f"err / bar {abs(g[0, i] - ref) / bar:.3f} (bar {bar / mag:.1e} of the absolute sum)")
        worst_g = max(worst_g, abs(g[0, i] - ref) / bar)
        assert abs(g[0, i] - ref) <= bar, (R.PLANES[1 + i], g[0, i], ref, bar)
    # the Hessian
    worst_h = 0.0
    for i in range(13):
        for j in range(13):
            ref = (2.0 / M) * dt[i] * dt[j] * math.fsum(sens[i] * sens[j] / mkt ** 2)
            mag = (2.0 / M) * abs(dt[i] * dt[j]) * math.fsum(np.abs(sens[i] * sens[j]) / mkt ** 2)
            bar = (2.0 / M) * abs(dt[i] * dt[j]) * math.fsum(
                (ds[i] * np.abs(sens[j]) + np.abs(sens[i]) * ds[j] + ds[i] * ds[j]) / mkt ** 2) \
                + rnd * mag
            worst_h = max(worst_h, abs(H[0, i, j] - ref) / bar)
            assert abs(H[0, i, j] - ref) <= bar, (R.PLANES[1 + i], R.PLANES[1 + j], H[0, i, j],
                                                  ref, bar)
    print(f"set {s}: worst err / bar: g {worst_g:.3f}, H {worst_h:.3f}")
