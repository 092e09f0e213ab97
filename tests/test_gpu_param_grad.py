"""GPU checks of the analytic parameter sensitivities and the loss gradient (dh_surface_param_sens*,
dh_param_sens_pairs, dh_surface_loss_grad*, gradient="analytic"): the device
against the NumPy restatement (tests/param_grad_reference.py) per plane, against Surface.price and
Surface.greeks, bit-reproducibility across tiles, P and the call forms, the loss and its gradient,
and a calibration run both ways.

Parity bar per plane i: |got - ref| <= 1e-6 |ref| + 1e-10 scale_i, scale_i = max |ref plane i| on
the surface -- the project's price parity rule carried to each plane's own unit."""
import functools

import numpy as np
import pytest

import param_grad_reference as R
from conftest import fd_grad_tol, rel_close
from oracle import dh_oracle as O

pytestmark = pytest.mark.gpu

S0, RATE = 100.0, 0.03
LO = np.array([0.025, 1.5, 0.025, 0.2, -0.85, 0.02, 0.3, 0.025, 0.1, -0.7, 0.05, -0.08, 0.03])
HI = np.array([0.08, 4.5, 0.065, 0.5, -0.4, 0.07, 1.2, 0.07, 0.35, -0.2, 0.25, -0.01, 0.12])
EPS_PRICE = 1e-13          # tests/test_gpu_parity.py's price noise of an FD gradient


@pytest.fixture(scope="module")
def native():
    from dhcos import _native
    if _native.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return _native


def records(seed, P):
    rs = np.random.RandomState(seed)
    rec = np.empty((P, 16))
    rec[:, :13] = LO + (HI - LO) * rs.rand(P, 13)
    rec[:, 13], rec[:, 14], rec[:, 15] = S0, RATE, 0.0
    return rec


def same_bits(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a).tobytes() == \
        np.ascontiguousarray(b).tobytes()


def assert_planes(got, want, label):
    scale = np.max(np.abs(want), axis=(1, 2), keepdims=True)
    err = np.abs(got - want)
    ok = err <= 1e-6 * np.abs(want) + 1e-10 * scale
    for i, name in enumerate(R.PLANES):
        print(f"{label} {name:9s}: worst |err| {err[i].max():.3e} = {np.max(err[i]) / scale[i, 0, 0]:.3e}"
              f" of max |plane| {scale[i, 0, 0]:.3e}")
    assert ok.all(), (label, [R.PLANES[i] for i in np.unique(np.argwhere(~ok)[:, 0])])


# ---- the cases, and their references (computed once) -------------------------------------------
def mixed_case():
    """3 sets x 36 options: 3 maturities x 12 strikes, calls and puts mixed, unsorted."""
    rs = np.random.RandomState(21)
    T = np.repeat([0.1, 0.8, 2.0], 12)
    K = S0 * rs.uniform(0.8, 1.2, 36)
    call = rs.rand(36) < 0.5
    order = rs.permutation(36)
    return records(31, 3), K[order], T[order], call[order]


def tile_case():
    """One maturity, 257 options: tiles of 256 and 1."""
    rs = np.random.RandomState(22)
    return records(32, 1), S0 * rs.uniform(0.8, 1.2, 257), np.full(257, 0.7), rs.rand(257) < 0.5


def clamp_case():
    """tests/test_gpu_greeks.py's clamp surface: the six clamp strikes at T = 0.1 in one tile with
    14 neighbours near the money, under the three sets that test draws.  The neighbours give every
    plane its unit for the parity rule: on the six strikes alone every option is so far from the
    money that max |plane| is 1e-6 (kappa2) to 3e-3 (v1_0), and a floor of 1e-10 of that falls below
    the fp64 rounding of the restatement itself (1.0e-12 on theta1 against an extended-precision
    evaluation, 3e-3 of that floor's unit).  The six strikes are therefore held a second time, to a
    bar in units of that rounding: test_clamped_options_... below."""
    rs = np.random.RandomState(7)
    K = np.concatenate([[5.0, 40.0, 60.0, 250.0, 500.0, 3000.0], S0 * rs.uniform(0.9, 1.1, 14)])
    call = rs.rand(20) < 0.5
    order = rs.permutation(20)
    return records(13, 3), K[order], np.full(20, 0.1), call[order]


@functools.lru_cache(maxsize=None)
def reference(name, N):
    rec, K, T, call = {"mixed": mixed_case, "clamp": clamp_case}[name]()
    return R.sens_surface(rec, K, T, call, N)


def surface_planes(native, rec, K, T, call, N):
    surf = native.Surface(native.default_context(), K, T, call)
    try:
        return surf.param_sens(rec, N)
    finally:
        surf.close()


# ---- device against the restatement ---------------------------------------------------------------
@pytest.mark.parametrize("N", [128, 1024])
def test_planes_match_the_restatement(native, N):
    rec, K, T, call = mixed_case()
    got = surface_planes(native, rec, K, T, call, N)
    assert got.shape == (14, 3, 36)
    assert_planes(got, reference("mixed", N), f"mixed N={N}")


def test_tile_boundary_leaves_the_bits_alone(native):
    """257 options of one maturity split into tiles of 256 and 1; 36 of them, from both tiles,
    priced alone (one tile) have the same bits."""
    rec, K, T, call = tile_case()
    sub = np.r_[np.arange(0, 245, 7), 256]
    assert sub.size == 36
    ctx = native.default_context()
    big, small = native.Surface(ctx, K, T, call), native.Surface(ctx, K[sub], T[sub], call[sub])
    try:
        assert big.n_tiles == 2 and small.n_tiles == 1
        whole = big.param_sens(rec, 128)
        alone = small.param_sens(rec, 128)
    finally:
        big.close()
        small.close()
    assert np.isfinite(whole).all()
    assert same_bits(whole[:, :, sub], alone)


def test_clamped_options_match_the_restatement_on_their_own_range(native):
    import greeks_reference as G
    rec, K, T, call = clamp_case()
    active = np.array([[G.clamp_active(r[:13], S0, k, 0.1, RATE) for k in K] for r in rec])
    print("clamp-active strikes per set:", [K[a].tolist() for a in active])
    assert active.sum() == 13 and not active[:, K == 60.0].any()  # K = 60 is never clamped
    assert not active[:, (K > 89.0) & (K < 111.0)].any()
    surf = native.Surface(native.default_context(), K, T, call)
    try:
        got = surf.param_sens(rec, 128)
        greeks = surf.greeks(rec, 128)
    finally:
        surf.close()
    for i, g in ((0, 0), (1, 4), (6, 5)):          # the per-term path against the Greeks' one
        d = np.abs(got[i] - greeks[g])
        print(f"{R.PLANES[i]} against the Greeks kernel on the clamp surface: worst {d.max():.3e}")
        assert np.all(d <= 1e-6 * np.abs(greeks[g]) + 1e-10 * np.max(np.abs(greeks[g])))
    want = reference("clamp", 128)
    print("smallest |price| on the clamp surface:", np.abs(want[0]).min())
    assert_planes(got, want, "clamp N=128")
    # The six far strikes (18 pairs, 13 of them on the per-term path) against a higher-precision
    # evaluation: the restatement's expressions on the same fp64 inputs and ranges in x87 extended
    # arithmetic (eps 1.1e-19; against the 50-digit fixture it is good to 1e-17 of a plane).  The
    # unit of the bar is fp64's own rounding of these sums, plane by plane: E_i = the fp64
    # restatement's worst |error| against that evaluation over the 18 pairs (measured here, on the
    # host; 4.5e-15 for lambda_j to 1.0e-12 for theta1).  The restatement rounds with libm (<= 1
    # ulp) and IEEE division (0.5 ulp); the device's primitives are held to 2 ulp and cdiv_rcp to
    # 6 ulp of |z| ("The characteristic function"), up to 12 times as much: the bar is
    # 16 E_i (the next power of two), beside the parity rule's relative part.
    far = np.isin(K, [5.0, 40.0, 60.0, 250.0, 500.0, 3000.0])
    assert far.sum() == 6 and active[:, far].sum() == 13
    exact = R.sens_surface(rec, K[far], T[far], call[far], 128, extended=True)
    own = np.max(np.abs(want[:, :, far] - exact), axis=(1, 2))
    err = np.abs(got[:, :, far] - exact)
    bar = 1e-6 * np.abs(exact) + 16.0 * own[:, None, None]
    for i, name in enumerate(R.PLANES):
        print(f"six strikes {name:9s}: restatement's own error {own[i]:.2e}, device worst "
              f"{err[i].max():.2e} = {err[i].max() / own[i]:.2f} of it (bar 16)")
    assert np.all(own > 0)
    assert np.all(err <= bar), [R.PLANES[i] for i in np.unique(np.argwhere(err > bar)[:, 0])]


# ---- consistency with the other requests --------------------------------------------------------
def test_price_and_v0_planes_match_price_and_greeks_and_the_call_forms_agree(native):
    import torch
    import dhcos
    rec, K, T, call = mixed_case()
    P, M, N = 3, K.size, 128
    ctx = native.default_context()
    surf = native.Surface(ctx, K, T, call)
    try:
        got = surf.param_sens(rec, N)
        prices = surf.price(rec, N)
        greeks = surf.greeks(rec, N)
        dev = torch.device("cuda", ctx.device)
        d_rec = torch.from_numpy(rec).to(dev)
        d_out = torch.full((14, P, M), -1.0, dtype=torch.float64, device=dev)
        stream = torch.cuda.Stream(device=dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream):
            surf.param_sens_dev(d_rec.data_ptr(), P, d_out.data_ptr(), N=N,
                                stream=stream.cuda_stream)
        stream.synchronize()
        assert same_bits(d_out.cpu().numpy(), got)
    finally:
        surf.close()
    print("max |price plane - Surface.price|", np.max(np.abs(got[0] - prices)))
    assert rel_close(got[0], prices, 1e-11, 1e-11).all()
    for i, g in ((1, 4), (6, 5)):
        scale = np.max(np.abs(greeks[g]))
        err = np.abs(got[i] - greeks[g])
        print(f"{R.PLANES[i]} against the Greeks' vega: worst {err.max():.3e}")
        assert np.all(err <= 1e-6 * np.abs(greeks[g]) + 1e-10 * scale)
    # the Greeks kernel's price plane, by the same rule (no bit-for-bit promise: the two kernels
    # share their source expressions, not their FMA contraction inside dh_device.h's functions)
    print("max |price plane - the Greeks' price plane|", np.max(np.abs(got[0] - greeks[0])))
    assert np.all(np.abs(got[0] - greeks[0]) <= 1e-6 * np.abs(greeks[0])
                  + 1e-10 * np.max(np.abs(greeks[0])))
    pairs = ctx.param_sens_pairs(np.repeat(rec, M, axis=0), np.tile(K, P), np.tile(T, P),
                                 np.tile(call, P), N)
    assert same_bits(pairs.reshape(14, P, M), got)
    opts = [{"strike": k, "maturity": t, "option_type": "call" if c else "put"}
            for k, t, c in zip(K, T, call)]
    top = dhcos.parameter_sensitivities(rec[:, :13], S0, RATE, opts, N=N)
    one = dhcos.parameter_sensitivities(dict(zip(dhcos.calibrator.PARAM_NAMES, rec[1, :13])), S0,
                                        RATE, opts, N=N)
    m = 5
    single = dhcos.DoubleHeston(S0=S0, K=K[m], T=T[m], r=RATE, option_type=opts[m]["option_type"],
                                **dict(zip(dhcos.pricer.MODEL_FIELDS, rec[2, :13]))
                                ).parameter_sensitivities(N)
    for i, name in enumerate(R.PLANES):
        assert same_bits(getattr(top, name), got[i]), name
        assert same_bits(getattr(one, name), got[i, 1]), name
        assert np.float64(getattr(single, name)).tobytes() == got[i, 2, m].tobytes(), name


def test_same_call_same_bits_and_a_set_does_not_depend_on_P(native):
    rec14 = records(33, 14)
    _, K, T, call = mixed_case()
    surf = native.Surface(native.default_context(), K, T, call)
    try:
        a = surf.param_sens(rec14, 128)
        b = surf.param_sens(rec14, 128)
        alone = [surf.param_sens(rec14[p:p + 1], 128) for p in (0, 9, 13)]
    finally:
        surf.close()
    assert np.isfinite(a).all() and same_bits(a, b)
    for p, one in zip((0, 9, 13), alone):
        assert same_bits(one, a[:, p:p + 1]), p


def test_refusals_name_the_argument(native):
    lib = native.load()
    rec, K, T, call = mixed_case()
    ctx = native.default_context()
    surf = native.Surface(ctx, K, T, call)                   # no market prices
    with_mkt = native.Surface(ctx, K, T, call, np.ones(36))
    empty = native.Surface(ctx, K[:0], T[:0], call[:0], np.ones(0))
    out = np.empty((14, 3, 36))
    x = np.tile(R.O.from_params(rec[0, :13]), (3, 1))
    f, g, bad = np.empty(3), np.empty((3, 13)), np.empty(3, np.int32)

    def sens(ctx_h=ctx.handle, s=surf.handle, prm=rec.ctypes.data, P=3, N=128, L=10.0,
             o=out.ctypes.data):
        return lib.dh_surface_param_sens(ctx_h, s, prm, P, N, L, o)

    def loss(ctx_h=ctx.handle, s=with_mkt.handle, xs=x.ctypes.data, S=3, spot=S0, r=RATE, N=128,
             L=10.0, fo=f.ctypes.data, go=g.ctypes.data, bo=bad.ctypes.data):
        return lib.dh_surface_loss_grad(ctx_h, s, xs, S, spot, r, N, L, fo, go, bo)

    def loss_dev(**kw):
        a = dict(s=with_mkt.handle, xs=x.ctypes.data, S=3, spot=S0, r=RATE, N=128, L=10.0,
                 fo=f.ctypes.data, go=g.ctypes.data, bo=bad.ctypes.data)
        a.update(kw)
        return lib.dh_surface_loss_grad_dev(ctx.handle, a["s"], a["xs"], a["S"], a["spot"], a["r"],
                                            a["N"], a["L"], a["fo"], a["go"], a["bo"], None)

    try:
        for call_, kw, word in [
                (sens, dict(N=0), b"N"), (sens, dict(N=native.PARAM_GRAD_MAX_N + 1), b"N"),
                (sens, dict(N=2048), b"N"), (sens, dict(P=0), b"P"), (sens, dict(L=0.0), b"L"),
                (sens, dict(ctx_h=None), b"ctx"), (sens, dict(s=None), b"surface"),
                (sens, dict(prm=None), b"params"), (sens, dict(o=None), b"out"),
                (loss, dict(N=0), b"N"), (loss, dict(N=1025), b"N"), (loss, dict(S=0), b"S"),
                (loss, dict(S=-2), b"S"), (loss, dict(L=0.0), b"L"),
                (loss, dict(ctx_h=None), b"ctx"), (loss, dict(s=None), b"surface"),
                (loss, dict(s=surf.handle), b"surface has no market"),
                (loss, dict(s=empty.handle), b"surface is empty"),
                (loss, dict(spot=0.0), b"S0"), (loss, dict(spot=-1.0), b"S0"),
                (loss, dict(spot=float("nan")), b"S0"), (loss, dict(spot=float("inf")), b"S0"),
                (loss, dict(r=float("nan")), b"r"), (loss, dict(r=float("inf")), b"r"),
                (loss, dict(xs=None), b"x"), (loss, dict(fo=None), b"f"),
                (loss, dict(go=None), b"g"), (loss, dict(bo=None), b"bad"),
                (loss_dev, dict(N=1025), b"N"), (loss_dev, dict(S=0), b"S"),
                (loss_dev, dict(spot=0.0), b"S0"), (loss_dev, dict(r=float("nan")), b"r"),
                (loss_dev, dict(s=surf.handle), b"surface has no market"),
                (loss_dev, dict(xs=None), b"x"), (loss_dev, dict(fo=None), b"f"),
                (loss_dev, dict(go=None), b"g"), (loss_dev, dict(bo=None), b"bad")]:
            assert call_(**kw) == -1, (call_.__name__, kw)               # DH_E_ARG
            assert lib.dh_last_error().startswith(word + b" "), (kw, lib.dh_last_error())
        assert sens() == 0 and np.isfinite(out).all()                    # and still usable
        assert loss() == 0 and np.isfinite(f).all() and np.isfinite(g).all() and not bad.any()
    finally:
        surf.close()
        with_mkt.close()
        empty.close()


# ---- the loss and its gradient -----------------------------------------------------------------
def test_loss_grad_rows(native, calib_golden):
    """S = 3 on the 15-option market: guesses_seed0[1] (Feller slack on one factor), the literature
    start (factor 2 on the Feller kink) and x = 5 (NaN prices)."""
    from dhcos import DoubleHestonJumpCalibrator as Cal
    market = calib_golden["test_market"]
    X = np.array([calib_golden["guesses_seed0"][1], calib_golden["guesses_seed0"][0],
                  np.full(13, 5.0)])
    cal = Cal(100.0, 0.05, market, gradient="analytic")
    f, g, low = cal.fg_batch(X)
    assert cal.loss_evals == 3
    bad = cal._get_surface().loss_grad(X, 100.0, 0.05)[2]
    f_fd = Cal(100.0, 0.05, market).loss_batch(X)
    print("f", f, "loss_batch", f_fd, "bad", bad)
    assert np.all(np.abs(f - f_fd) <= 1e-9 * np.abs(f_fd))
    assert bad[2] > 0 and bad[0] == 0 and bad[1] == 0
    assert f[2] == 1e10 and not g[2].any() and np.signbit(g[2]).sum() == 0
    assert low[0] == f[0] and low[1] == f[1] and low[2] == np.inf
    # the restatement
    ref = [R.loss_grad(x, market, 100.0, 0.05) for x in X[:2]]
    for row in (0, 1):
        want = ref[row][1]
        tol = 1e-6 * np.abs(want) + 1e-10 * np.max(np.abs(want))
        err = np.abs(g[row] - want)
        if row == 1:
            # On the kink sigma2^2 - 2 kappa2 theta2 is zero to an ulp, and its sign is that of the
            # last bits of three exponentials: the device's exp need not round as NumPy's does.
            # Either one-sided derivative is the contract there; the other ten components are not
            # touched by the penalty.
            p = O.to_params(X[1])
            other = want.copy()
            kink = np.array([0.0] * 6 + [-2000.0 * p[6] * p[7]] * 2 + [2000.0 * p[8] ** 2]
                            + [0.0] * 4)
            assert not R.feller_grad_x(p)[:6].any()            # factor 1 has no slack here
            other += kink if R.feller_grad_x(p)[8] == 0.0 else -kink
            err = np.minimum(err, np.abs(g[row] - other))
        for i, n in enumerate(O.PARAM_NAMES):
            print(f"row {row} {n:9s} g {g[row, i]: .9e} ref {want[i]: .9e} err {err[i]:.2e}")
        assert np.all(err <= tol), (row, [O.PARAM_NAMES[i] for i in np.flatnonzero(err > tol)])
    # off the kink the forward-difference gradient agrees within its own bar
    fd = Cal(100.0, 0.05, market)
    f0, g_fd = fd.compute_loss_and_grad(X[0])
    from dhcos.calibrator import fd_request_points
    dx = fd_request_points(X[0])[1]
    bar = fd_grad_tol(g_fd, f0, dx, EPS_PRICE)
    print("analytic - FD:", np.abs(g[0] - g_fd), "bar", bar)
    assert np.all(np.abs(g[0] - g_fd) <= bar)
    # compute_loss_and_grad follows the switch
    f1, g1 = cal.compute_loss_and_grad(X[0])
    assert f1 == f[0] and same_bits(g1, g[0]) and cal.n_calls == 1


def test_loss_grad_dev_gives_the_host_forms_bits(native, calib_golden):
    import torch
    market = calib_golden["test_market"]
    X = np.array(calib_golden["guesses_seed0"][:3])
    K = np.array([o["strike"] for o in market], dtype=np.float64)
    T = np.array([o["maturity"] for o in market])
    mkt = np.array([o["price"] for o in market])
    ctx = native.default_context()
    surf = native.Surface(ctx, K, T, np.ones(15, bool), mkt)
    try:
        f, g, bad = surf.loss_grad(X, 100.0, 0.05, 256)
        dev = torch.device("cuda", ctx.device)
        d_x = torch.from_numpy(X).to(dev)
        d_f = torch.empty(3, dtype=torch.float64, device=dev)
        d_g = torch.empty((3, 13), dtype=torch.float64, device=dev)
        d_bad = torch.empty(3, dtype=torch.int32, device=dev)
        stream = torch.cuda.Stream(device=dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream):
            surf.loss_grad_dev(d_x.data_ptr(), 3, 100.0, 0.05, d_f.data_ptr(), d_g.data_ptr(),
                               d_bad.data_ptr(), N=256, stream=stream.cuda_stream)
        stream.synchronize()
        one = surf.loss_grad(X[1:2], 100.0, 0.05, 256)
    finally:
        surf.close()
    assert same_bits(d_f.cpu().numpy(), f) and same_bits(d_g.cpu().numpy(), g)
    assert np.array_equal(d_bad.cpu().numpy(), bad)
    assert one[0][0] == f[1] and same_bits(one[1][0], g[1])               # S = 1 against S = 3


# ---- calibration both ways --------------------------------------------------------------------
def test_calibration_with_the_analytic_gradient_converges_where_fd_does(native, calib_golden):
    """One start at get_initial_guess(1) under seed 0, maxiter 300.  Trajectories are chaotic
    (DESIGN.md 2): neither x nor nit is compared.  The analytic run must report convergence and end
    within a decade of the FD run's loss."""
    from dhcos import DoubleHestonJumpCalibrator as Cal
    market = calib_golden["test_market"]
    runs = {}
    for gradient in ("fd", "analytic"):
        np.random.seed(0)
        cal = Cal(100.0, 0.05, market, gradient=gradient)
        x0 = cal.get_initial_guess(1)
        res = cal.calibrate(maxiter=300, multi_start=1, x0s=[x0])
        runs[gradient] = res
        print(f"{gradient}: start loss {Cal(100.0, 0.05, market).compute_loss(x0):.6e} final "
              f"{res.final_loss:.6e} nit {res.iterations} requests {cal.lockstep_launches} "
              f"loss evaluations {cal.loss_evals} n_calls {cal.n_calls} {res.message!r}")
        if gradient == "analytic":                 # one loss evaluation per request
            assert cal.n_calls == cal.lockstep_launches == cal.loss_evals
    an, fd = runs["analytic"], runs["fd"]
    assert an.success or "CONVERGENCE" in an.message, an.message
    assert np.isfinite(an.final_loss) and an.final_loss <= 10.0 * fd.final_loss
