"""The surface's spot cache (dh_surface_stage_spot, Surface.stage_spot): a staged surface gives the
bits of an unstaged one -- prices, sse and n_bad, np.array_equal -- on the smallest shapes that
reach each build of the fused request kernel, through PATH_FUSED and PATH_SPLIT; records that
carry another spot or a NaN fall back set by set; and one oracle check at the 1e-10 bar, so that
"equal" cannot mean "equally wrong".

Shapes (strikes x maturities, one tile per maturity):
* 5 x 3, N = 128, 14 sets: the one-option-per-lane-group fused build;
* 32 x 2, N = 256, 14 sets: a one-round grid of two groups (tables mapped to blocks by XCD);
* 100 x 2, N = 512, 3 sets: four options per lane group on G = 10 lanes, reduced through LDS;
* 100 x 2, N = 512, 513 sets: 1,026 tables, more than one round of resident blocks (256 CUs x 4),
  so later blocks read the prologue records formed ahead;
* 5 x 3, one start's function+gradient request: 14 records in the launch's kernel arguments.
"""
import numpy as np
import pytest

from conftest import rel_close
from oracle import dh_oracle as O

pytestmark = pytest.mark.gpu

S0, R = 100.0, 0.03
LO = np.array([0.025, 1.5, 0.025, 0.2, -0.85, 0.02, 0.3, 0.025, 0.1, -0.7, 0.05, -0.08, 0.03])
HI = np.array([0.08, 4.5, 0.065, 0.5, -0.4, 0.07, 1.2, 0.07, 0.35, -0.2, 0.25, -0.01, 0.12])


@pytest.fixture(scope="module")
def native():
    from dhcos import _native
    if _native.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return _native


def _records(P, seed, spot=S0):
    params = LO + (HI - LO) * np.random.RandomState(seed).rand(P, 13)
    rec = np.empty((P, 16))
    rec[:, :13], rec[:, 13], rec[:, 14], rec[:, 15] = params, spot, R, 0.0
    return params, rec


def _options(nK, nT, seed, lo=0.8, hi=1.2):
    """nK strikes at each of nT maturities, puts and calls; market = a smooth positive curve (the
    loss only needs mkt > 0)."""
    rs = np.random.RandomState(seed)
    T = np.repeat(np.linspace(0.25, 1.5, nT) if nT > 1 else np.array([0.75]), nK)
    K = S0 * rs.uniform(lo, hi, T.size)
    call = rs.rand(T.size) < 0.5
    mkt = 5.0 + 2.0 * np.cos(np.arange(float(T.size)))
    return K, T, call, mkt


def _with_path(ctx, path, fn):
    ctx.set_path(path)
    try:
        return fn()
    finally:
        ctx.set_path(0)


def _request(native, surf, rec, N):
    """Everything a request returns, through both paths: prices, then (sse, n_bad, prices) with
    and (sse, n_bad) without price columns."""
    ctx = surf.ctx
    out = []
    for path in (native.PATH_FUSED, native.PATH_SPLIT):
        out.append(_with_path(ctx, path, lambda: surf.price(rec, N)))
        assert ctx.last_path == path
        out.extend(_with_path(ctx, path, lambda: surf.loss_terms(rec, N, want_prices=True)))
        out.extend(_with_path(ctx, path, lambda: surf.loss_terms(rec, N))[:2])
    return out


def _same(got, want):
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b, equal_nan=True), (k, np.argwhere(~(a == b))[:4].tolist())


def _pair(native, K, T, call, mkt, spot=S0, mode=None):
    """(a surface staged at spot, the same surface never staged)"""
    ctx = native.default_context()
    mode = native.STRIKE_ABSOLUTE if mode is None else mode
    staged = native.Surface(ctx, K, T, call, mkt, strike_mode=mode)
    staged.stage_spot(spot)
    return staged, native.Surface(ctx, K, T, call, mkt, strike_mode=mode)


GRIDS = {"5x3_N128": (5, 3, 128, 14), "32x2_N256": (32, 2, 256, 14), "100x2_N512": (100, 2, 512, 3),
         "100x2_N512_ahead": (100, 2, 512, 513)}


@pytest.mark.parametrize("name", list(GRIDS))
def test_staged_equals_unstaged(native, name):
    nK, nT, N, P = GRIDS[name]
    K, T, call, mkt = _options(nK, nT, 7 + nK)
    params, rec = _records(P, 11 + nK + P)
    staged, plain = _pair(native, K, T, call, mkt)
    got, want = _request(native, staged, rec, N), _request(native, plain, rec, N)
    _same(got, want)
    assert np.isfinite(got[0]).all()
    if P <= 14:      # "equal" is not "equally wrong": the oracle's prices at the usual bar
        ref = np.stack([O.price_many(params[p], S0, K, T, R, call, N) for p in range(min(P, 3))])
        err = np.max(np.abs(got[0][:len(ref)] - ref) / (1e-10 * np.abs(ref) + 1e-10))
        print(f"{name}: max error / bar {err:.3g}")
        assert rel_close(got[0][:len(ref)], ref, 1e-10, 1e-10).all(), err
    staged.close()
    plain.close()


def test_one_start_request_records_in_kernel_arguments(native):
    """A one-start function+gradient request: 14 records in the fused launch's kernel arguments
    (the KP build), and the split launches of the same request."""
    from dhcos.calibrator import fd_models
    K, T, call, mkt = _options(5, 3, 21)
    x0 = np.array([O.from_params(_records(1, 22)[0][0])])
    staged, plain = _pair(native, K, T, call, mkt)
    for path in (native.PATH_AUTO, native.PATH_FUSED, native.PATH_SPLIT):
        got = _with_path(staged.ctx, path, lambda: staged.fg(x0, S0, R, 128, model=fd_models(x0)))
        want = _with_path(plain.ctx, path, lambda: plain.fg(x0, S0, R, 128, model=fd_models(x0)))
        _same(got, want)
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    staged.close()
    plain.close()


def test_other_spot_and_nan_spot_fall_back_set_by_set(native):
    K, T, call, mkt = _options(5, 3, 31)
    _, rec = _records(4, 32)
    rec[1:3, :13] = rec[0, :13]           # sets 0, 1, 2: one model, three spots
    rec[1, 13] = 101.0
    rec[2, 13] = np.nan
    staged, plain = _pair(native, K, T, call, mkt)
    got, want = _request(native, staged, rec, 128), _request(native, plain, rec, 128)
    _same(got, want)
    pr = got[0]
    assert np.isfinite(pr[[0, 1, 3]]).all() and np.isnan(pr[2]).all()
    assert not np.array_equal(pr[0], pr[1])           # the record's own spot priced set 1
    staged.close()
    plain.close()


def test_clamp_widened_options(native):
    """Strikes so far out at a short maturity that the truncation range is widened for them (the
    clamp mask, decided from the staged log-moneyness): clamped and other prices equal, and the
    oracle's."""
    T = np.full(5, 0.02)
    K = S0 * np.array([0.5, 0.9, 1.0, 1.1, 2.0])
    call = np.array([True, False, True, False, True])
    params, rec = _records(2, 41)
    for p in params:      # the unwidened range leaves both far strikes' +-0.1 windows outside
        a, b = O.trunc_range(p, S0, S0, 0.02, R)
        assert np.log(0.5) - 0.1 < a and np.log(2.0) + 0.1 > b
    ref = np.stack([O.price_many(p, S0, K, T, R, call, 128) for p in params])
    staged, plain = _pair(native, K, T, call, np.abs(ref[0]) + 1e-3)
    got, want = _request(native, staged, rec, 128), _request(native, plain, rec, 128)
    _same(got, want)
    assert rel_close(got[0], ref, 1e-10, 1e-10).all()
    staged.close()
    plain.close()


def test_percent_of_spot_surface_and_restaging(native):
    """A STRIKE_PCT_SPOT surface staged at one spot, priced with records at that spot and at
    another; then restaged at the other spot."""
    K, T, call, mkt = _options(5, 3, 51)
    K = K / S0 * 100.0                                # K_relative
    params, rec = _records(4, 52)
    rec[2:, 13] = 105.0
    staged, plain = _pair(native, K, T, call, mkt, mode=native.STRIKE_PCT_SPOT)
    want = _request(native, plain, rec, 128)
    _same(_request(native, staged, rec, 128), want)
    staged.stage_spot(105.0)
    _same(_request(native, staged, rec, 128), want)
    ref = np.stack([O.price_many(params[p], rec[p, 13], K * rec[p, 13] / 100.0, T, R, call, 128)
                    for p in range(4)])
    assert rel_close(want[0], ref, 1e-10, 1e-10).all()
    with pytest.raises(RuntimeError):
        staged.stage_spot(float("nan"))
    staged.close()
    plain.close()


def test_restaging_an_absolute_surface(native):
    K, T, call, mkt = _options(32, 2, 61)
    _, rec = _records(4, 62)
    rec[::2, 13] = 97.5
    staged, plain = _pair(native, K, T, call, mkt)
    want = _request(native, plain, rec, 256)
    _same(_request(native, staged, rec, 256), want)
    staged.stage_spot(97.5)
    _same(_request(native, staged, rec, 256), want)
    staged.close()
    plain.close()


def test_unstaged_surface_after_a_staged_one(native):
    """The context's next request on a surface never staged, of another size, after a staged
    surface's: the bits it gave before (no cache pointer survives in the launch arguments)."""
    Ka, Ta, ca, ma = _options(32, 2, 71)
    Kb, Tb, cb, mb = _options(5, 3, 72)
    _, rec = _records(3, 73)
    ctx = native.default_context()
    plain = native.Surface(ctx, Kb, Tb, cb, mb)
    before = _request(native, plain, rec, 128)
    staged = native.Surface(ctx, Ka, Ta, ca, ma)
    staged.stage_spot(S0)
    _request(native, staged, rec, 128)
    _same(_request(native, plain, rec, 128), before)
    staged.close()
    _same(_request(native, plain, rec, 128), before)
    plain.close()
