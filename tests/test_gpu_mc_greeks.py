"""GPU tests of the coupled-path Monte Carlo Greeks (csrc/dh_mc_greeks.h): the
price plane against dh_mc_price's bits, the coupled walks against dh_mc_price on bumped records,
all five values and standard errors against the recomposition of dh_mc_paths' statistics
(tests/mc_greeks_reference.py), the statistical case against the restatement and against central
differences of the device's COS prices, the knock-out term of a barrier delta, and the refusals of
the C-ABI."""
import ctypes as C

import numpy as np
import pytest

import mc_greeks_reference as G
import mc_reference as R

pytestmark = pytest.mark.gpu

SPOT, RATE = 100.0, 0.03
SPY, SEED, N = 8, 11, 1000
EPS, BUMP = 1e-2, 5e-2
NOJUMP = R.README_PARAMS.copy()
NOJUMP[10] = 0.0
# a generic set with jumps, the same without, and one whose factor 1 sits on the exponential QE
# branch (psi > 1.5: v0 = 0.01, sigma = 1 at dt = 1/8; the test below counts its draws)
SETS = np.stack([R.README_PARAMS, NOJUMP, R.STRESSED_PARAMS])

MIX = [                                    # all four kinds, calls and puts, steps 2, 4, 8
    {"strike": 100.0, "maturity": 0.25, "option_type": "call"},
    {"strike": 95.0, "maturity": 1.0, "option_type": "put"},
    {"strike": 100.0, "maturity": 0.5, "option_type": "call", "kind": "asian"},
    {"strike": 105.0, "maturity": 1.0, "option_type": "put", "kind": "asian"},
    {"strike": 100.0, "maturity": 0.5, "option_type": "call", "kind": "up_and_out",
     "barrier": 120.0},
    {"strike": 110.0, "maturity": 1.0, "option_type": "put", "kind": "up_and_out",
     "barrier": 115.0},
    {"strike": 90.0, "maturity": 0.25, "option_type": "call", "kind": "down_and_out",
     "barrier": 92.0},
    {"strike": 100.0, "maturity": 1.0, "option_type": "put", "kind": "down_and_out",
     "barrier": 80.0},
    {"strike": 90.0, "maturity": 1.0, "option_type": "call", "kind": "up_and_out",
     "barrier": 115.0},                    # the knock-out edge: see test_knock_out_term
    {"strike": 0.0, "maturity": 1.0, "option_type": "call"},
]
KNOCK = 8
# 64 options: the mix at seven strike shifts, cut to the limit of a call
MANY = [dict(o, strike=max(o["strike"] + 2.0 * (k - 3), 0.0)) for k in range(7) for o in MIX][:64]
OBS = (2, 4, 8)


def _records(sets=SETS, spot=SPOT):
    from dhcos import _native
    sets = np.atleast_2d(sets)
    rec = np.zeros((len(sets), _native.PARAM_STRIDE))
    rec[:, :13] = sets
    rec[:, 13], rec[:, 14] = spot, RATE
    return rec


def _opts(options, spy=SPY):
    from dhcos.montecarlo import _options
    return _options(options, spy)


@pytest.fixture(scope="module")
def ctx():
    from dhcos import _native
    return _native.default_context()


@pytest.fixture(scope="module")
def mix_greeks(ctx):
    """value, stderr [3, 10, 5] of MIX under SETS at N paths.  Computed once; read-only."""
    value, err = ctx.mc_greeks(_records(), _opts(MIX), N, SPY, SEED, EPS, BUMP)
    value.setflags(write=False), err.setflags(write=False)
    return value, err


@pytest.mark.parametrize("n_paths", [2, 255, 256, 257, 1000])
def test_price_plane_is_the_pricers_bits(ctx, n_paths):
    """The PRICE plane and its stderr against dh_mc_price, bit for bit, at P = 1 and 3 and at 1 and
    64 options; the device-pointer form against the host form; the same call twice."""
    import torch
    for P in (1, 3):
        for options in (MIX[:1], MANY):
            rec, opts = _records(SETS[:P]), _opts(options)
            value, err = ctx.mc_greeks(rec, opts, n_paths, SPY, SEED, EPS, BUMP)
            price, perr = ctx.mc_price(rec, opts, n_paths, SPY, SEED)
            assert value.shape == err.shape == (P, len(options), 5)
            assert np.all(np.isfinite(value)) and np.all(np.isfinite(err))
            assert np.array_equal(value[..., 0], price), (P, len(options))
            assert np.array_equal(err[..., 0], perr), (P, len(options))
            again = ctx.mc_greeks(rec, opts, n_paths, SPY, SEED, EPS, BUMP)
            assert np.array_equal(again[0], value) and np.array_equal(again[1], err)
            d = ctx.mc_greeks_dev(torch.from_numpy(rec).to(f"cuda:{ctx.device}"), opts, n_paths,
                                  SPY, SEED, EPS, BUMP)
            ctx.synchronize()
            assert np.array_equal(d[0].cpu().numpy(), value)
            assert np.array_equal(d[1].cpu().numpy(), err)


def test_price_plane_when_a_block_sums_two_chunks(ctx):
    """More chunks than slots: the grid-stride loop runs twice for slot 0 (4 steps, 1,024 slots,
    n_paths = slots 256 + 256)."""
    options = [MIX[0], dict(MIX[3], maturity=1.0), dict(MIX[8], maturity=0.5)]
    rec, opts, n = _records(SETS[:1]), _opts(options, 4), 1024 * 256 + 256
    value, err = ctx.mc_greeks(rec, opts, n, 4, SEED, EPS, BUMP)
    price, perr = ctx.mc_price(rec, opts, n, 4, SEED)
    assert np.array_equal(value[..., 0], price) and np.array_equal(err[..., 0], perr)
    assert np.all(err > 0.0)


def _bumped_records():
    """[3, 7, 16]: per set the base record, spot u+, spot u-, then v0_1 +- d_1, v0_2 +- d_2."""
    out = []
    for p in SETS:
        sets = G.bumped_sets(p, BUMP)
        rec = _records(np.concatenate([sets[:1], sets[:1], sets]))
        rec[1, 13], rec[2, 13] = SPOT * (1.0 + EPS), SPOT * (1.0 - EPS)
        out.append(rec)
    return np.stack(out)


def test_coupled_walks_are_the_pricers_walks(ctx, mix_greeks):
    """delta, gamma and the vegas against the same differences of dh_mc_price's prices on records
    with the bumped spot or v0, same seed: 1e-10 of (|p+| + |p-|) / (2 bump), for gamma of
    (|p+| + 2 |p| + |p-|) / h^2.  Only u (S0 e^x) against (S0 u) e^x may differ, in the last ulp."""
    value, _ = mix_greeks
    rec = _bumped_records()
    price, _ = ctx.mc_price(rec.reshape(-1, rec.shape[-1]), _opts(MIX), N, SPY, SEED)
    p = price.reshape(3, 7, len(MIX))
    h = EPS * SPOT
    assert np.array_equal(p[:, 0], value[..., 0])
    for s in range(3):
        d1, d2 = BUMP * SETS[s, 0], BUMP * SETS[s, 5]
        base, sp, sm = p[s, 0], p[s, 1], p[s, 2]
        want = [(sp - sm) / (2.0 * h), ((sp - base) + (sm - base)) / (h * h),
                (p[s, 3] - p[s, 4]) / (2.0 * d1), (p[s, 5] - p[s, 6]) / (2.0 * d2)]
        bar = [1e-10 * (np.abs(sp) + np.abs(sm)) / (2.0 * h),
               1e-10 * (np.abs(sp) + 2.0 * np.abs(base) + np.abs(sm)) / (h * h),
               1e-10 * (np.abs(p[s, 3]) + np.abs(p[s, 4])) / (2.0 * d1),
               1e-10 * (np.abs(p[s, 5]) + np.abs(p[s, 6])) / (2.0 * d2)]
        for g in range(4):
            diff = np.abs(value[s, :, g + 1] - want[g])
            print(f"set {s} {G.NAMES[g + 1]}: worst |greeks - price difference| / bar "
                  f"{np.max(diff / np.maximum(bar[g], 1e-300)):.3e}")
            assert np.all(diff <= bar[g]), (s, G.NAMES[g + 1], diff, bar[g])
        assert np.any(value[s, :, 3] != 0.0) and np.any(value[s, :, 4] != 0.0)


@pytest.fixture(scope="module")
def bumped_paths(ctx):
    """dh_mc_paths of the base record and the four bumped-v0 records of each set at the options'
    steps: [3, 5, N, 3, 6]."""
    rec = _bumped_records()[:, [0, 3, 4, 5, 6]]
    out = ctx.mc_paths(rec.reshape(-1, rec.shape[-1]), OBS, 0, N, SPY, SEED)
    out = out.reshape(3, 5, N, len(OBS), 6)
    out.setflags(write=False)
    return out


def test_values_and_standard_errors_are_the_recomposition_of_the_paths(mix_greeks, bumped_paths):
    """All five values and standard errors against the host recomposition of dh_mc_paths'
    statistics: values to 1e-11 of the mean absolute sample, stderrs to 1e-9 relative."""
    value, err = mix_greeks
    for s in range(3):
        want, want_err, mean_abs = G.from_states(bumped_paths[s], OBS, SETS[s], SPOT, RATE, MIX,
                                                 SPY, EPS, BUMP)
        dv, de = np.abs(value[s] - want), np.abs(err[s] - want_err)
        with np.errstate(invalid="ignore", divide="ignore"):
            print(f"set {s}: worst |value - recomposition| / mean |sample| "
                  f"{np.nanmax(dv / mean_abs):.3e}, worst relative stderr difference "
                  f"{np.nanmax(de / want_err):.3e}")
        assert np.all(dv <= 1e-11 * mean_abs), (s, dv, mean_abs)
        assert np.all(de <= 1e-9 * want_err), (s, de, want_err)
        assert np.all(want_err[:, 1] > 0.0) and np.all(mean_abs[:9, 3:] > 0.0)
    # the third set's factor 1 walks the exponential branch, the first two the quadratic one
    stats = R.new_stats()
    R.simulate(SETS[2], SPOT, RATE, np.arange(64), 8, SPY, SEED, (), stats)
    assert stats["expo"] > 0 and stats["zero"] > 0 and stats["quad"] > 0


def test_knock_out_term_of_a_barrier_delta(mix_greeks, bumped_paths):
    """The up-and-out call whose barrier lies between max and u+ max on some paths that end in the
    money: its delta carries their -y_S- / (2 h), and is the recomposition's and the price
    difference's (the two tests above hold it to both)."""
    value, _ = mix_greeks
    o, state = MIX[KNOCK], bumped_paths[0, 0, :, 2]
    crossing = (state[:, 3] < o["barrier"]) & ((1.0 + EPS) * state[:, 3] >= o["barrier"]) \
        & ((1.0 - EPS) * state[:, 0] > o["strike"])
    assert crossing.sum() >= 3
    g = G.samples(bumped_paths[0][:, :, 2], SETS[0], SPOT, o, 8, EPS, BUMP)
    term = np.exp(-RATE) * g[1, crossing].sum() / N
    assert term < 0.0 and np.all(g[1, crossing] < 0.0)
    smooth = np.exp(-RATE) * g[1, ~crossing].sum() / N
    assert abs(value[0, KNOCK, 1] - (smooth + term)) <= 1e-12 * (abs(smooth) + abs(term))


@pytest.fixture(scope="module")
def stat_restatement():
    return G.greeks(G.STAT_PARAMS, G.STAT_SPOT, G.STAT_RATE, G.STAT_OPTIONS, G.STAT_PATHS,
                    G.STAT_SPY, G.STAT_SEED, G.STAT_SPOT_BUMP, G.STAT_V0_BUMP)


def test_statistical_case_against_the_restatement_and_cos(stat_restatement):
    """The CPU test's statistical case through the Python entry point: within 1e-9 relative of the
    restatement's figures, recomputed here, and delta, gamma and both vegas within 4 standard
    errors of the central differences of the device's COS prices (N = 512)."""
    import dhcos
    res = dhcos.monte_carlo_greeks(G.STAT_PARAMS, G.STAT_SPOT, G.STAT_RATE, G.STAT_OPTIONS,
                                   n_paths=G.STAT_PATHS, steps_per_year=G.STAT_SPY,
                                   seed=G.STAT_SEED, spot_bump=G.STAT_SPOT_BUMP,
                                   v0_bump=G.STAT_V0_BUMP)
    want, want_err = stat_restatement
    K = np.array([o["strike"] for o in G.STAT_OPTIONS])
    T = np.array([o["maturity"] for o in G.STAT_OPTIONS])
    call = np.array([o["option_type"] == "call" for o in G.STAT_OPTIONS])

    def cos(p, s):
        return dhcos.DoubleHeston.price_batch(np.tile(p, (K.size, 1)), s, K, T, G.STAT_RATE, call,
                                              N=512)

    diffs = (cos(G.STAT_PARAMS, G.STAT_SPOT),) + G.cos_differences(
        cos, G.STAT_PARAMS, G.STAT_SPOT, G.STAT_SPOT_BUMP, G.STAT_V0_BUMP)
    for g, name in enumerate(G.NAMES):
        got, got_err = getattr(res, name), getattr(res, name + "_stderr")
        rel = np.max(np.abs(got - want[:, g]) / np.abs(want[:, g]))
        rel_err = np.max(np.abs(got_err - want_err[:, g]) / want_err[:, g])
        z = np.abs(got - diffs[g]) / got_err
        print(f"{name}: device against restatement {rel:.2e} (stderr {rel_err:.2e}); "
              f"max |MC - COS difference| / stderr {z.max():.2f}")
        assert rel <= 1e-9 and rel_err <= 1e-9, name
        assert np.all(z <= 4.0), (name, z)
    one = dhcos.DoubleHeston(G.STAT_SPOT, 100.0, 0.25, G.STAT_RATE, *G.STAT_PARAMS,
                             option_type="call").monte_carlo_greeks(
        n_paths=4096, steps_per_year=G.STAT_SPY, seed=G.STAT_SEED)
    many = dhcos.monte_carlo_greeks(G.STAT_PARAMS, G.STAT_SPOT, G.STAT_RATE, G.STAT_OPTIONS[4:5],
                                    n_paths=4096, steps_per_year=G.STAT_SPY, seed=G.STAT_SEED)
    assert one.delta == many.delta[0] and one.vega_v02_stderr == many.vega_v02_stderr[0]


def test_refusals_name_the_argument(ctx):
    from dhcos import _native
    lib = _native.load()
    opts, out = _opts(MIX[:1]), np.empty((2, 3, 1, 5))

    def call(rec, eps, bump):
        return lib.dh_mc_greeks(ctx._h, rec.ctypes.data, len(rec), opts, 1, N, SPY, SEED, eps,
                                bump, out[0].ctypes.data, out[1].ctypes.data)

    rec = _records()
    for eps, bump, name in ((1.0, BUMP, b"spot_bump"), (float("nan"), BUMP, b"spot_bump"),
                            (EPS, 0.0, b"v0_bump"), (EPS, -0.1, b"v0_bump"),
                            (EPS, float("inf"), b"v0_bump")):
        assert call(rec, eps, bump) == -1
        assert name in lib.dh_last_error(), lib.dh_last_error()
    for col, name in ((0, b"v01 of set 2"), (5, b"v02 of set 2")):
        bad = _records()
        bad[2, col] = 0.0
        assert call(bad, EPS, BUMP) == -1
        assert name in lib.dh_last_error(), lib.dh_last_error()
    bad = _records()
    bad[1, 3] = -1.0                        # what dh_mc_price refuses
    assert call(bad, EPS, BUMP) == -1 and b"sigma1 of set 1" in lib.dh_last_error()
    assert lib.dh_mc_greeks(ctx._h, rec.ctypes.data, 3, opts, 1, 1, SPY, SEED, EPS, BUMP,
                            out[0].ctypes.data, out[1].ctypes.data) == -1
    assert b"n_paths" in lib.dh_last_error()
    assert lib.dh_mc_greeks_dev(ctx._h, None, 3, opts, 1, N, SPY, SEED, 2.0, BUMP, None, None,
                                None) == -1
    assert b"spot_bump" in lib.dh_last_error()
    assert C.sizeof(_native.McOption) == 32
