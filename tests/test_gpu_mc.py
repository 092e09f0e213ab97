"""GPU tests of the Monte Carlo path pricer (csrc/dh_mc.h): the library's paths
against the NumPy restatement (tests/mc_reference.py) and against the 50-digit walk of the step
(tests/golden/mc_truth.npz) with the high words of key and counter live, the CIR moments of the
variance factors, its prices against the reduction of its own paths (one chunk per block and
several, the full option table, barrier ties, ragged path counts, degenerate parameters), bitwise
identities and reproducibility (back-to-back device-pointer calls included), the model check
against the COS pricer, and the refusals of the C-ABI."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import mc_reference as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SPOT, RATE = 100.0, 0.03
U = 2.0 ** -53
SPY, OBS, SEED = 8, (2, 4, 8), 1          # the small walk of tests 1-4: dt = 1/8, T = 1/4, 1/2, 1
N_SMALL = 320                              # a full chunk + one full wave: a partial chunk
SETS = np.stack([R.README_PARAMS, R.STRESSED_PARAMS])

MIX = [                                    # all four kinds, calls and puts, three maturities
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
    {"strike": 0.0, "maturity": 1.0, "option_type": "call"},
]


def _records(sets=SETS):
    from dhcos import _native
    rec = np.zeros((len(sets), _native.PARAM_STRIDE))
    rec[:, :13] = sets
    rec[:, 13], rec[:, 14] = SPOT, RATE
    return rec


@pytest.fixture(scope="module")
def ctx():
    from dhcos import _native
    return _native.default_context()


@pytest.fixture(scope="module")
def reference_paths():
    """The restatement's statistics [2, 320, 3, 6] of paths 0..319 under both sets, and its branch
    counts.  Computed once; read-only."""
    stats = R.new_stats()
    obs = np.stack([R.simulate(p, SPOT, RATE, np.arange(N_SMALL), OBS[-1], SPY, SEED, OBS, stats)[1]
                    for p in SETS])
    obs.setflags(write=False)
    return obs, stats


@pytest.fixture(scope="module")
def device_paths(ctx):
    out = ctx.mc_paths(_records(), OBS, 0, N_SMALL, SPY, SEED)
    out.setflags(write=False)
    return out


def _parity_ratio(got, want):
    """Worst |got - want| over its bar: 1e-10 relative on all six statistics, plus 1e-14 absolute
    on the two variances."""
    bar = 1e-10 * np.abs(want)
    bar[..., 1:3] += 1e-14
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(got == want, 0.0, np.abs(got - want) / bar)
    return float(np.max(ratio))


def test_paths_match_the_restatement(ctx, reference_paths, device_paths):
    want, stats = reference_paths
    # the inputs reach every branch of the step, none within rounding of a switch
    assert stats["quad"] > 0 and stats["expo"] > 0 and stats["zero"] > 0, stats
    assert stats["n1"] > 0 and stats["n2"] > 0, stats
    assert stats["psi_gap"] > 1e-9 and stats["u_gap"] > 1e-9, stats
    assert np.all(np.isfinite(device_paths))
    r0 = _parity_ratio(device_paths, want)
    # paths 1000..1063: the stream is indexed by the path, not by the lane
    far = np.stack([R.simulate(p, SPOT, RATE, np.arange(1000, 1064), OBS[-1], SPY, SEED, OBS)[1]
                    for p in SETS])
    r1 = _parity_ratio(ctx.mc_paths(_records(), OBS, 1000, 64, SPY, SEED), far)
    print(f"mc path parity: worst |device - restatement| / bar = {r0:.3e} (paths 0..319), "
          f"{r1:.3e} (paths 1000..1063); bar 1e-10 relative (+1e-14 on v1, v2); branch counts "
          f"{stats}")
    assert r0 <= 1.0 and r1 <= 1.0


def _option_array(options, spy=SPY):
    from dhcos.montecarlo import _options
    return _options(options, spy)


def _steps(options, spy=SPY):
    return [int(round(o["maturity"] * spy)) for o in options]


def _reduction_bars(pay, disc):
    """(price, its bar, stderr, its bar) of the payoffs `pay` of n paths, by math.fsum.
    With A = sum |payoff|, s2 = sum payoff^2, V = s2 - s1^2 / n and u = 2^-53, any order of
    summation keeps |d s1| <= (n - 1) u A, so the price bar is e^{-rT} (n - 1) u A / n.  For the
    standard error e^{-rT} sqrt(V / (n (n - 1))): |d s2| <= n u s2 (the squares' roundings
    included), |d (s1^2 / n)| <= 2 n u A^2 / n, the subtraction adds u V, so |dV| <= dV := n u s2 +
    2 u A^2 + u V, and |sqrt(V + d) - sqrt(V)| <= min(|d| / (2 sqrt V), sqrt |d|); four more
    roundings (division, square root, discount) add 4 u of the result."""
    n = pay.size
    s1, A, s2 = math.fsum(pay), math.fsum(np.abs(pay)), math.fsum(pay * pay)
    V = math.fsum((pay - s1 / n) ** 2)
    want_p = disc * s1 / n
    want_e = disc * math.sqrt(V / (n * (n - 1)))
    bar_p = disc * (n - 1) * U * A / n + 4 * U * abs(want_p)
    dV = n * U * s2 + 2 * U * A * A + U * V
    dsq = min(dV / (2 * math.sqrt(V)), math.sqrt(dV)) if V > 0 else math.sqrt(dV)
    bar_e = disc * dsq / math.sqrt(n * (n - 1)) + 4 * U * want_e
    return want_p, bar_p, want_e, bar_e


def _assert_reduction(price, err, options, paths, obs, where=()):
    """price, err [n_options] of one parameter set against the math.fsum reduction of payoffs
    formed in NumPy from that set's paths [n, len(obs), 6], to the bars of _reduction_bars."""
    for j, (o, st) in enumerate(zip(options, _steps(options))):
        pay = R.payoff(o.get("kind", "european"), o["option_type"] == "call", o["strike"],
                       o.get("barrier", 0.0), st, paths[:, obs.index(st)])
        want_p, bar_p, want_e, bar_e = _reduction_bars(pay, math.exp(-RATE * o["maturity"]))
        assert abs(price[j] - want_p) <= bar_p, (*where, j, price[j], want_p, bar_p)
        assert abs(err[j] - want_e) <= bar_e, (*where, j, err[j], want_e, bar_e)


def test_prices_are_the_reduction_of_the_librarys_own_paths(ctx, device_paths):
    """price and stderr against math.fsum over payoffs formed in NumPy from dh_mc_paths' output,
    to the summation bounds derived in _reduction_bars."""
    price, err = ctx.mc_price(_records(), _option_array(MIX), N_SMALL, SPY, SEED)
    for p in range(len(SETS)):
        _assert_reduction(price[p], err[p], MIX, device_paths[p], OBS, (p,))
    assert np.all(price[:, :8] > 0)        # every option of the mix pays on some path


def test_identities_hold_bitwise(ctx):
    eu = [{"strike": 100.0, "maturity": 0.5, "option_type": t} for t in ("call", "put")]
    opts = eu + [dict(o, kind="up_and_out", barrier=1e300) for o in eu] \
        + [dict(o, kind="down_and_out", barrier=1e-300) for o in eu] \
        + [dict(o, maturity=1.0 / SPY, kind=k) for o in eu for k in ("european", "asian")] \
        + [{"strike": 0.0, "maturity": 0.5, "option_type": "call"}]
    price, err = ctx.mc_price(_records(), _option_array(opts), N_SMALL, SPY, SEED)
    for a in (price, err):
        assert np.array_equal(a[:, 0:2], a[:, 2:4])        # a barrier never reached, above
        assert np.array_equal(a[:, 0:2], a[:, 4:6])        # and below
        assert np.array_equal(a[:, [6, 8]], a[:, [7, 9]])  # the one-date average is S_T
    # put-call parity against the same run's forward, to the three prices' reduction bounds
    call, put, fwd = price[:, 0], price[:, 1], price[:, 10]
    k_disc = 100.0 * math.exp(-RATE * 0.5)
    bar = (N_SMALL - 1) * U * (call + put + fwd) + 4 * U * k_disc
    assert np.all(np.abs(call - put - (fwd - k_disc)) <= bar), (call - put - (fwd - k_disc), bar)


def test_results_are_reproducible_bitwise(ctx, device_paths):
    import torch
    opts = _option_array(MIX)
    three = np.stack([R.README_PARAMS, R.STRESSED_PARAMS, 0.5 * (R.README_PARAMS
                                                                 + R.STRESSED_PARAMS)])
    n = 3 * 256 + 7                        # three chunks and a ragged fourth
    a = ctx.mc_price(_records(three), opts, n, SPY, SEED)
    b = ctx.mc_price(_records(three), opts, n, SPY, SEED)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for p in range(3):                     # a set alone is the set in the batch
        alone = ctx.mc_price(_records(three[p:p + 1]), opts, n, SPY, SEED)
        assert np.array_equal(alone[0][0], a[0][p]) and np.array_equal(alone[1][0], a[1][p])
    more = ctx.mc_paths(_records(), OBS, 0, 576, SPY, SEED)
    assert np.array_equal(more[:, :N_SMALL], device_paths)
    rec = torch.from_numpy(_records(three)).to(f"cuda:{ctx.device}")
    d_price, d_err = ctx.mc_price_dev(rec, opts, n, SPY, SEED)
    ctx.synchronize()
    assert np.array_equal(d_price.cpu().numpy(), a[0])
    assert np.array_equal(d_err.cpu().numpy(), a[1])
    # another seed is another sample
    assert not np.array_equal(ctx.mc_price(_records(three), opts, n, SPY, SEED + 1)[0], a[0])


def test_prices_agree_with_the_cos_pricer():
    """2^19 paths at 32 steps per year, seed 2024, the generator's grid as calls and as puts:
    every |MC - COS(N = 512)| <= 4 stderr, the forward within 4 of its standard errors of spot at
    each maturity.  4 is the statistical bar alone (no allowance for time-step bias)."""
    import dhcos
    grid = [{"strike": float(k), "maturity": float(t), "option_type": ot}
            for ot in ("call", "put") for k, t in zip(R.GRID_K, R.GRID_T)]
    fwds = [{"strike": 0.0, "maturity": t, "option_type": "call"} for t in (0.25, 0.5, 1.0)]
    res = dhcos.monte_carlo(R.README_PARAMS, SPOT, RATE, grid + fwds, n_paths=1 << 19,
                            steps_per_year=32, seed=2024)
    assert res.price.shape == (33,) and res.stderr.shape == (33,)
    cos = dhcos.DoubleHeston.price_batch(R.README_PARAMS, SPOT, np.tile(R.GRID_K, 2),
                                         np.tile(R.GRID_T, 2), RATE,
                                         [o["option_type"] for o in grid], N=512)
    z = np.abs(res.price[:30] - cos) / res.stderr[:30]
    zf = np.abs(res.price[30:] - SPOT) / res.stderr[30:]
    print(f"mc vs COS: max |MC - COS| / stderr {z.max():.2f} over 30 options; forward "
          f"{zf.max():.2f}")
    assert np.all(z <= 4.0), z
    assert np.all(zf <= 4.0), zf
    lo, hi = res.confidence()
    assert np.all(lo < res.price) and np.all(res.price < hi)
    # the instance method prices its own option from the same paths
    dh = dhcos.DoubleHeston(SPOT, 105.0, 0.5, RATE, *R.README_PARAMS, option_type="call")
    p, e = dh.monte_carlo(n_paths=1 << 19, steps_per_year=32, seed=2024)
    j = next(i for i, o in enumerate(grid) if o["strike"] == 105.0 and o["maturity"] == 0.5)
    assert p == res.price[j] and e == res.stderr[j]


def _set(**kw):
    names = ["v01", "kappa1", "theta1", "sigma1", "rho1", "v02", "kappa2", "theta2", "sigma2",
             "rho2", "lambda_j", "mu_j", "sigma_j", "spot", "rate"]
    rec = _records(SETS[:1])
    for k, v in kw.items():
        rec[0, names.index(k)] = v
    return rec


REFUSALS = {                               # case -> (call arguments, the name in the message)
    "nan": (dict(rec=_set(mu_j=np.nan)), "mu_j"),
    "inf rate": (dict(rec=_set(rate=np.inf)), "rate"),
    "v0": (dict(rec=_set(v02=-0.01)), "v02"),
    "kappa": (dict(rec=_set(kappa1=0.0)), "kappa1"),
    "theta": (dict(rec=_set(theta2=-0.1)), "theta2"),
    "sigma": (dict(rec=_set(sigma1=0.0)), "sigma1"),
    "rho": (dict(rec=_set(rho2=1.0)), "rho2"),
    "lambda": (dict(rec=_set(lambda_j=-1.0)), "lambda_j"),
    "lambda dt": (dict(rec=_set(lambda_j=8.5)), "lambda_j"),
    "sigma_j": (dict(rec=_set(sigma_j=-0.1)), "sigma_j"),
    "spot": (dict(rec=_set(spot=0.0)), "spot"),
    "n_paths": (dict(n_paths=1), "n_paths"),
    "steps_per_year": (dict(spy=0), "steps_per_year"),
    "maturity": (dict(opt=(0, 1, 100.0, 0.3, 0.0)), "maturity"),
    "kind": (dict(opt=(4, 1, 100.0, 0.5, 0.0)), "kind"),
    "barrier": (dict(opt=(2, 1, 100.0, 0.5, 0.0)), "barrier"),
    "barrier below": (dict(opt=(3, 0, 100.0, 0.5, -1.0)), "barrier"),
    "n_options": (dict(n_opt=0), "n_options"),
    "n_options 65": (dict(n_opt=65), "n_options"),         # DH_MC_MAX_OPTIONS + 1
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_the_abi_refuses_bad_arguments_before_any_launch(ctx, case):
    from dhcos import _native
    kw, name = REFUSALS[case]
    rec = kw.get("rec", _records(SETS[:1]))
    n_arr = max(1, kw.get("n_opt", 1))                     # as many records as the call names
    opts = (_native.McOption * n_arr)(*[_native.McOption(*kw.get("opt", (0, 1, 100.0, 0.5, 0.0)))
                                        for _ in range(n_arr)])
    price, err = np.full(n_arr, -7.0), np.full(n_arr, -7.0)
    lib = _native.load()
    rc = lib.dh_mc_price(ctx.handle, rec.ctypes.data, 1, opts, kw.get("n_opt", 1),
                         kw.get("n_paths", 512), kw.get("spy", SPY), 0, price.ctypes.data,
                         err.ctypes.data)
    assert rc == -1                                        # DH_E_ARG
    assert name in lib.dh_last_error().decode()
    assert np.all(price == -7.0) and np.all(err == -7.0)
    if "rec" in kw:                                        # the validation export checks the same
        out = np.full(6, -7.0)
        obs = np.array([1], dtype=np.int32)
        rc = lib.dh_mc_paths(ctx.handle, rec.ctypes.data, 1, 1, obs.ctypes.data, 0, 1, SPY, 0,
                             out.ctypes.data)
        assert rc == -1 and name in lib.dh_last_error().decode() and np.all(out == -7.0)


# ---- paths against the 50-digit truth, the high words of key and counter live ---------------------
TRUTH_RANGES = ((0, 24), (1000, 4), ((1 << 32) - 1, 3), (5 * (1 << 32) + 77, 1))
STATS = ("S", "v1", "v2", "max", "min", "sum")


@pytest.fixture(scope="module")
def truth():
    with np.load(os.path.join(GOLDEN, R.TRUTH_FILE)) as z:
        return {k: z[k] for k in z.files}


def test_paths_match_the_50_digit_truth(ctx, truth):
    """dh_mc_paths against the mpmath walk of the step (tests/golden/mc_truth.npz): seed
    0x9E3779B900000005, path ranges whose high counter word is 0, 1 and 5, one of them carrying
    from 2^32 - 1 into the high word inside a wave; the four sets of the fixture.

    Bar: per statistic, 16 x the NumPy restatement's own stored worst relative error against the
    same truth (floored at 2^-53), and on the variances 16 x its stored absolute error on top.
    The kernel's exp, log and sincos are documented within 1 ulp (dsincos 2) where NumPy's are
    within about half an ulp, and the errors accumulate alike over the eight steps: 16 admits
    that and sits four decades under the 1e-10 of the parity test above.  An exact 0 of the truth
    is an exact 0."""
    hi, lo = truth["truth"], truth["truth_lo"]
    assert [int(p) for p in truth["paths"]] == [p0 + i for p0, n in TRUTH_RANGES for i in range(n)]
    rec = _records(truth["sets"])
    assert (float(truth["spot"]), float(truth["rate"])) == (SPOT, RATE)
    got = np.concatenate([ctx.mc_paths(rec, truth["obs_steps"], p0, n, int(truth["steps_per_year"]),
                                       int(truth["seed"])) for p0, n in TRUTH_RANGES], axis=1)
    assert got.shape == hi.shape and np.all(np.isfinite(got))
    zero = hi == 0.0
    assert np.all(got[zero] == 0.0) and np.all(got[~zero] != 0.0)
    rel, ab = R.truth_errors(got, hi, lo)
    ref_rel = np.maximum(truth["rel_err"], U)
    print("mc paths vs 50-digit truth: worst relative error, device / restatement: "
          + ", ".join(f"{s} {a:.2e} / {b:.2e} = {a / b:.2f}" for s, a, b in zip(STATS, rel, ref_rel))
          + f"; absolute on v1, v2: device {ab}, restatement {truth['abs_err']}")
    bar = 16.0 * ref_rel * np.abs(hi)
    bar[..., 1:3] += 16.0 * truth["abs_err"]
    d = np.abs((got - hi) - lo)
    worst = np.where(zero, 0.0, d / np.where(zero, 1.0, bar)).reshape(-1, 6).max(axis=0)
    assert np.all(worst <= 1.0), dict(zip(STATS, worst))


def test_both_high_words_reach_the_generator(ctx):
    rec = _records(SETS[:1])

    def spot_of(path, seed):
        return ctx.mc_paths(rec, (1,), path, 1, SPY, seed)[0, 0, 0, 0]
    assert spot_of(0, R.TRUTH_SEED) != spot_of(0, R.TRUTH_SEED & 0xFFFFFFFF)     # seed 5
    assert R.TRUTH_SEED & 0xFFFFFFFF == 5
    assert spot_of(77, R.TRUTH_SEED) != spot_of(5 * (1 << 32) + 77, R.TRUTH_SEED)


# ---- the CIR moments: a check that does not pass through the restatement of the step -------------
def test_variance_factors_have_the_cir_moments(ctx):
    """2^16 paths, 8 steps per year, step 8, seed 0x9E3779B900000005, both sets: the sample mean
    and variance of v1 and v2 within 4 of their standard errors of the CIR closed forms, the
    discounted mean of S_T within 4 of its own of spot (mc_reference.moment_z_scores derives the
    closed forms; tests/test_mc.py runs the same function on the restatement, worst 1.05)."""
    out = ctx.mc_paths(_records(), (8,), 0, 1 << 16, 8, R.TRUTH_SEED)
    for p, params in enumerate(SETS):
        z = R.moment_z_scores(params, out[p, :, 0], SPOT, RATE, 1.0)
        print(f"mc moments, set {p}: " + ", ".join(f"{k} {v:.2f}" for k, v in z.items()))
        assert all(v <= 4.0 for v in z.values()), (p, z)


# ---- exact reduction where a block walks several chunks ------------------------------------------
def test_reduction_is_exact_over_several_chunks_per_block(ctx):
    """2 * 1024 * 256 + 256 + 7 paths: 2050 chunks over 1024 slots, so slot 0 walks three chunks,
    slot 1 two and a ragged third, every other slot two; five options of all four kinds at steps
    2 and 8 against the reduction of the library's own paths."""
    n = 2 * 1024 * 256 + 256 + 7
    opts = [{"strike": 100.0, "maturity": 0.25, "option_type": "call"},
            {"strike": 105.0, "maturity": 0.25, "option_type": "put", "kind": "asian"},
            {"strike": 100.0, "maturity": 1.0, "option_type": "call", "kind": "up_and_out",
             "barrier": 130.0},
            {"strike": 100.0, "maturity": 1.0, "option_type": "put", "kind": "down_and_out",
             "barrier": 70.0},
            {"strike": 95.0, "maturity": 1.0, "option_type": "put"}]
    rec = _records(SETS[1:2])
    paths = ctx.mc_paths(rec, (2, 8), 0, n, SPY, R.TRUTH_SEED)[0]
    price, err = ctx.mc_price(rec, _option_array(opts), n, SPY, R.TRUTH_SEED)
    _assert_reduction(price[0], err[0], opts, paths, (2, 8))
    assert np.all(price > 0)


# ---- the full option table ------------------------------------------------------------------------
def _full_table():
    """64 options at 8 steps per year: 42 at step 8, 12 at step 4, 10 at step 2; the first 16 in
    descending order of maturity, the rest shuffled; every kind as call and as put; the last four
    repeat entries 0, 17, 30 and 45."""
    rs = np.random.RandomState(64)
    steps = [8] * 6 + [4] * 5 + [2] * 5 + list(rs.permutation([8] * 36 + [4] * 7 + [2] * 1))
    kinds = ["european", "asian", "up_and_out", "down_and_out"]
    table = []
    for j, st in enumerate(steps):
        o = {"strike": float(80 + 5 * (j % 9)), "maturity": st / SPY,
             "option_type": ("call", "put")[(j // 4) % 2], "kind": kinds[j % 4]}
        if o["kind"] == "up_and_out":
            o["barrier"] = float(110 + 3 * (j % 11))
        if o["kind"] == "down_and_out":
            o["barrier"] = float(95 - 2 * (j % 13))
        table.append(o)
    return table + [dict(table[k]) for k in (0, 17, 30, 45)]


FULL = _full_table()
DUPLICATES = ((60, 0), (61, 17), (62, 30), (63, 45))


def test_the_full_option_table(ctx, device_paths):
    assert len(FULL) == 64 and _steps(FULL).count(8) >= 40 and set(_steps(FULL)) == set(OBS)
    assert _steps(FULL) != sorted(_steps(FULL)) and _steps(FULL)[:16] == sorted(_steps(FULL)[:16],
                                                                                reverse=True)
    assert {(o["kind"], o["option_type"]) for o in FULL} == {(k, t) for k in R.KINDS
                                                             for t in ("call", "put")}
    price, err = ctx.mc_price(_records(), _option_array(FULL), N_SMALL, SPY, SEED)
    for p in range(len(SETS)):
        _assert_reduction(price[p], err[p], FULL, device_paths[p], OBS, (p,))
    assert np.count_nonzero(price > 0) > 100               # 128 entries; most of the table pays
    for a in (price, err):
        for dup, first in DUPLICATES:
            assert np.array_equal(a[:, dup], a[:, first]), (dup, first)
    # a permuted list gives the permuted outputs: each result lands at its caller's index
    perm = np.random.RandomState(7).permutation(64)
    assert not np.array_equal(perm, np.arange(64))
    p_price, p_err = ctx.mc_price(_records(), _option_array([FULL[k] for k in perm]), N_SMALL, SPY,
                                  SEED)
    assert np.array_equal(p_price, price[:, perm]) and np.array_equal(p_err, err[:, perm])
    assert len({x for x in price[0]}) > 40                  # the columns are told apart


# ---- ties on a barrier, ragged path counts ---------------------------------------------------------
def test_a_barrier_on_an_attained_extreme_knocks_out(ctx, device_paths):
    """max < H and min > H are strict: a barrier set to exactly the running maximum (minimum) a
    path attains knocks that path out.  Per set: an up-and-out put (strike 110) with H the maximum
    of an in-the-money path at step 8, a down-and-out call (strike 90) with H the minimum of one."""
    j8 = OBS.index(8)
    opts, picked = [], []
    for p in range(len(SETS)):
        S, mx, mn = (device_paths[p][:, j8, c] for c in (0, 3, 4))
        itm = np.flatnonzero(S < 110.0)                     # the median maximum among them: other
        i = itm[np.argsort(mx[itm])[itm.size // 2]]         # paths fall on either side of H
        opts.append({"strike": 110.0, "maturity": 1.0, "option_type": "put", "kind": "up_and_out",
                     "barrier": float(mx[i])})
        itm = np.flatnonzero(S > 90.0)
        k = itm[np.argsort(mn[itm])[itm.size // 2]]
        opts.append({"strike": 90.0, "maturity": 1.0, "option_type": "call",
                     "kind": "down_and_out", "barrier": float(mn[k])})
        picked += [(p, i), (p, k)]
    # the inputs discriminate: with <= (>=) the tied path pays, so the sums differ
    for o, (p, i) in zip(opts, picked):
        st = device_paths[p][:, j8]
        call = o["option_type"] == "call"
        strict = R.payoff(o["kind"], call, o["strike"], o["barrier"], 8, st)
        lax = R.payoff("european", call, o["strike"], 0.0, 8, st)
        lax = np.where(st[:, 3] <= o["barrier"] if o["kind"] == "up_and_out"
                       else st[:, 4] >= o["barrier"], lax, 0.0)
        assert strict[i] == 0.0 and lax[i] > 0.0
        assert math.fsum(strict) != math.fsum(lax) and math.fsum(strict) > 0.0
    price, err = ctx.mc_price(_records(), _option_array(opts), N_SMALL, SPY, SEED)
    for p in range(len(SETS)):
        _assert_reduction(price[p], err[p], opts, device_paths[p], OBS, (p,))


@pytest.mark.parametrize("n", [2, 65, 257])
def test_ragged_path_counts(ctx, device_paths, n):
    """Two lanes of one wave; one wave and one lane of the next; one chunk and one lane of the
    next: the inactive lanes and waves pay 0 and the divisor is n."""
    price, err = ctx.mc_price(_records(), _option_array(MIX), n, SPY, SEED)
    for p in range(len(SETS)):
        _assert_reduction(price[p], err[p], MIX, device_paths[p][:n], OBS, (p, n))
    if n == 2:                                              # sqrt(((a - m)^2 + (b - m)^2) / 2)
        for j in (1, 8):                                    # the put and the forward at step 8
            st = device_paths[0][:2, OBS.index(8)]
            a, b = R.payoff("european", j == 8, MIX[j]["strike"], 0.0, 8, st)
            want = math.exp(-RATE) * abs(a - b) / 2.0
            assert abs(err[0, j] - want) <= _reduction_bars(np.array([a, b]), math.exp(-RATE))[3]
            assert a != b or j == 1                         # the two forwards differ


# ---- legal degenerate parameters -------------------------------------------------------------------
def test_degenerate_parameters_price(ctx):
    """The fixture's third and fourth sets (v0 = 0 without jumps at |rho| = 0.999; lambda dt = 1
    with sigma_j = 0): finite prices that are the reduction of the library's own paths."""
    rec = _records(R.TRUTH_SETS[2:])
    paths = ctx.mc_paths(rec, OBS, 0, N_SMALL, SPY, SEED)
    price, err = ctx.mc_price(rec, _option_array(MIX), N_SMALL, SPY, SEED)
    assert np.all(np.isfinite(paths)) and np.all(np.isfinite(price)) and np.all(np.isfinite(err))
    for p in range(2):
        _assert_reduction(price[p], err[p], MIX, paths[p], OBS, (p,))
    assert np.all(price[:, [0, 1, 8]] > 0)


def test_jump_size_is_inert_without_jumps(ctx):
    """lambda_j = 0: the drift is r dt and the jump term +-0 whatever mu_j and sigma_j, so two
    sets that differ only in those give the same bits; with v0 = 0 too, S after one step is
    finite and positive on every path."""
    a = R.ZERO_V0_PARAMS
    b = a.copy()
    b[11], b[12] = 0.3, 0.5
    assert a[10] == b[10] == 0.0 and a[11] != b[11] and a[12] != b[12]
    paths = ctx.mc_paths(_records(np.stack([a, b])), (1, 8), 0, N_SMALL, SPY, SEED)
    assert np.array_equal(paths[0], paths[1])
    price, err = ctx.mc_price(_records(np.stack([a, b])), _option_array(MIX), N_SMALL, SPY, SEED)
    assert np.array_equal(price[0], price[1]) and np.array_equal(err[0], err[1])
    s1 = paths[0][:, 0, 0]
    assert np.all(np.isfinite(s1)) and np.all(s1 > 0.0) and np.ptp(s1) > 0.0


# ---- back-to-back device-pointer calls -------------------------------------------------------------
def test_device_pointer_calls_back_to_back(ctx):
    """Eight dh_mc_price_dev calls queued on one stream of a fresh context without a
    synchronisation between them, alternating 3 and 40 options and 263 and 775 paths (the second
    call regrows the partial-sum scratch the first allocated; every call rewrites the option
    records the one before read): each equals the same call made alone."""
    import torch
    from dhcos import _native
    three = np.stack([R.README_PARAMS, R.STRESSED_PARAMS, 0.5 * (R.README_PARAMS
                                                                 + R.STRESSED_PARAMS)])
    lists = (MIX[:3], FULL[:40])
    counts = (263, 3 * 256 + 7)
    calls = [(lists[i % 2], counts[(i + i // 2) % 2], R.TRUTH_SEED + i) for i in range(8)]
    assert (len(calls[0][0]), calls[0][1]) == (3, 263) and (len(calls[1][0]), calls[1][1]) == (40,
                                                                                               775)
    assert {(len(o), n) for o, n, _ in calls} == {(3, 263), (3, 775), (40, 263), (40, 775)}
    rec = torch.from_numpy(_records(three)).to(f"cuda:{ctx.device}")
    fresh = _native.Context(ctx.device)
    try:
        outs = [fresh.mc_price_dev(rec, _option_array(o), n, SPY, seed) for o, n, seed in calls]
        fresh.synchronize()
        outs = [(p.cpu().numpy(), e.cpu().numpy()) for p, e in outs]
    finally:
        fresh.close()
    for (o, n, seed), (price, err) in zip(calls, outs):
        alone = ctx.mc_price(_records(three), _option_array(o), n, SPY, seed)
        assert np.array_equal(price, alone[0]) and np.array_equal(err, alone[1]), (len(o), n)
