"""GPU tests of the least-squares Monte Carlo pricer of American and Bermudan options
(csrc/dh_lsm.h): the device against the NumPy restatement of the backward pass
(tests/lsm_reference.py) on the device's own paths -- every path's exercise date, the skipped
dates, the coefficients to the conditioning of the Gram matrix, the prices to the reordering of a
sum -- on ragged path counts, two chunks per block, idle options and 1 and 16 options; one
exercise date; degenerate dates; reproducibility and independence; the Black-Scholes limit against
a binomial tree; and the refusals of the C-ABI."""
import json
import os

import numpy as np
import pytest

import lsm_reference as L
import mc_reference as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SPOT, RATE, SPY, EVERY, SEED = L.DEV_SPOT, L.DEV_RATE, L.DEV_SPY, L.DEV_EVERY, L.DEV_SEED
SETS = np.stack([R.README_PARAMS, R.STRESSED_PARAMS])          # jumps on in both
NAMES = ("price", "stderr", "european", "european_stderr")


@pytest.fixture(scope="module")
def ctx():
    from dhcos import _native
    return _native.default_context()


def _records(sets, spot=SPOT, rate=RATE):
    from dhcos import _native
    sets = np.atleast_2d(sets)
    rec = np.zeros((len(sets), _native.PARAM_STRIDE))
    rec[:, :13] = sets
    rec[:, 13], rec[:, 14] = spot, rate
    return rec


def _lsm(ctx, sets, options, n_paths, spy=SPY, every=EVERY, seed=SEED, policy=True, **kw):
    """dh_lsm_price -> dict of price, stderr, european, european_stderr, coef, exercise_date."""
    from dhcos.american import _options
    opts, dates = _options(options, spy, every)
    out = ctx.lsm_price(_records(sets, **kw), opts, dates, n_paths, spy, every, seed, policy=policy)
    return dict(zip(NAMES + ("coef", "exercise_date"), out))


def _same_bits(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def _assert_matches_restatement(ctx, sets, options, n_paths):
    """The comparison of test 4.  Exercise dates and skipped dates equal; coefficients within
    64 eps cond(G) |beta| per fitted date, cond(G) from NumPy's Gram matrix; the four prices
    within n_paths eps relative (the worst case of reordering a sum of n_paths non-negative
    terms).  First, on these very paths, the restatement's own decisions must not hang on its
    solver."""
    sets = np.atleast_2d(sets)
    dates = SPY // EVERY
    got = _lsm(ctx, sets, options, n_paths)
    states = ctx.mc_paths(_records(sets), np.arange(EVERY, SPY + 1, EVERY), 0, n_paths, SPY, SEED)
    assert got["coef"].shape == (len(sets), len(options), dates, 10)
    assert got["exercise_date"].shape == (len(sets), len(options), n_paths)
    worst_c = worst_p = 0.0
    for p, params in enumerate(sets):
        want = L.restate(states[p], params, options)
        alt = L.restate(states[p], params, options, solver="lstsq")
        assert np.array_equal(want["exercise_date"], alt["exercise_date"])
        assert np.array_equal(got["exercise_date"][p], want["exercise_date"]), \
            int(np.sum(got["exercise_date"][p] != want["exercise_date"]))
        skipped = np.isnan(want["coef"][..., 0])
        assert np.array_equal(np.isnan(got["coef"][p]), np.isnan(want["coef"]))
        assert not skipped.all() and np.any(want["exercise_date"] < dates)
        for j, d in zip(*np.nonzero(~skipped)):
            beta = want["coef"][j, d]
            bar = 64 * EPS * np.linalg.cond(want["gram"][j, d]) * np.linalg.norm(beta)
            err = np.linalg.norm(got["coef"][p, j, d] - beta)
            worst_c = max(worst_c, err / bar)
            assert err <= bar, (p, j, d, err, bar)
        for k in NAMES:
            rel = np.abs(got[k][p] - want[k]) / np.abs(want[k])
            worst_p = max(worst_p, float(rel.max()))
            assert np.all(rel <= n_paths * EPS), (k, p, rel)
    print(f"lsm vs restatement, {n_paths} paths, {len(options)} options: worst coefficient error "
          f"/ bar {worst_c:.2e}, worst relative price error {worst_p:.2e} (bar "
          f"{n_paths * EPS:.2e})")
    return got


def test_device_matches_the_restatement_on_its_own_paths(ctx):
    """Test 4: 4096 paths, 8 exercise dates (exercise_every 4 at 32 steps a year), 3 puts and a
    call with 8 and 4 dates, two parameter sets."""
    _assert_matches_restatement(ctx, SETS, L.DEV_OPTIONS, 4096)


def test_partial_last_chunk(ctx):
    """1000 paths: the lanes past the end enter no regression and no mean."""
    _assert_matches_restatement(ctx, SETS, L.DEV_OPTIONS, 1000)


def test_two_chunks_per_block_and_sixteen_options(ctx):
    """256 LSM_SLOTS + 300 paths: the first block walks two chunks, the second of them partial;
    16 options with 1, 2, 4 and 8 dates, so most go idle in the early launches."""
    from dhcos import _native
    got = _assert_matches_restatement(ctx, SETS[0], L.DEV_OPTIONS_16,
                                      256 * _native.LSM_SLOTS + 300)
    assert sorted(set(L.option_columns(L.DEV_OPTIONS_16)[2])) == [1, 2, 4, 8]
    assert np.all(np.isfinite(got["price"]))


def test_one_option(ctx):
    _assert_matches_restatement(ctx, SETS[1], L.DEV_OPTIONS[:1], 1000)


def test_one_exercise_date_is_the_european_option(ctx):
    """exercise_every = the maturity step: price == european bit for bit, and european is
    dh_mc_price's European value of the same seed, paths and steps to the order of a sum."""
    from dhcos.montecarlo import _options as mc_options
    options = [{"strike": k, "maturity": 0.5, "option_type": t}
               for k, t in ((95.0, "put"), (100.0, "put"), (105.0, "call"))]
    n = 4096
    got = _lsm(ctx, SETS, options, n, every=SPY // 2)
    assert np.array_equal(got["price"], got["european"])
    assert np.array_equal(got["stderr"], got["european_stderr"])
    assert np.all(np.isnan(got["coef"])) and np.all(got["exercise_date"] == 1)
    price, err = ctx.mc_price(_records(SETS), mc_options(options, SPY), n, SPY, SEED)
    assert np.all(np.abs(got["european"] - price) <= n * EPS * price)
    assert np.all(np.abs(got["european_stderr"] - err) <= n * EPS * err)


def test_degenerate_dates(ctx):
    """A put struck at 1% of spot has no path in the money: every date is skipped, price ==
    european bit for bit, no NaN in a price.  A put struck at 10 x spot has every path in the
    money at every date and prices finite."""
    deep = [{"strike": 1.0, "maturity": 1.0, "option_type": "put"},
            {"strike": 1000.0, "maturity": 1.0, "option_type": "put"}]
    got = _lsm(ctx, SETS, deep, 4096)
    assert np.all(np.isnan(got["coef"][:, 0]))
    assert np.all(got["exercise_date"][:, 0] == 8)
    for k in NAMES:
        assert np.all(np.isfinite(got[k])), k
    assert np.array_equal(got["price"][:, 0], got["european"][:, 0])
    assert np.all(got["price"][:, 0] == 0.0)
    assert not np.any(np.isnan(got["coef"][:, 1, :7])) and np.all(np.isnan(got["coef"][:, 1, 7]))
    # deep in the money the put is exercised at once: K - S at date 1 beats every later value
    assert np.all(got["price"][:, 1] >= got["european"][:, 1])
    assert np.all(got["price"][:, 1] > 880.0) and np.all(got["price"][:, 1] < 1000.0)


def test_reproducibility_and_independence(ctx):
    import torch
    n = 1000
    three = np.stack([R.README_PARAMS, R.STRESSED_PARAMS, R.CAP_JUMP_PARAMS])
    a = _lsm(ctx, three, L.DEV_OPTIONS, n)
    assert _same_bits(a, _lsm(ctx, three, L.DEV_OPTIONS, n))
    for p in range(3):                                   # set p of P = 3 alone
        one = _lsm(ctx, three[p], L.DEV_OPTIONS, n)
        assert all(np.array_equal(one[k][0], a[k][p], equal_nan=True) for k in a), p
    for j in range(4):                                   # option j of 4 alone
        one = _lsm(ctx, three, L.DEV_OPTIONS[j:j + 1], n)
        dj = L.option_columns(L.DEV_OPTIONS)[2][j]
        for k in NAMES + ("exercise_date",):
            assert np.array_equal(one[k][:, 0], a[k][:, j]), (j, k)
        assert np.array_equal(one["coef"][:, 0], a["coef"][:, j, :dj], equal_nan=True)
    # the device-pointer form on a stream of the caller's
    from dhcos.american import _options
    opts, dates = _options(L.DEV_OPTIONS, SPY, EVERY)
    dev = torch.device("cuda", ctx.device)
    rec = torch.tensor(_records(three), dtype=torch.float64, device=dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    out = ctx.lsm_price_dev(rec, opts, dates, n, SPY, EVERY, SEED, policy=True, stream=st)
    st.synchronize()
    for k, t in zip(a, out):
        assert np.array_equal(t.cpu().numpy(), a[k], equal_nan=True), k
    with pytest.raises(ValueError):
        ctx.lsm_price_dev(rec, opts, dates, n, SPY, EVERY, SEED,
                          stream=torch.cuda.default_stream(dev))


def test_public_api(ctx):
    import dhcos
    res = dhcos.american_monte_carlo(SETS, SPOT, RATE, L.DEV_OPTIONS, n_paths=1000,
                                     steps_per_year=SPY, exercise_every=EVERY, seed=SEED,
                                     policy=True)
    raw = _lsm(ctx, SETS, L.DEV_OPTIONS, 1000)
    assert np.array_equal(res.price, raw["price"]) and res.price.shape == (2, 4)
    assert np.array_equal(res.coefficients, raw["coef"], equal_nan=True)
    assert np.array_equal(res.exercise_date, raw["exercise_date"])
    assert np.array_equal(res.premium, res.price - res.european)
    lo, hi = res.confidence()
    assert np.all(lo < res.price) and np.all(res.price < hi)
    assert (res.n_paths, res.steps_per_year, res.exercise_every, res.seed) == (1000, SPY, EVERY,
                                                                               SEED)
    one = dhcos.american_monte_carlo(SETS[0], SPOT, RATE, L.DEV_OPTIONS, n_paths=1000,
                                     steps_per_year=SPY, exercise_every=EVERY, seed=SEED)
    assert np.array_equal(one.price, res.price[0]) and one.coefficients is None
    dh = dhcos.DoubleHeston(SPOT, 105.0, 0.5, RATE, *SETS[0], option_type="put")
    price, err = dh.american_monte_carlo(n_paths=1000, steps_per_year=SPY, exercise_every=EVERY,
                                         seed=SEED)
    assert (price, err) == (res.price[0, 1], res.stderr[0, 1])


def test_black_scholes_limit_against_the_tree(ctx):
    """The inputs of the CPU test of the restatement, on the device: puts at K / S0 = 0.9, 1.0,
    1.1 against the binomial Bermudan values, |LSM - tree| <= |recorded mean bias| + 4 stderr."""
    with open(os.path.join(GOLDEN, L.BIAS_FILE)) as fh:
        bias = json.load(fh)
    options = [{"strike": k, "maturity": L.BS_T, "option_type": "put"} for k in L.BS_STRIKES]
    got = _lsm(ctx, L.BS_PARAMS, options, L.BS_PATHS, spy=L.BS_SPY, every=1, seed=L.BS_TEST_SEED,
               spot=L.BS_SPOT, rate=L.BS_RATE)
    assert not np.any(np.isnan(got["coef"][0, :, :L.BS_DATES - 1]))
    for j, k in enumerate(L.BS_STRIKES):
        tree, euro = bias["tree"][j], bias["tree_european"][j]
        allow = abs(bias["mean_bias"][j]) + 4.0 * got["stderr"][0, j]
        diff = got["price"][0, j] - tree
        print(f"K {k}: device LSM {got['price'][0, j]:.4f} +- {got['stderr'][0, j]:.4f}, tree "
              f"{tree:.4f}, LSM - tree {diff:+.4f}, allowance {allow:.4f}")
        assert tree - euro > allow
        assert abs(diff) <= allow, (k, diff, allow)


def test_native_refusals(ctx):
    """DH_E_ARG with a message naming the argument for each new case; the storage cap by
    arithmetic on a huge n_paths (nothing is allocated)."""
    from dhcos import _native
    lib = _native.load()
    rec = _records(SETS[0])
    out = np.full(4, -7.0)

    def call(options, n_paths=1024, every=EVERY):
        arr = (_native.LsmOption * max(len(options), 1))(*options)
        rc = lib.dh_lsm_price(ctx.handle, rec.ctypes.data, 1, arr, len(options), n_paths, SPY,
                              every, SEED, *(out[k:].ctypes.data for k in range(4)), None, None)
        return rc, lib.dh_last_error().decode()

    ok = _native.LsmOption(0, 0, 100.0, 0.5)
    for args, word in [(dict(options=[ok], every=0), "exercise_every"),
                       (dict(options=[ok], every=-3), "exercise_every"),
                       (dict(options=[ok], every=5), "multiple of exercise_every"),
                       (dict(options=[ok, _native.LsmOption(0, 0, 100.0, 0.4375)]), "option 1"),
                       (dict(options=[]), "n_options"),
                       (dict(options=[ok] * 17), "n_options"),
                       (dict(options=[ok], n_paths=1 << 40),
                        "fewer paths or parameter sets per call"),
                       (dict(options=[ok], n_paths=1), "n_paths"),
                       (dict(options=[_native.LsmOption(0, 0, -1.0, 0.5)]), "strike"),
                       (dict(options=[_native.LsmOption(0, 0, 100.0, 0.51)]), "maturity")]:
        rc, msg = call(**args)
        assert rc == -1 and word in msg, (args, rc, msg)
    rc, msg = call([ok], n_paths=1 << 40)
    assert f"{_native.LSM_MAX_GIB} GiB" in msg
    assert np.all(out == -7.0)                           # no refusal wrote anything
    rc, msg = call([ok])
    assert rc == 0 and np.all(np.isfinite(out)) and np.all(out > 0.0)
