"""GPU tests of the path pricer's variance reduction (csrc/dh_mc_vr.h): the
mirror paths against the NumPy restatement (tests/mc_vr_reference.py), the estimator against its
evaluation in rationals on the library's own paths, the bitwise ties to dh_mc_price, the exact
identities of a control that is the payoff, the control means against the samples they centre,
an end-to-end comparison with the plain pricer on independent samples, reproducibility, and the
refusals of the C-ABI."""
import math

import numpy as np
import pytest

import mc_reference as R
import mc_vr_reference as V

pytestmark = pytest.mark.gpu

SPOT, RATE = 100.0, 0.03
U = 2.0 ** -53
SPY, OBS, SEED = 8, (2, 4, 8), 1
SETS = np.stack([R.README_PARAMS, R.STRESSED_PARAMS])
A, C = V.ANTITHETIC, V.CONTROL
N_BIG = 1024 * 256 + 7                     # 1,025 chunks, the last ragged: slot 0 walks two
FIELDS = ("price", "stderr", "base_price", "base_stderr", "beta")

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
# the reduction test's options and seed: every control has Ccc >= 1e-3 sum c^2 at every sample count
# and flag combination of the test (asserted there on the library's paths).  Found with the
# restatement on the CPU: the pair average of S_T varies little (that is the antithetic at work),
# so the two S controls sit at the longest maturity, and of seeds 1..39 this one has the largest
# worst ratio over n = 2, 65, 257 (3.8e-3; the first two pairs of most seeds are too alike).
RSEED = 29
REDUCE = [
    {"strike": 80.0, "maturity": 1.0, "option_type": "call"},
    {"strike": 120.0, "maturity": 1.0, "option_type": "put"},
    {"strike": 80.0, "maturity": 0.5, "option_type": "call", "kind": "asian"},
    {"strike": 80.0, "maturity": 1.0, "option_type": "call", "kind": "up_and_out",
     "barrier": 130.0},
    {"strike": 120.0, "maturity": 0.25, "option_type": "put", "kind": "down_and_out",
     "barrier": 85.0},
    {"strike": 0.0, "maturity": 1.0, "option_type": "call", "kind": "asian"},
]


def _records(sets=SETS, q=0.0):
    from dhcos import _native
    rec = np.zeros((len(sets), _native.PARAM_STRIDE))
    rec[:, :13] = sets
    rec[:, 13], rec[:, 14], rec[:, 15] = SPOT, RATE, q
    return rec


def _option_array(options, spy=SPY):
    from dhcos.montecarlo import _options
    return _options(options, spy)


def _steps(options, spy=SPY):
    return [int(round(o["maturity"] * spy)) for o in options]


@pytest.fixture(scope="module")
def ctx():
    from dhcos import _native
    return _native.default_context()


def _vr(ctx, rec, options, n_paths, flags, seed=SEED, spy=SPY):
    return dict(zip(FIELDS + ("control_mean",),
                    ctx.mc_price_vr(rec, _option_array(options, spy), n_paths, spy, seed, flags)))


# ---- the mirror paths -------------------------------------------------------------------------------
def _parity_ratio(got, want):
    bar = 1e-10 * np.abs(want)
    bar[..., 1:3] += 1e-14
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(got == want, 0.0, np.abs(got - want) / bar)
    return float(np.max(ratio))


def test_mirror_paths_match_the_restatement(ctx):
    """simulate_paths(mirror=True) against the restatement's mirrored walk, both sets, paths
    0..319 and 1000..1063 at steps 2, 4 and 8 of 8 per year, to the path bar of the plain pricer
    (1e-10 relative, +1e-14 on the variances); the mirrors reach every branch of the step."""
    from dhcos.montecarlo import simulate_paths
    stats = R.new_stats()
    worst = []
    for p0, n in ((0, 320), (1000, 64)):
        want = np.stack([V.simulate(p, SPOT, RATE, np.arange(p0, p0 + n), OBS[-1], SPY, SEED, OBS,
                                    mirror=True, stats=stats if p0 == 0 else None)[1]
                         for p in SETS])
        got = simulate_paths(SETS, SPOT, RATE, OBS, n_paths=n, path0=p0, steps_per_year=SPY,
                             seed=SEED, mirror=True)
        assert got.shape == want.shape and np.all(np.isfinite(got))
        worst.append(_parity_ratio(got, want))
        plain = simulate_paths(SETS, SPOT, RATE, OBS, n_paths=n, path0=p0, steps_per_year=SPY,
                               seed=SEED)
        assert np.array_equal(plain, ctx.mc_paths(_records(), OBS, p0, n, SPY, SEED))
        assert np.array_equal(plain, ctx.mc_paths_vr(_records(), OBS, p0, n, SPY, SEED, False))
        assert not np.array_equal(plain, got)
    assert stats["quad"] > 0 and stats["expo"] > 0 and stats["zero"] > 0, stats
    assert stats["n1"] > 0 and stats["n2"] > 0, stats
    assert stats["psi_gap"] > 1e-9 and stats["u_gap"] > 1e-9, stats
    print(f"mc mirror path parity: worst |device - restatement| / bar = {worst}; mirror branch "
          f"counts {stats}")
    assert max(worst) <= 1.0


# ---- the estimator against rationals on the library's own paths -------------------------------------
@pytest.fixture(scope="module")
def big_paths(ctx):
    """Paths 0 .. N_BIG - 1 of the README set and their mirrors at steps 2, 4, 8: [2, N_BIG, 3, 6]
    (0 the paths, 1 the mirrors).  Computed once; read-only."""
    rec = _records(SETS[:1])
    out = np.stack([ctx.mc_paths_vr(rec, OBS, 0, N_BIG, SPY, RSEED, m)[0] for m in (False, True)])
    out.setflags(write=False)
    return out


def _cov_bar(n, sab, abs_ab, sa, sb, abs_a, abs_b, cab):
    """|d Cab| for Cab = Sab - Sa Sb / n summed in any order: n u sum|a b| on Sab (the products'
    roundings included), (n - 1) u sum|a| on Sa and the same on Sb carried through Sa Sb / n, two
    roundings of that term and one of the subtraction."""
    return (n * U * abs_ab + (n - 1) * U * (abs(sa) * abs_b + abs(sb) * abs_a) / n
            + 2 * U * abs(sa * sb) / n + U * abs(cab))


def _root_bar(v, dv):
    return min(dv / (2 * math.sqrt(v)), math.sqrt(dv)) if v > 0 else math.sqrt(dv)


def _vr_bars(y, c, disc, mean, ctrl):
    """The estimator in rationals on the samples y and controls c -> (want, bar), dicts over
    FIELDS.  The bars carry the summation bounds of the five sums (_reduction_bars of
    tests/test_gpu_mc.py: |d sum a| <= (n - 1) u sum|a|, |d sum a b| <= n u sum|a b|) to first
    order through the formulas of 3.15.2, plus a few u of each result for the roundings of its
    own few operations (the discount's exp included, as there):
        d beta = d Cyc / Ccc + |Cyc| d Ccc / Ccc^2,
        d price = d base_price + |D| d beta + |beta| d D,    D = disc Sc / n - m,
        d (Cyy - beta Cyc) = d Cyy + |Cyc| d beta + |beta| d Cyc,
    and |sqrt(V + d) - sqrt(V)| <= min(|d| / (2 sqrt V), sqrt |d|)."""
    n = y.size
    sums = V.five_sums(y, c)
    want = V.estimator(sums, n, disc, mean, ctrl, exact=True)
    sy, syy, sc, scc, syc = sums
    ay, ac, ayc = math.fsum(np.abs(y)), math.fsum(np.abs(c)), math.fsum(np.abs(y * c))
    cyy = syy - sy * sy / n
    d_cyy = _cov_bar(n, syy, syy, sy, sy, ay, ay, cyy)
    scale = disc / math.sqrt(n * (n - 1.0))
    bar = {"base_price": disc * (n - 1) * U * ay / n + 4 * U * abs(want["base_price"]),
           "base_stderr": scale * _root_bar(cyy, d_cyy) + 4 * U * want["base_stderr"],
           "beta": 0.0}
    bar["price"], bar["stderr"] = bar["base_price"], bar["base_stderr"]
    if ctrl:
        ccc, cyc = scc - sc * sc / n, syc - sy * sc / n
        d_ccc = _cov_bar(n, scc, scc, sc, sc, ac, ac, ccc)
        d_cyc = _cov_bar(n, syc, ayc, sy, sc, ay, ac, cyc)
        beta = cyc / ccc
        d_beta = d_cyc / ccc + abs(cyc) * d_ccc / (ccc * ccc) + 2 * U * abs(beta)
        D = disc * sc / n - mean
        d_D = disc * (n - 1) * U * ac / n + 4 * U * abs(disc * sc / n) + U * abs(D)
        bar["beta"] = d_beta
        bar["price"] = (bar["base_price"] + abs(D) * d_beta + abs(beta) * d_D
                        + 2 * U * abs(beta * D) + 2 * U * abs(want["price"]))
        resid = cyy - beta * cyc
        d_resid = (d_cyy + abs(cyc) * d_beta + abs(beta) * d_cyc + 2 * U * abs(beta * cyc)
                   + U * abs(resid))
        bar["stderr"] = scale * _root_bar(max(resid, 0.0), d_resid) + 4 * U * want["stderr"]
    return want, bar


@pytest.mark.parametrize("n", [2, 65, 257, N_BIG])
@pytest.mark.parametrize("flags", [A, C, A | C])
def test_the_estimator_is_the_reduction_of_the_librarys_own_paths(ctx, big_paths, flags, n):
    """price, stderr, base_price, base_stderr and beta of n samples (n pairs = 2 n walks under the
    antithetic flag) against the estimator in rationals on samples formed in NumPy from
    dh_mc_paths_vr's paths and mirrors, to the bars of _vr_bars.  n = 2: two lanes; 65: a wave and
    a lane; 257: a chunk and a lane; 1024 * 256 + 7: 1,025 chunks, so slot 0 walks two."""
    anti, ctrl = bool(flags & A), bool(flags & C)
    rec = _records(SETS[:1])
    got = _vr(ctx, rec, REDUCE, 2 * n if anti else n, flags, seed=RSEED)
    worst = {k: 0.0 for k in FIELDS}
    for j, (o, st) in enumerate(zip(REDUCE, _steps(REDUCE))):
        k = OBS.index(st)
        y, c = V.sample_and_control(o, st, big_paths[0][:n, k], big_paths[1][:n, k] if anti else None)
        mean = got["control_mean"][0, j]
        if ctrl:
            ccc = math.fsum(c * c) - math.fsum(c) ** 2 / n
            assert ccc >= 1e-3 * math.fsum(c * c), (j, n, ccc)      # the inputs, not the library
            assert np.isfinite(mean) and (V.has_twin(o) or mean == SPOT)
        else:
            assert np.isnan(mean)
        want, bar = _vr_bars(y, c, math.exp(-RATE * o["maturity"]), float(mean), ctrl)
        for f in FIELDS:
            d = abs(got[f][0, j] - want[f])
            if d > 0.0:
                worst[f] = max(worst[f], d / bar[f] if bar[f] > 0.0 else np.inf)
        if not ctrl:
            assert got["beta"][0, j] == 0.0 and got["price"][0, j] == got["base_price"][0, j]
            assert got["stderr"][0, j] == got["base_stderr"][0, j]
    print(f"mc vr reduction, flags {flags}, n {n}: worst |device - rational| / bar {worst}")
    assert all(v <= 1.0 for v in worst.values()), worst


# ---- ties to the plain pricer, the algebra of the control -------------------------------------------
@pytest.mark.parametrize("n", [2, 65, 257, 775])
def test_the_base_estimate_is_the_plain_pricers_bits(ctx, n):
    """Under the control flag alone the samples are dh_mc_price's: base_price and base_stderr are
    its bits for a table of all four kinds, both sets; and stderr <= base_stderr for every
    option, which holds by construction (beta Cyc = Cyc^2 / Ccc >= 0)."""
    got = _vr(ctx, _records(), MIX, n, C)
    price, err = ctx.mc_price(_records(), _option_array(MIX), n, SPY, SEED)
    assert np.array_equal(got["base_price"], price) and np.array_equal(got["base_stderr"], err)
    assert np.all(got["stderr"] <= got["base_stderr"])
    assert np.all(np.isfinite(got["price"])) and np.all(np.isfinite(got["beta"]))
    both = _vr(ctx, _records(), MIX, 2 * n, A | C)
    assert np.all(both["stderr"] <= both["base_stderr"])
    only = _vr(ctx, _records(), MIX, 2 * n, A)             # the pairs' plain mean is the same
    assert np.array_equal(only["base_price"], both["base_price"])
    assert np.array_equal(only["base_stderr"], both["base_stderr"])


# ---- identities -------------------------------------------------------------------------------------
def _twin_prices(ctx, rec, options):
    """dh_surface_price of the options' European twins at the control means' N and L."""
    from dhcos import _native
    surf = _native.Surface(ctx, [o["strike"] for o in options], [o["maturity"] for o in options],
                           [V.is_call(o) for o in options])
    try:
        return surf.price(rec, N=_native.MC_VR_COS_N, L=_native.MC_VR_COS_L)
    finally:
        surf.close()


@pytest.mark.parametrize("flags", [C, A | C])
def test_a_control_that_is_the_payoff_prices_at_its_mean(ctx, flags):
    """An Asian with a one-step maturity, an up-and-out with barrier 1e9 and a down-and-out with
    barrier 1e-9 are their European twins on every path: beta == 1 and stderr == 0 exactly, the
    price within 4 ulp of control_mean, control_mean the bits of dh_surface_price of the twins
    (N = 256, L = 10, q = 0); a European's control mean is spot; a twin that pays nowhere gives
    beta == 0 and the base price; q in slot 15 of a record changes no bit."""
    same = [{"strike": 100.0, "maturity": 1.0 / SPY, "option_type": "call", "kind": "asian"},
            {"strike": 105.0, "maturity": 1.0 / SPY, "option_type": "put", "kind": "asian"},
            {"strike": 95.0, "maturity": 0.5, "option_type": "call", "kind": "up_and_out",
             "barrier": 1e9},
            {"strike": 100.0, "maturity": 1.0, "option_type": "put", "kind": "down_and_out",
             "barrier": 1e-9}]
    dead = [{"strike": 1e6, "maturity": 0.5, "option_type": "call", "kind": "asian"}]
    eu = [{"strike": 100.0, "maturity": 0.5, "option_type": "put"},
          {"strike": 0.0, "maturity": 1.0, "option_type": "call", "kind": "asian"}]
    opts = same + dead + eu
    got = _vr(ctx, _records(), opts, 320, flags)
    ns = len(same)
    assert np.all(got["beta"][:, :ns] == 1.0) and np.all(got["stderr"][:, :ns] == 0.0)
    assert np.all(got["base_stderr"][:, :ns] > 0.0)
    m = got["control_mean"]
    tol = 4 * 2.0 ** -52 * np.maximum(np.abs(got["base_price"][:, :ns]), np.abs(m[:, :ns]))
    assert np.all(np.abs(got["price"][:, :ns] - m[:, :ns]) <= tol)
    assert np.array_equal(m[:, :ns + 1], _twin_prices(ctx, _records(), opts[:ns + 1]))
    assert np.all(m[:, ns + 1:] == SPOT)
    assert np.all(got["beta"][:, ns] == 0.0)
    assert np.array_equal(got["price"][:, ns], got["base_price"][:, ns])
    assert np.all(got["base_price"][:, ns] == 0.0)
    with_q = _vr(ctx, _records(q=0.02), opts, 320, flags)
    for k in got:
        assert np.array_equal(got[k], with_q[k]), k


# ---- the control means centre their samples ---------------------------------------------------------
def test_control_means_are_right():
    """README set, the generator's grid as calls and as puts, 2^17 paths at 32 steps per year,
    seed 2024, control only: |price - base_price| <= 4 sqrt(base_stderr^2 - stderr^2), i.e. the
    control's sample mean within 4 of its standard errors of the mean the library holds for it."""
    import dhcos
    grid = [{"strike": float(k), "maturity": float(t), "option_type": ot}
            for ot in ("call", "put") for k, t in zip(R.GRID_K, R.GRID_T)]
    res = dhcos.monte_carlo(R.README_PARAMS, SPOT, RATE, grid, n_paths=1 << 17, steps_per_year=32,
                            seed=2024, control_variate=True)
    assert isinstance(res, dhcos.VarianceReducedResult) and res.price.shape == (30,)
    assert np.all(res.control_mean == SPOT) and res.control_variate and not res.antithetic
    z = np.abs(res.price - res.base_price) / np.sqrt(res.base_stderr ** 2 - res.stderr ** 2)
    print(f"mc vr control means: max |price - base| / sqrt(base_stderr^2 - stderr^2) {z.max():.2f}; "
          f"variance ratios {res.variance_ratio.min():.2f} .. {res.variance_ratio.max():.2f}")
    assert np.all(z <= 4.0), z
    assert np.all(res.variance_ratio >= 1.0)


# ---- end to end, independent samples ----------------------------------------------------------------
def test_reduced_prices_agree_with_the_plain_pricer_on_other_paths():
    """Asian, up-and-out (H = 125) and down-and-out (H = 85) calls and puts at K = 90, 100, 110,
    T = 0.5: both flags at 2^16 walks, seed 1, against the plain pricer at 2^19 paths, seed 2:
    |difference| <= 4 sqrt(stderr_vr^2 + stderr_plain^2).  The restatement on the CPU at 2^13
    walks against 2^15 plain paths (same seeds, COS means from the oracle at N = 256) gave a worst
    ratio of 1.68 against the bar's 4."""
    import dhcos
    table = [dict({"strike": k, "maturity": 0.5, "option_type": ot, "kind": kind},
                  **({"barrier": h} if h else {}))
             for kind, h in (("asian", None), ("up_and_out", 125.0), ("down_and_out", 85.0))
             for ot in ("call", "put") for k in (90.0, 100.0, 110.0)]
    vr = dhcos.monte_carlo(R.README_PARAMS, SPOT, RATE, table, n_paths=1 << 16, steps_per_year=64,
                           seed=1, antithetic=True, control_variate=True)
    plain = dhcos.monte_carlo(R.README_PARAMS, SPOT, RATE, table, n_paths=1 << 19,
                              steps_per_year=64, seed=2)
    z = np.abs(vr.price - plain.price) / np.sqrt(vr.stderr ** 2 + plain.stderr ** 2)
    print(f"mc vr end to end: max |vr - plain| / combined stderr {z.max():.2f}; variance ratios "
          f"{np.array2string(vr.variance_ratio, precision=2)}")
    assert np.all(z <= 4.0), z
    assert type(plain) is dhcos.MonteCarloResult
    # the instance method passes the keywords on
    dh = dhcos.DoubleHeston(SPOT, 105.0, 0.5, RATE, *R.README_PARAMS, option_type="call")
    p, e = dh.monte_carlo(n_paths=1 << 12, steps_per_year=SPY, seed=3, antithetic=True,
                          control_variate=True)
    one = dhcos.monte_carlo(R.README_PARAMS, SPOT, RATE,
                            [{"strike": 105.0, "maturity": 0.5, "option_type": "call"}],
                            n_paths=1 << 12, steps_per_year=SPY, seed=3, antithetic=True,
                            control_variate=True)
    assert p == one.price[0] and e == one.stderr[0]


# ---- reproducibility --------------------------------------------------------------------------------
def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def test_results_are_reproducible_bitwise(ctx):
    import torch
    from dhcos import _native
    three = np.stack([R.README_PARAMS, R.STRESSED_PARAMS, 0.5 * (R.README_PARAMS
                                                                 + R.STRESSED_PARAMS)])
    rec = _records(three)
    n = 2 * (3 * 256 + 7)                  # pairs: three chunks and a ragged fourth
    lists = (_option_array(MIX), _option_array(REDUCE[2:5]))
    calls = [(lists[i % 2], (A | C, C, A, A | C)[i], R.TRUTH_SEED + i) for i in range(4)]
    alone = []
    for opts, flags, seed in calls:
        a = ctx.mc_price_vr(rec, opts, n, SPY, seed, flags)
        assert _same(a, ctx.mc_price_vr(rec, opts, n, SPY, seed, flags))
        for p in range(3):                 # a set alone is the set in the batch
            one = ctx.mc_price_vr(rec[p:p + 1], opts, n, SPY, seed, flags)
            assert _same([x[0] for x in one], [x[p] for x in a]), (flags, p)
        alone.append(a)
    d_rec = torch.from_numpy(rec).to(f"cuda:{ctx.device}")
    fresh = _native.Context(ctx.device)
    try:                                   # four calls queued with no synchronisation between
        outs = [fresh.mc_price_vr_dev(d_rec, opts, n, SPY, seed, flags)
                for opts, flags, seed in calls]
        fresh.synchronize()
        outs = [[t.cpu().numpy() for t in o] for o in outs]
    finally:
        fresh.close()
    for a, o, (opts, flags, _) in zip(alone, outs, calls):
        assert _same(a, o), (len(opts), flags)
    assert not _same(alone[0][:2], ctx.mc_price_vr(rec, lists[0], n, SPY, R.TRUTH_SEED + 9,
                                                   A | C)[:2])


# ---- refusals ---------------------------------------------------------------------------------------
REFUSALS = {                               # case -> (call arguments, the name in the message)
    "no flags": (dict(flags=0), "flags"),
    "unknown flag": (dict(flags=4), "flags"),
    "unknown flag beside a known one": (dict(flags=A | 8), "flags"),
    "negative flags": (dict(flags=-1), "flags"),
    "odd pairs": (dict(flags=A, n_paths=513), "n_paths"),
    "one pair": (dict(flags=A | C, n_paths=2), "n_paths"),
    "one path": (dict(flags=C, n_paths=1), "n_paths"),
    "steps_per_year": (dict(flags=C, spy=0), "steps_per_year"),
    "nan": (dict(flags=C, nan=True), "mu_j"),
    "kind": (dict(flags=A, opt=(4, 1, 100.0, 0.5, 0.0)), "kind"),
    "barrier": (dict(flags=C, opt=(2, 1, 100.0, 0.5, 0.0)), "barrier"),
    "n_options": (dict(flags=C, n_opt=0), "n_options"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_the_abi_refuses_bad_arguments_before_any_launch(ctx, case):
    from dhcos import _native
    kw, name = REFUSALS[case]
    rec = _records(SETS[:1])
    if kw.get("nan"):
        rec[0, 11] = np.nan
    opts = (_native.McOption * 1)(_native.McOption(*kw.get("opt", (1, 1, 100.0, 0.5, 0.0))))
    outs = [np.full(1, -7.0) for _ in range(6)]
    lib = _native.load()
    rc = lib.dh_mc_price_vr(ctx.handle, rec.ctypes.data, 1, opts, kw.get("n_opt", 1),
                            kw.get("n_paths", 512), kw.get("spy", SPY), 0, kw["flags"],
                            *(o.ctypes.data for o in outs))
    assert rc == -1                                        # DH_E_ARG
    assert name in lib.dh_last_error().decode()
    assert all(np.all(o == -7.0) for o in outs)


def test_the_optional_outputs_may_be_null(ctx):
    from dhcos import _native
    rec = _records(SETS[:1])
    opts = _option_array(MIX)
    price, err = np.empty(len(MIX)), np.empty(len(MIX))
    rc = _native.load().dh_mc_price_vr(ctx.handle, rec.ctypes.data, 1, opts, len(MIX), 512, SPY,
                                       SEED, A | C, price.ctypes.data, err.ctypes.data, None, None,
                                       None, None)
    assert rc == 0
    full = _vr(ctx, rec, MIX, 512, A | C)
    assert np.array_equal(price, full["price"][0]) and np.array_equal(err, full["stderr"][0])
