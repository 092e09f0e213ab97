"""GPU tests of the Monte Carlo path pricer (csrc/dh_mc.h): the library's paths
against the NumPy restatement (tests/mc_reference.py), its prices against the reduction of its own
paths, bitwise identities and reproducibility, the model check against the COS pricer, and the
refusals of the C-ABI."""
import ctypes as C
import math

import numpy as np
import pytest

import mc_reference as R

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


def test_prices_are_the_reduction_of_the_librarys_own_paths(ctx, device_paths):
    """price and stderr against math.fsum over payoffs formed in NumPy from dh_mc_paths' output.
    With A = sum |payoff|, s2 = sum payoff^2, V = s2 - s1^2 / n and u = 2^-53, any order of
    summation keeps |d s1| <= (n - 1) u A, so the price bar is e^{-rT} (n - 1) u A / n.  For the
    standard error e^{-rT} sqrt(V / (n (n - 1))): |d s2| <= n u s2 (the squares' roundings
    included), |d (s1^2 / n)| <= 2 n u A^2 / n, the subtraction adds u V, so |dV| <= dV := n u s2 +
    2 u A^2 + u V, and |sqrt(V + d) - sqrt(V)| <= min(|d| / (2 sqrt V), sqrt |d|); four more
    roundings (division, square root, discount) add 4 u of the result."""
    price, err = ctx.mc_price(_records(), _option_array(MIX), N_SMALL, SPY, SEED)
    n = N_SMALL
    for p in range(len(SETS)):
        for j, (o, st) in enumerate(zip(MIX, _steps(MIX))):
            pay = R.payoff(o.get("kind", "european"), o["option_type"] == "call", o["strike"],
                           o.get("barrier", 0.0), st, device_paths[p][:, OBS.index(st)])
            disc = math.exp(-RATE * o["maturity"])
            s1, A, s2 = math.fsum(pay), math.fsum(np.abs(pay)), math.fsum(pay * pay)
            V = math.fsum((pay - s1 / n) ** 2)
            want_p = disc * s1 / n
            want_e = disc * math.sqrt(V / (n * (n - 1)))
            bar_p = disc * (n - 1) * U * A / n + 4 * U * abs(want_p)
            dV = n * U * s2 + 2 * U * A * A + U * V
            dsq = min(dV / (2 * math.sqrt(V)), math.sqrt(dV)) if V > 0 else math.sqrt(dV)
            bar_e = disc * dsq / math.sqrt(n * (n - 1)) + 4 * U * want_e
            assert abs(price[p, j] - want_p) <= bar_p, (p, j, price[p, j], want_p, bar_p)
            assert abs(err[p, j] - want_e) <= bar_e, (p, j, err[p, j], want_e, bar_e)
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
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_the_abi_refuses_bad_arguments_before_any_launch(ctx, case):
    from dhcos import _native
    kw, name = REFUSALS[case]
    rec = kw.get("rec", _records(SETS[:1]))
    opts = (_native.McOption * 1)(_native.McOption(*kw.get("opt", (0, 1, 100.0, 0.5, 0.0))))
    price, err = np.full(1, -7.0), np.full(1, -7.0)
    lib = _native.load()
    rc = lib.dh_mc_price(ctx.handle, rec.ctypes.data, 1, opts, kw.get("n_opt", 1),
                         kw.get("n_paths", 512), kw.get("spy", SPY), 0, price.ctypes.data,
                         err.ctypes.data)
    assert rc == -1                                        # DH_E_ARG
    assert name in lib.dh_last_error().decode()
    assert price[0] == -7.0 and err[0] == -7.0
    if "rec" in kw:                                        # the validation export checks the same
        out = np.full(6, -7.0)
        obs = np.array([1], dtype=np.int32)
        rc = lib.dh_mc_paths(ctx.handle, rec.ctypes.data, 1, 1, obs.ctypes.data, 0, 1, SPY, 0,
                             out.ctypes.data)
        assert rc == -1 and name in lib.dh_last_error().decode() and np.all(out == -7.0)
