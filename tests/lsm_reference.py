"""NumPy restatement of the least-squares Monte Carlo backward pass of DESIGN.md 3.15.1, and a
Cox-Ross-Rubinstein binomial Bermudan pricer as the Black-Scholes-limit truth (test infrastructure
only).

Written from the document, not from the kernel: the same basis, the same rules with their strict
inequalities, the same skip rule.  The normal equations are solved by ``numpy.linalg.solve`` (or,
to show that a seed's exercise decisions do not hang on the solver, by ``numpy.linalg.lstsq`` on
the design matrix).  Nothing in dhcos/ imports this module.
"""
import numpy as np

BASIS = 10
MIN_ITM = 64


def basis(S, v1, v2, strike, theta1, theta2):
    """[n, 10]: 1, x, y1, y2, x^2, y1^2, y2^2, x y1, x y2, y1 y2 with x = S / K - 1,
    y_i = v_i / theta_i - 1."""
    x, y1, y2 = S / strike - 1.0, v1 / theta1 - 1.0, v2 / theta2 - 1.0
    return np.stack([np.ones_like(x), x, y1, y2, x * x, y1 * y1, y2 * y2, x * y1, x * y2, y1 * y2],
                    axis=1)


def intrinsic(S, strike, is_call):
    return np.maximum(S - strike, 0.0) if is_call else np.maximum(strike - S, 0.0)


def _positive_definite(G):
    """True where Cholesky without pivoting meets only pivots > 0."""
    if not np.all(np.isfinite(G)):
        return False
    try:
        np.linalg.cholesky(G)
    except np.linalg.LinAlgError:
        return False
    return True


def backward_one(states, strike, is_call, dates, r, delta, theta1, theta2, solver="solve"):
    """One option over states [n_paths, D, 3] (S, v1, v2 at dates 1 .. D), exercisable at dates
    1 .. dates (<= D), the last its maturity -> dict of price, stderr, european, european_stderr,
    coef [D, 10] (row d - 1: the coefficients used at date d; NaN where skipped, at the maturity
    date and past it), exercise_date [n_paths], gram [D, 10, 10] (the Gram matrix of each fitted
    date, NaN elsewhere) and margin (the smallest |h - fitted value| over the in-the-money paths
    of the fitted dates)."""
    n, D = states.shape[0], states.shape[1]
    disc = np.exp(-r * delta)
    h_T = intrinsic(states[:, dates - 1, 0], strike, is_call)
    cash = h_T.copy()
    tau = np.full(n, dates, dtype=np.int32)
    coef = np.full((D, BASIS), np.nan)
    gram = np.full((D, BASIS, BASIS), np.nan)
    margin = np.inf
    for d in range(dates - 1, 0, -1):
        S, v1, v2 = (states[:, d - 1, k] for k in range(3))
        h = intrinsic(S, strike, is_call)
        itm = h > 0.0
        Y = disc * cash
        cash = Y
        if int(itm.sum()) < MIN_ITM:
            continue
        phi = basis(S[itm], v1[itm], v2[itm], strike, theta1, theta2)
        G = phi.T @ phi
        if not _positive_definite(G):
            continue
        if solver == "solve":
            beta = np.linalg.solve(G, phi.T @ Y[itm])
        else:
            beta = np.linalg.lstsq(phi, Y[itm], rcond=None)[0]
        coef[d - 1], gram[d - 1] = beta, G
        cont = phi @ beta
        margin = min(margin, float(np.min(np.abs(h[itm] - cont))))
        ex = np.flatnonzero(itm)[h[itm] > cont]
        cash = Y.copy()
        cash[ex] = h[ex]
        tau[ex] = d
    nn = float(n)

    def finish(x, df):
        s1, s2 = x.sum(), (x * x).sum()
        return df * s1 / nn, df * np.sqrt(max(s2 - s1 * s1 / nn, 0.0) / (nn * (nn - 1.0)))

    price, err = finish(cash, disc)
    euro, euro_err = finish(h_T, np.exp(-r * (dates * delta)))
    return {"price": price, "stderr": err, "european": euro, "european_stderr": euro_err,
            "coef": coef, "exercise_date": tau, "gram": gram, "margin": margin}


def backward(states, strikes, is_call, dates, r, delta, theta1, theta2, solver="solve"):
    """backward_one for every option (strikes, is_call, dates: one entry each) -> a dict of the
    same names, each stacked over the options."""
    outs = [backward_one(states, float(k), bool(c), int(dj), r, delta, theta1, theta2, solver)
            for k, c, dj in zip(strikes, is_call, dates)]
    return {k: np.stack([np.asarray(o[k]) for o in outs]) for k in outs[0]}


def crr_bermudan(spot, strike, r, sigma, T, n_dates, steps_per_date, is_call=False):
    """Cox-Ross-Rubinstein tree of n_dates * steps_per_date steps; exercise only at the steps
    steps_per_date, 2 steps_per_date, ..., the last the maturity (time 0 is not a date)
    -> (Bermudan value, European value of the same tree)."""
    N = n_dates * steps_per_date
    dt = T / N
    u = np.exp(sigma * np.sqrt(dt))
    p = (np.exp(r * dt) - 1.0 / u) / (u - 1.0 / u)
    df = np.exp(-r * dt)

    def level(k):
        return spot * u ** (2.0 * np.arange(k + 1) - k)

    berm = intrinsic(level(N), strike, is_call)
    euro = berm.copy()
    for k in range(N - 1, -1, -1):
        berm = df * (p * berm[1:] + (1.0 - p) * berm[:-1])
        euro = df * (p * euro[1:] + (1.0 - p) * euro[:-1])
        if k > 0 and k % steps_per_date == 0:
            berm = np.maximum(berm, intrinsic(level(k), strike, is_call))
    return float(berm[0]), float(euro[0])


# ---- the Black-Scholes limit of the model: the configuration of tests/golden/lsm_bias.json ------
# v0 = theta in both factors, sigma1 = sigma2 = 1e-3, no jumps, total variance 0.04
BS_PARAMS = np.array([0.02, 1.0, 0.02, 1e-3, 0.0, 0.02, 1.0, 0.02, 1e-3, 0.0, 0.0, 0.0, 0.0])
BS_SPOT, BS_RATE, BS_SIGMA, BS_T = 100.0, 0.05, 0.2, 1.0
BS_DATES, BS_SPY, BS_PATHS = 8, 8, 1 << 15
BS_STRIKES = (90.0, 100.0, 110.0)
BS_FIT_SEEDS = tuple(range(1, 9))        # the seeds the recorded bias is the mean over
BS_TEST_SEED = 9
BS_TREE_STEPS = 500                      # tree steps per exercise interval
BIAS_FILE = "lsm_bias.json"


def bs_restatement(seed):
    """The restatement's puts at BS_STRIKES on mc_reference's paths of `seed` -> backward()'s
    dict."""
    import mc_reference as R
    _, obs = R.simulate(BS_PARAMS, BS_SPOT, BS_RATE, np.arange(BS_PATHS), BS_SPY, BS_SPY, seed,
                        tuple(range(1, BS_DATES + 1)))
    return backward(obs[:, :, :3], BS_STRIKES, [False] * 3, [BS_DATES] * 3, BS_RATE,
                    1.0 / BS_SPY, BS_PARAMS[2], BS_PARAMS[7])


def bs_tree():
    """[(Bermudan, European)] of the tree at BS_STRIKES."""
    return [crr_bermudan(BS_SPOT, k, BS_RATE, BS_SIGMA, BS_T, BS_DATES, BS_TREE_STEPS)
            for k in BS_STRIKES]


# ---- the configurations the device is compared on (tests/test_gpu_lsm.py) ------------------------
DEV_SPOT, DEV_RATE = 100.0, 0.03
DEV_SPY, DEV_EVERY, DEV_SEED = 32, 4, 7          # 8 exercise dates a year
DEV_OPTIONS = [                                  # date counts 8 and 4
    {"strike": 100.0, "maturity": 1.0, "option_type": "put"},
    {"strike": 105.0, "maturity": 0.5, "option_type": "put"},
    {"strike": 95.0, "maturity": 1.0, "option_type": "put"},
    {"strike": 100.0, "maturity": 0.5, "option_type": "call"},
]
DEV_OPTIONS_16 = [{"strike": 85.0 + 2.5 * j, "maturity": (0.25, 0.5, 1.0, 0.125)[j % 4],
                   "option_type": "call" if j % 5 == 4 else "put"} for j in range(16)]


def option_columns(options, spy=DEV_SPY, every=DEV_EVERY):
    """-> (strikes, is_call, date counts) of option dicts."""
    return ([o["strike"] for o in options], [o["option_type"] == "call" for o in options],
            [int(round(o["maturity"] * spy)) // every for o in options])


def restate(states, params, options, rate=DEV_RATE, spy=DEV_SPY, every=DEV_EVERY, solver="solve"):
    """backward() of `options` over the states [n_paths, D, >= 3] of one parameter set."""
    k, c, dj = option_columns(options, spy, every)
    return backward(states[:, :, :3], k, c, dj, rate, every / spy, params[2], params[7], solver)
