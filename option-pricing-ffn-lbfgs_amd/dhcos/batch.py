"""``calibrate_batch``: many markets on one option grid, calibrated together on the device.

The reference's pipeline is generator -> FFN -> L-BFGS refinement of the FFN's guess, sample after
sample (lbfgs_calibrator.py:236-336 once per sample).  Here B markets that share one option grid
-- strikes in percent of each market's spot (the generator's grid), or one listed absolute grid
under moving spots -- run every start of every market through the same launches
(dh_calibrate_lbfgs_batch): each iteration prices the 14 points of every live
start's pending request in one launch, reduces each against its own market's prices and advances
every start's L-BFGS-B state.  A start's trajectory depends on its own x0 and market alone, so a
market's result does not depend on what else is in the batch.

``objective="iv"`` fits implied vols instead of relative prices (dh_calibrate_lbfgs_batch_iv,
DESIGN.md 3.13): the loss of a market is sum_m w_m (iv_model,m - iv_mkt,m)^2 / sum(w) + Feller,
with every model price inverted on the device under its own market's spot and rate.

``gradient="analytic"`` hands the optimiser the exact gradient of the price objective
(dh_calibrate_lbfgs_batch_grad): a request is one point per start -- the parameter
planes of its record and a reduction against its market's prices -- where ``"fd"`` prices fourteen.

``objective="iv"`` with ``gradient="vega"`` is the vol objective's exact gradient
(dh_calibrate_lbfgs_batch_iv_grad): the same parameter planes, each option's price
sensitivities divided by its Black-Scholes vega.  A request inverts M prices where ``"fd"`` inverts
14 M, and no inverter noise is divided by the difference step.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
from scipy.optimize._lbfgsb_py import status_messages, task_messages

from . import _native
from .calibrator import (_MAXFUN, N_PARAMS, PARAM_NAMES, CalibrationResult,
                         DoubleHestonJumpCalibrator, x_to_model)
from .ffn import FFNModel
from .generator import MATURITIES, STRIKES_PCT, grid_surface
from .pricer import implied_vol, resolve_call

OBJECTIVES = ("price", "iv")
GRADIENTS = ("fd", "analytic")
IV_GRADIENTS = ("fd", "vega")                          # objective="iv"'s
METHODS = ("lbfgs", "lm")

FAILED_MESSAGE = "All optimization starts failed"      # lbfgs_calibrator.py:318-333
RANK_RCOND = 1e-12      # uncertainty(): eigenvalues of H at or below this share of the largest are cut


def task_message(task: int, method: str = "lbfgs") -> str:
    """SciPy's message for a task code status * 1000 + message (dh_lb_result.task); under
    method="lm" the message of a DH_LM_* code."""
    if method == "lm":
        return _native.LM_MESSAGES[int(task)]
    return status_messages[int(task) // 1000] + ": " + task_messages[int(task) % 1000]


@dataclass
class ParameterUncertainty:
    """BatchCalibrationResult.uncertainty()'s result, arrays over markets [B]; NaN (rank -1) where
    a market has no winner or its winner's loss is invalid."""
    hessian: np.ndarray          # [B, 13, 13] Gauss-Newton Hessian of the price loss in x
    covariance_x: np.ndarray     # [B, 13, 13] 2 f / dof pinv(H), in the optimiser's x
    covariance: np.ndarray       # [B, 13, 13] the same in model parameters: J covariance_x J
    stderr: np.ndarray           # [B, 13] sqrt of covariance's diagonal
    condition: np.ndarray        # [B] largest / smallest eigenvalue of H (inf: not positive)
    weakest: np.ndarray          # [B, 13] unit eigenvector of H's smallest eigenvalue, in x
    rank: np.ndarray             # [B] eigenvalues above RANK_RCOND times the largest
    dof: int                     # max(M - 13, 1)


def transform_jacobian(x) -> np.ndarray:
    """d(model parameter)/dx of x [..., 13], the transform's diagonal: 1 - tanh(x)^2 for the two
    correlations, 1 for mu_j, exp(x) otherwise."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore"):
        j = np.exp(x)
    j[..., [4, 9]] = 1.0 - np.tanh(x[..., [4, 9]]) ** 2
    j[..., 11] = 1.0
    return j


def gauss_newton_uncertainty(H, f, x, M, valid=None) -> ParameterUncertainty:
    """The 13 x 13 algebra of uncertainty() on the host (NumPy): H [B, 13, 13] symmetric, f [B]
    the losses, x [B, 13] the points, M the options per market, valid [B] bool (default all).
    With H = V diag(e) V', the eigenvalues e_k <= RANK_RCOND max(e) are cut: rank counts the rest,
    pinv(H) = sum_kept v_k v_k' / e_k, covariance_x = 2 f / dof pinv(H) with dof = max(M - 13, 1)
    (sigma^2 (J'J)^-1 for this loss: f = RSS / M and H = 2 J'J / M), condition = max(e) / min(e)
    (inf where min(e) <= 0) and weakest = the eigenvector of min(e), its largest component
    positive."""
    H = np.asarray(H, dtype=np.float64)
    B = H.shape[0]
    f, x = np.asarray(f, dtype=np.float64), np.asarray(x, dtype=np.float64)
    valid = np.ones(B, dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
    dof = max(int(M) - N_PARAMS, 1)
    out = ParameterUncertainty(
        hessian=np.where(valid[:, None, None], H, np.nan),
        covariance_x=np.full((B, N_PARAMS, N_PARAMS), np.nan),
        covariance=np.full((B, N_PARAMS, N_PARAMS), np.nan), stderr=np.full((B, N_PARAMS), np.nan),
        condition=np.full(B, np.nan), weakest=np.full((B, N_PARAMS), np.nan),
        rank=np.full(B, -1, dtype=np.int64), dof=dof)
    for b in np.flatnonzero(valid):
        if not np.all(np.isfinite(H[b])):
            continue
        e, V = np.linalg.eigh(H[b])                    # ascending
        keep = e > RANK_RCOND * e[-1] if e[-1] > 0.0 else np.zeros(N_PARAMS, dtype=bool)
        out.rank[b] = int(keep.sum())
        out.condition[b] = e[-1] / e[0] if e[0] > 0.0 else np.inf
        w = V[:, 0]
        out.weakest[b] = w if w[np.argmax(np.abs(w))] > 0.0 else -w
        pinv = (V[:, keep] / e[keep]) @ V[:, keep].T
        out.covariance_x[b] = (2.0 * f[b] / dof) * pinv
        j = transform_jacobian(x[b])
        out.covariance[b] = j[:, None] * out.covariance_x[b] * j[None, :]
        out.stderr[b] = np.sqrt(np.diag(out.covariance[b]))
    return out


def pick_winners(fun) -> np.ndarray:
    """best start per market of fun [B, S]: the first start, in start order, whose fun is strictly
    below every earlier one's and below inf (lbfgs_calibrator.py:271-275, dh_best_start's rule);
    NaN never wins; -1 where no start qualifies."""
    fun = np.asarray(fun, dtype=np.float64)
    if fun.ndim != 2:
        raise ValueError(f"fun must be [B, S], got {fun.shape}")
    B, S = fun.shape
    if S == 0:
        return np.full(B, -1, dtype=np.int64)
    f = np.where(np.isnan(fun), np.inf, fun)
    best = np.argmin(f, axis=1)                        # the first occurrence of the minimum
    return np.where(f[np.arange(B), best] < np.inf, best, -1)


@dataclass
class BatchCalibrationResult:
    """calibrate_batch's result: arrays over markets [B] and over starts [B, S]."""
    spots: np.ndarray            # [B]
    risk_free: np.ndarray        # [B]
    market_prices: np.ndarray    # [B, M]
    strikes: np.ndarray          # [B, M] absolute strikes of each market
    maturities: np.ndarray       # [M]
    is_call: np.ndarray          # [M] bool
    # per market (the winning start; the reference's failure row where none wins)
    parameters: np.ndarray       # [B, 13] model parameters
    x: np.ndarray                # [B, 13] unconstrained
    final_loss: np.ndarray       # [B]
    iterations: np.ndarray       # [B]
    success: np.ndarray          # [B] bool
    task: np.ndarray             # [B] SciPy task code of the winner (0 where none)
    best_start: np.ndarray       # [B] (-1 where none)
    model_prices: np.ndarray     # [B, M]
    calibration_time: np.ndarray   # [B] seconds until the host saw the winner finish
    # per start
    fun: np.ndarray              # [B, S]
    nit: np.ndarray              # [B, S]
    nfev: np.ndarray             # [B, S]
    start_task: np.ndarray       # [B, S]
    status: np.ndarray           # [B, S] SciPy warnflag
    best_loss: np.ndarray        # [B, S]
    n_calls: np.ndarray          # [B, S]
    start_x: np.ndarray          # [B, S, 13]
    iterations_enqueued: int = 0
    # objective="iv": final_loss, fun and best_loss are vol-space losses
    objective: str = "price"
    market_ivs: np.ndarray = None    # [B, M] the vols fitted (None under "price")
    iv_weights: np.ndarray = None    # [B, M]
    model_ivs: np.ndarray = None     # [B, M] the winners' vols, NaN where a price has none
    # "fd": 14 loss evaluations per request; "analytic" and "vega": one (n_calls == nfev)
    gradient: str = "fd"
    loss_evals: int = 0              # loss evaluations of the whole call: n_calls summed
    # "lbfgs": task holds SciPy's codes; "lm": the DH_LM_* codes, and success is a tolerance stop
    method: str = "lbfgs"
    grid: tuple = None               # calibrate_batch's option grid, _surface's arguments

    def message(self, b: int) -> str:
        if self.best_start[b] < 0:
            return FAILED_MESSAGE
        return task_message(self.task[b], self.method)

    def uncertainty(self, N=128, device=None) -> ParameterUncertainty:
        """How well each market determines its calibrated parameters: one
        Surface.gauss_newton_rows call at the winners' x, then 13 x 13 algebra on the host
        (gauss_newton_uncertainty) -> ParameterUncertainty.  Works after either method, for the
        price objective (the Hessian is the price loss's).

        What the numbers are: a LOCAL estimate at the returned x, from the GAUSS-NEWTON Hessian
        H = 2 J'J / M of the relative price errors (second derivatives of the prices and the Feller
        penalty's curvature are left out), with the COS series' truncation range held FIXED as the
        parameter sensitivities hold it.  covariance_x = 2 f / dof pinv(H), dof = max(M - 13, 1),
        is the usual sigma^2 (J'J)^-1 with the residual variance estimated from the fit itself; it
        says how far the parameters could move before the fit degrades as much as it already
        misses, not how far they are from a true model.  Directions whose eigenvalue is at or below
        RANK_RCOND of the largest are cut from pinv (rank < 13): the standard errors then cover
        the retained directions only.  Markets with no winner get NaN and rank -1."""
        if self.grid is None:
            raise ValueError("uncertainty() needs the option grid of a calibrate_batch result")
        if self.objective != "price":
            raise ValueError("uncertainty() is the price objective's")
        surf = _surface(_native.default_context(device), *self.grid)
        B = self.x.shape[0]
        won = np.flatnonzero(self.best_start >= 0)
        H = np.full((B, N_PARAMS, N_PARAMS), np.nan)
        f = np.full(B, np.nan)
        valid = np.zeros(B, dtype=bool)
        if won.size:
            fw, _, bad, Hw = surf.gauss_newton_rows(self.x[won], self.market_prices, self.spots,
                                                    self.risk_free, won.astype(np.int32), N)
            H[won], f[won] = Hw, fw
            valid[won] = (bad == 0) & np.isfinite(fw)
        return gauss_newton_uncertainty(H, f, self.x, self.market_prices.shape[1], valid)

    def market_options(self, b: int):
        return [{"strike": float(k), "maturity": float(t), "price": float(p),
                 "option_type": "call" if c else "put"}
                for k, t, p, c in zip(self.strikes[b], self.maturities, self.market_prices[b],
                                      self.is_call)]

    def result(self, b: int) -> CalibrationResult:
        """Market b as the reference's CalibrationResult (lbfgs_calibrator.py:21-41)."""
        b = int(b)
        return CalibrationResult(
            date="", spot=float(self.spots[b]), risk_free=float(self.risk_free[b]),
            parameters={n: float(v) for n, v in zip(PARAM_NAMES, self.parameters[b])},
            market_prices=self.market_prices[b].copy(), model_prices=self.model_prices[b].copy(),
            market_options=self.market_options(b), final_loss=float(self.final_loss[b]),
            calibration_time=float(self.calibration_time[b]), success=bool(self.success[b]),
            iterations=int(self.iterations[b]), message=self.message(b))


def _grid(strikes_pct, maturities, strikes, is_call):
    """-> (K [M] in grid order (T outer, K inner), T [M], flags [M] bool, strike mode)."""
    if strikes is not None:
        k, mode = np.asarray(strikes, dtype=np.float64).reshape(-1), _native.STRIKE_ABSOLUTE
    else:
        k, mode = np.asarray(strikes_pct, dtype=np.float64).reshape(-1), _native.STRIKE_PCT_SPOT
    t = np.asarray(maturities, dtype=np.float64).reshape(-1)
    K, T = np.tile(k, t.size), np.repeat(t, k.size)
    if K.size == 0:
        raise ValueError("the option grid is empty")
    if not (np.all(np.isfinite(K)) and np.all(K > 0) and np.all(np.isfinite(T)) and np.all(T > 0)):
        raise ValueError("strikes and maturities must be finite and positive")
    if isinstance(is_call, str):
        flags = np.full(K.size, resolve_call(is_call), dtype=bool)
    else:
        flags = np.asarray(is_call)
        if flags.dtype.kind not in "biu":
            raise ValueError("is_call must be a bool, or bools per option")
        flags = flags.astype(bool)
        if flags.ndim == 0:
            flags = np.full(K.size, bool(flags))
        elif flags.shape != (K.size,):
            raise ValueError(f"is_call must be a scalar or [{K.size}], got {flags.shape}")
    return K, T, flags, mode


def check_markets(market_prices, spots, risk_free, M):
    """-> (market [B, M], spots [B], rates [B]) as float64, or ValueError."""
    mkt = np.ascontiguousarray(market_prices, dtype=np.float64)
    if mkt.ndim != 2 or mkt.shape[1] != M:
        raise ValueError(f"market_prices must be [B, {M}], got {mkt.shape}")
    B = mkt.shape[0]
    sp = np.ascontiguousarray(spots, dtype=np.float64)
    if sp.shape != (B,):
        raise ValueError(f"spots must be [{B}], got {sp.shape}")
    if not (np.all(np.isfinite(sp)) and np.all(sp > 0)):
        raise ValueError("every spot must be finite and > 0")
    r = np.asarray(risk_free, dtype=np.float64)
    if r.ndim == 0:
        r = np.full(B, float(r))
    elif r.shape != (B,):
        raise ValueError(f"risk_free must be a scalar or [{B}], got {r.shape}")
    if not np.all(np.isfinite(r)):
        raise ValueError("every rate must be finite")
    return mkt, sp, np.ascontiguousarray(r)


def check_objective(objective):
    if objective not in OBJECTIVES:
        raise ValueError(f"objective must be 'price' or 'iv', not {objective!r}")
    return objective


def check_gradient(gradient, objective, N):
    """The gradient switch of calibrate_batch, or ValueError: "analytic" differentiates the price
    objective only and "vega" the vol objective only, both on series of at most PARAM_GRAD_MAX_N
    terms."""
    if gradient not in GRADIENTS and gradient not in IV_GRADIENTS:
        raise ValueError(f"gradient must be 'fd', 'analytic' or 'vega', not {gradient!r}")
    if gradient == "analytic" and objective != "price":
        raise ValueError("gradient='analytic' differentiates the price objective only; "
                         "objective='iv' runs gradient='fd' or its exact gradient, "
                         "gradient='vega'")
    if gradient == "vega" and objective != "iv":
        raise ValueError("gradient='vega' differentiates the vol objective (objective='iv') only; "
                         "objective='price' runs gradient='fd' or gradient='analytic'")
    if gradient != "fd":
        if not (isinstance(N, (int, np.integer)) and 1 <= N <= _native.PARAM_GRAD_MAX_N):
            raise ValueError(f"gradient={gradient!r}: N must be a whole number in "
                             f"[1, {_native.PARAM_GRAD_MAX_N}], got {N!r}")
    return gradient


def check_method(method, gradient, objective, N):
    """The optimiser switch of calibrate_batch, or ValueError.  "lm" fits the price objective on
    its analytic Jacobian, whatever `gradient` says -- except "vega", the vol objective's -- on
    series of at most PARAM_GRAD_MAX_N terms."""
    if method not in METHODS:
        raise ValueError(f"method must be 'lbfgs' or 'lm', not {method!r}")
    if method == "lm":
        if objective != "price":
            raise ValueError("method='lm' fits the price objective only; objective='iv' runs "
                             "method='lbfgs'")
        if gradient == "vega":
            raise ValueError("gradient='vega' differentiates the vol objective; method='lm' "
                             "fits the price objective on its analytic Jacobian")
        if not (isinstance(N, (int, np.integer)) and 1 <= N <= _native.PARAM_GRAD_MAX_N):
            raise ValueError(f"method='lm': N must be a whole number in "
                             f"[1, {_native.PARAM_GRAD_MAX_N}], got {N!r}")
    return method


def check_iv_market(market_ivs, iv_weights, B, M):
    """-> (market_ivs [B, M], iv_weights [B, M]) as float64, or ValueError: iv_weights is [M]
    (every market's) or [B, M], default 1, finite, >= 0 and not all 0 in any market; a market vol
    must be finite and >= 0 wherever its weight is positive (the message names the markets and
    options)."""
    iv = np.ascontiguousarray(market_ivs, dtype=np.float64)
    if iv.shape != (B, M):
        raise ValueError(f"market_ivs must be [{B}, {M}], got {iv.shape}")
    if iv_weights is not None:
        w = np.asarray(iv_weights, dtype=np.float64)
        if w.shape not in ((M,), (B, M)):
            raise ValueError(f"iv_weights must be [{M}] or [{B}, {M}], got {w.shape}")
        iv_weights = w
    return _native.iv_rows(M, iv, iv_weights)


def invert_markets(mkt, sp, r, Kabs, T, flags, device=None):
    """The market vols [B, M] of market prices [B, M]: one dh_implied_vol call at each market's
    spot and rate and q = 0 (what DoubleHestonJumpCalibrator(objective="iv") forms for one
    market); NaN where a price has no vol."""
    return np.ascontiguousarray(
        implied_vol(mkt, sp[:, None], Kabs, T[None, :], r[:, None], 0.0, flags[None, :],
                    device=device), dtype=np.float64).reshape(mkt.shape)


def _options(b, mkt, sp, Kabs, T, flags):
    return [{"strike": Kabs[b, j], "maturity": T[j], "price": mkt[b, j],
             "option_type": "call" if flags[j] else "put"} for j in range(T.size)]


def default_starts(mkt, sp, r, Kabs, T, flags, multi_start):
    """The starts a loop of calibrate() calls over the markets would draw, in market order:
    DoubleHestonJumpCalibrator(spot_b, r_b, options_b).start_points(multi_start) -- the only
    consumer of the global RNG, consumed exactly as that loop consumes it.  -> [B, S, 13]."""
    B, S = mkt.shape[0], int(multi_start)
    out = np.empty((B, S, N_PARAMS))
    for b in range(B):
        cal = DoubleHestonJumpCalibrator(float(sp[b]), float(r[b]),
                                         _options(b, mkt, sp, Kabs, T, flags))
        pts = cal.start_points(S)
        if S:
            out[b] = np.stack(pts)
    return out


def check_model_grid(model, strikes_pct, maturities, strikes, flags):
    """ValueError unless the call's option grid is the one the network's price row stands for:
    calls on model.grid = (strikes_pct, maturities), strikes in percent of spot.  A model without
    a stored grid (grid None) is taken at its word: the grid is then the caller's promise."""
    if model.grid is None:
        return
    k, t = model.grid
    same = (strikes is None and bool(np.all(flags))
            and np.array_equal(np.asarray(strikes_pct, dtype=np.float64).reshape(-1), k)
            and np.array_equal(np.asarray(maturities, dtype=np.float64).reshape(-1), t))
    if not same:
        raise ValueError("x0s=model: the network was trained on calls at strikes_pct "
                         f"{k.tolist()} x maturities {t.tolist()}; this call's grid differs")


def resolve_starts(x0s, B):
    """x0s as [B, S, 13] unconstrained: an array of that shape, or [B][S] dicts of the 13 model
    parameters (an FFN's output), mapped as inverse_transform_params maps them."""
    rows = list(x0s) if not isinstance(x0s, np.ndarray) else x0s
    if len(rows) != B:
        raise ValueError(f"x0s must hold {B} markets, got {len(rows)}")
    flat = [e for row in rows for e in (row if not isinstance(row, dict) else [row])]
    n_dict = sum(isinstance(e, dict) for e in flat)
    if n_dict and n_dict != len(flat):
        raise ValueError("x0s mixes parameter dicts and arrays")
    if n_dict:
        if any(isinstance(row, dict) for row in rows):
            raise ValueError("x0s of dicts must be [B][S]: a list of starts per market")
        S = len(rows[0])
        if any(len(row) != S for row in rows):
            raise ValueError("every market needs the same number of starts")
        out = np.empty((B, S, N_PARAMS))
        for b, row in enumerate(rows):
            for s, d in enumerate(row):
                missing = [n for n in PARAM_NAMES if n not in d]
                if missing:
                    raise ValueError(f"x0s[{b}][{s}] lacks {missing}")
                out[b, s] = DoubleHestonJumpCalibrator.inverse_transform_params(None, d)
        return out
    try:
        arr = np.ascontiguousarray(x0s, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"x0s must be [B, S, 13] numbers or [B][S] dicts: {e}") from None
    if arr.ndim != 3 or arr.shape[0] != B or arr.shape[2] != N_PARAMS:
        raise ValueError(f"x0s must be [{B}, S, {N_PARAMS}], got {arr.shape}")
    return arr


def _surface(ctx, K, T, flags, mode, strikes_pct, maturities):
    if mode == _native.STRIKE_PCT_SPOT and flags.all():
        return grid_surface(ctx, strikes_pct, maturities)[0]       # the generator's cached grid
    grids = ctx.__dict__.setdefault("_batch_surfaces", {})
    key = (K.tobytes(), T.tobytes(), flags.tobytes(), mode)
    surf = grids.get(key)
    if surf is None:
        surf = grids[key] = _native.Surface(ctx, K, T, flags.astype(np.int8), strike_mode=mode)
    return surf


def summarize(mkt, sp, r, Kabs, T, flags, X, fun, nit, nfev, task, status, best_loss, n_calls,
              t_done, model_prices_of, enqueued=0, *, objective="price", market_ivs=None,
              iv_weights=None, gradient="fd", method="lbfgs",
              grid=None) -> BatchCalibrationResult:
    """Per-market rows from per-start results [B, S]: the winner of each market
    (pick_winners), re-priced by model_prices_of(params [W, 13], markets [W]) -> [W, M] in one
    call; a market without a winner gets the reference's failure row (zeros, inf, success
    False).  objective="iv": model_prices_of returns (prices [W, M], vols [W, M]) of that one
    call, and the result carries the market vols, the weights and the winners' vols."""
    check_objective(objective)
    B, M = mkt.shape
    best = pick_winners(fun)
    won = np.flatnonzero(best >= 0)
    bw = best[won]
    x = np.zeros((B, N_PARAMS))
    params = np.zeros((B, N_PARAMS))
    final = np.full(B, np.inf)
    iters = np.zeros(B, dtype=np.int64)
    ok = np.zeros(B, dtype=bool)
    wtask = np.zeros(B, dtype=np.int64)
    model = np.zeros((B, M))
    model_iv = np.zeros((B, M)) if objective == "iv" else None
    ctime = np.zeros(B)
    if won.size:
        x[won] = X[won, bw]
        params[won] = x_to_model(x[won])
        final[won] = fun[won, bw]
        iters[won] = nit[won, bw]
        ok[won] = status[won, bw] == 0
        wtask[won] = task[won, bw]
        ctime[won] = t_done[won, bw]
        if objective == "iv":
            model[won], model_iv[won] = model_prices_of(params[won], won)
        else:
            model[won] = model_prices_of(params[won], won)
    return BatchCalibrationResult(
        spots=sp, risk_free=r, market_prices=mkt, strikes=Kabs, maturities=T, is_call=flags,
        parameters=params, x=x, final_loss=final, iterations=iters, success=ok, task=wtask,
        best_start=best, model_prices=model, calibration_time=ctime, fun=fun, nit=nit, nfev=nfev,
        start_task=task, status=status, best_loss=best_loss, n_calls=n_calls, start_x=X,
        iterations_enqueued=enqueued, objective=objective, market_ivs=market_ivs,
        iv_weights=iv_weights, model_ivs=model_iv, gradient=gradient,
        loss_evals=int(np.sum(n_calls)), method=method, grid=grid)


def calibrate_batch(market_prices, spots, risk_free, *, strikes_pct=STRIKES_PCT,
                    maturities=MATURITIES, strikes=None, is_call=True, x0s=None, multi_start=3,
                    maxiter=300, N=128, device=None, chunk=8, objective="price",
                    market_ivs=None, iv_weights=None, gradient="fd",
                    method="lbfgs") -> BatchCalibrationResult:
    """Calibrate B markets that share one option grid, all starts of all markets together in the
    device-resident L-BFGS-B.

    market_prices [B, M] in grid order (maturity outer, strike inner -- the generator's), spots
    [B], risk_free a scalar or [B].  The grid is strikes_pct x maturities (strikes in percent of
    each market's spot), or strikes x maturities (absolute, the same for every market).
    x0s: [B, S, 13] unconstrained start points, [B][S] dicts of the 13 model parameters, an
    FFNModel (one start per market, [B, 1, 13], from ``model.predict`` on the device: the hybrid
    scheme is this call with maxiter=10; the global RNG is not consumed; a model that carries its
    grid refuses another one with ValueError, for a model without one -- ``model.grid`` None --
    the grid is the caller's promise), or None for each
    market's start_points(multi_start) (the global RNG is consumed as a loop of calibrate() calls
    over the markets would consume it).

    objective="price" (the default) fits relative price errors, the reference's loss.
    objective="iv" fits Black-Scholes vols: market_ivs [B, M] (default: the device inversion of
    market_prices at each market's spot and rate and q = 0, one call) under iv_weights [M] or
    [B, M] (default 1; 0 drops an option), loss = sum w (iv_model - iv_mkt)^2 / sum(w) + Feller.
    A market without a vol at a positive weight raises ValueError naming the markets and options,
    before any start is drawn.  final_loss and fun are then vol-space losses and the result's
    model_ivs holds the winners' vols.  The generator's vols fit as they are:

        g = generate_synthetic_calibrations(n, None, as_arrays=True, implied_vols=True)
        calibrate_batch(g["market_prices"], g["spot"], g["risk_free"], objective="iv",
                        market_ivs=g["market_iv"], x0s=...)

    One market in vol space on the device is this call with B = 1.

    gradient="fd" (the default): SciPy's forward differences on the device, 14 loss evaluations
    per request, the reference's optimiser.  gradient="analytic": the loss and its exact gradient
    from one evaluation per request (dh_calibrate_lbfgs_batch_grad: the COS series differentiated
    term by term at a fixed truncation range); the price objective only, N <= 1024.  The result's
    n_calls and loss_evals then count one evaluation per request (n_calls == nfev).  On the Feller
    kink the analytic gradient is the penalty's one-sided derivative, not the forward quotient's
    slope, so a start on it may move where the "fd" run stalls.  One market with the analytic
    gradient on the device is this call with B = 1 (calibrate(driver="device") runs "fd" only).
    gradient="vega": the same for objective="iv", and for it only
    (dh_calibrate_lbfgs_batch_iv_grad: each option's price sensitivities divided by its
    Black-Scholes vega at the model vol); N <= 1024, n_calls == nfev.  An option whose model price
    sits at its lower bound (vol 0.0) adds its residual to the loss and nothing to the gradient,
    the one-sided rule of the Feller kink.

    method="lbfgs" (the default): the device-resident L-BFGS-B, as above.  method="lm":
    Levenberg-Marquardt on the Gauss-Newton Hessian of the price loss (dh_calibrate_lm_batch,
    DESIGN.md 3.21): every request is the parameter planes, reduced to the loss, its gradient and
    the 13 x 13 Hessian, and one damped Cholesky step.  The price objective only, N <= 1024; the
    Jacobian is always the analytic planes, so `gradient` is not consulted (gradient="vega" and
    objective="iv" raise ValueError).  nit counts accepted steps, nfev == n_calls requests; the
    returned x is the last accepted point, so fun never exceeds the start's loss; task holds an
    LM_* code (result.message(b) names it) and success means a tolerance stop.

    result.uncertainty() estimates, after either method, how well each market determines its
    parameters."""
    check_objective(objective)
    check_method(method, gradient, objective, N)
    if method == "lbfgs":
        check_gradient(gradient, objective, N)
    if objective == "price" and (market_ivs is not None or iv_weights is not None):
        raise ValueError("market_ivs and iv_weights belong to objective='iv'")
    K, T, flags, mode = _grid(strikes_pct, maturities, strikes, is_call)
    mkt, sp, r = check_markets(market_prices, spots, risk_free, K.size)
    B = mkt.shape[0]
    Kabs = (K[None, :] * sp[:, None] / 100.0 if mode == _native.STRIKE_PCT_SPOT
            else np.broadcast_to(K, (B, K.size)).copy())
    ivs = wts = None
    if objective == "iv":                               # before any RNG draw
        if market_ivs is None:
            market_ivs = invert_markets(mkt, sp, r, Kabs, T, flags, device)
        ivs, wts = check_iv_market(market_ivs, iv_weights, B, K.size)
    if x0s is None:
        if int(multi_start) < 0:
            raise ValueError("multi_start < 0")
        X = default_starts(mkt, sp, r, Kabs, T, flags, multi_start)
    elif isinstance(x0s, FFNModel):
        # one start per market from the network's device forward; no RNG draw
        check_model_grid(x0s, strikes_pct, maturities, strikes, flags)
        X = np.ascontiguousarray(x0s.predict(mkt, sp, device)[:, None, :])
    else:
        X = resolve_starts(x0s, B)
    S = X.shape[1]
    ctx = _native.default_context(device)
    surf = _surface(ctx, K, T, flags, mode, strikes_pct, maturities)
    market_of = np.repeat(np.arange(B, dtype=np.int32), S)
    if objective == "iv":
        run = (surf.calibrate_lbfgs_batch_iv_grad if gradient == "vega"
               else surf.calibrate_lbfgs_batch_iv)
        res, enqueued = run(ivs, wts, sp, r, X.reshape(B * S, N_PARAMS), market_of, N,
                            maxiter=maxiter, maxfun=_MAXFUN, chunk=chunk)
    else:
        run = (surf.calibrate_lm_batch if method == "lm"
               else surf.calibrate_lbfgs_batch_grad if gradient == "analytic"
               else surf.calibrate_lbfgs_batch)
        res, enqueued = run(mkt, sp, r, X.reshape(B * S, N_PARAMS), market_of, N,
                            maxiter=maxiter, maxfun=_MAXFUN, chunk=chunk)

    def col(name, dtype):
        return np.array([getattr(q, name) for q in res], dtype=dtype).reshape(B, S)

    Xf = np.array([q.x[:] for q in res], dtype=np.float64).reshape(B, S, N_PARAMS)

    def model_prices_of(params, markets):
        rec = np.zeros((params.shape[0], _native.PARAM_STRIDE))
        rec[:, :13] = params
        rec[:, 13] = sp[markets]
        rec[:, 14] = r[markets]
        if objective == "iv":                          # priced and inverted in one call
            iv, prices = surf.implied_vol(rec, N, want_prices=True)
            return prices, iv
        return surf.price(rec, N)                      # every winner in one launch

    return summarize(mkt, sp, r, Kabs, T, flags, Xf, col("fun", np.float64),
                     col("nit", np.int64), col("nfev", np.int64), col("task", np.int64),
                     col("warnflag", np.int64), col("best_loss", np.float64),
                     col("n_calls", np.int64), col("t_done", np.float64), model_prices_of,
                     enqueued, objective=objective, market_ivs=ivs, iv_weights=wts,
                     gradient="analytic" if method == "lm" else gradient, method=method,
                     grid=(K, T, flags, mode, strikes_pct, maturities))
