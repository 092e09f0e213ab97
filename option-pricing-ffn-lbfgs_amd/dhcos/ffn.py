"""The warm start: a feed-forward network from a quoted surface to an optimiser start point.

The reference's documents (docs/THEORY.md 6-7, docs/METHODOLOGY.md 3-4) describe a network that maps
a few features of the quoted surface to the thirteen parameters and whose prediction starts a short
L-BFGS-B run; the reference ships no code for it.  Here:

    model, hist = train_ffn_on_generator(100_000)            # PyTorch-ROCm: plumbing
    x0 = model.predict(market_prices, spots)                 # one launch of ffn_forward_kernel
    res = calibrate_batch(market_prices, spots, r, x0s=model, maxiter=10, gradient="analytic")

Every documented feature is linear in the prices, so the input is f = (C p) / S0 for one matrix C
(``price_features`` builds the documented eleven).  The target is the optimiser's own x -- log of
the positive parameters, arctanh of the correlations, mu_j as it is -- standardised; the output
therefore needs no clipping and goes into the drivers unchanged (the reference's text regresses raw
correlations).  Training is torch.nn (Linear -> BatchNorm1d -> ReLU (-> Dropout),
Adam, MSE, early stopping); on export BatchNorm's evaluation statistics are folded into W and b in
float64 and rounded once to float32.  Inference is the hand-written gfx950 kernel (csrc/dh_ffn.h):
there is no torch in ``predict`` and no CPU fallback.
"""
from __future__ import annotations

import time

import numpy as np

from . import _native
from .calibrator import _EXP, _IDENT, _TANH, N_PARAMS, x_to_model

DEFAULT_HIDDEN = (512, 256, 128, 64)        # METHODOLOGY 3.2
_NPZ_VERSION = 1


def model_to_x(params) -> np.ndarray:
    """Model parameters [..., 13] -> the optimiser's x, as inverse_transform_params maps one set:
    log of the positive ones, arctanh of the correlations clipped to +-0.999, mu_j unchanged."""
    P = np.asarray(params, dtype=np.float64)
    if P.shape[-1] != N_PARAMS:
        raise ValueError(f"params must be [..., {N_PARAMS}], got {P.shape}")
    X = np.empty_like(P)
    X[..., _EXP] = np.log(P[..., _EXP])
    X[..., _TANH] = np.arctanh(np.clip(P[..., _TANH], -0.999, 0.999))
    X[..., _IDENT] = P[..., _IDENT]
    return X


def price_features(strikes_pct, maturities):
    """The documented features of a strikes x maturities grid of calls, as a matrix over the
    market's price row (maturity outer, strike inner: the generator's order).  Per maturity: the
    ATM price (the strike nearest 100 %), the skew P(highest strike) - P(lowest strike) and the
    convexity P(lowest) + P(highest) - 2 P(ATM); then the term slope ATM(last T) - ATM(first T)
    and the sum of the ATM prices.  -> (C float64 [3 n_T + 2, n_K n_T], the feature names)."""
    k = np.asarray(strikes_pct, dtype=np.float64).reshape(-1)
    t = np.asarray(maturities, dtype=np.float64).reshape(-1)
    if k.size < 1 or t.size < 1:
        raise ValueError("the grid is empty")
    nK, nT = k.size, t.size
    atm, lo, hi = int(np.argmin(np.abs(k - 100.0))), int(np.argmin(k)), int(np.argmax(k))
    C = np.zeros((3 * nT + 2, nK * nT))
    names = []
    for i in range(nT):
        base = i * nK
        C[3 * i, base + atm] = 1.0
        C[3 * i + 1, base + hi] += 1.0
        C[3 * i + 1, base + lo] -= 1.0
        C[3 * i + 2, base + lo] += 1.0
        C[3 * i + 2, base + hi] += 1.0
        C[3 * i + 2, base + atm] -= 2.0
        names += [f"atm_T{t[i]:g}", f"skew_T{t[i]:g}", f"convexity_T{t[i]:g}"]
        C[3 * nT + 1, base + atm] += 1.0
    C[3 * nT, (nT - 1) * nK + atm] += 1.0
    C[3 * nT, atm] -= 1.0
    names += ["term_slope", "atm_sum"]
    return C, names


def mlp_forward(weights, biases, z) -> np.ndarray:
    """NumPy float64 forward of a folded stack on standardised inputs z [B, F]: ReLU after every
    layer but the last.  -> [B, out]."""
    a = np.asarray(z, dtype=np.float64)
    for l, (W, b) in enumerate(zip(weights, biases)):
        a = a @ np.asarray(W, dtype=np.float64).T + np.asarray(b, dtype=np.float64)
        if l + 1 < len(weights):
            a = np.maximum(a, 0.0)
    return a


def _check_hidden(hidden):
    hidden = tuple(int(h) for h in hidden)
    if not 1 <= len(hidden) <= _native.FFN_MAX_HIDDEN:
        raise ValueError(f"between 1 and {_native.FFN_MAX_HIDDEN} hidden layers, got {len(hidden)}")
    for h in hidden:
        if h < 32 or h > _native.FFN_MAX_WIDTH or h % 32:
            raise ValueError(f"hidden width {h}: a multiple of 32 in [32, {_native.FFN_MAX_WIDTH}]")
    return hidden


class FFNModel:
    """A trained warm-start network, a plain container:

    features   float64 C [F, M]: the network's input is f = (C p) / S0 of a price row p [M]
    x_mean, x_std [F]; y_mean, y_std [13]   float64 standardisation of the input and the target
    weights, biases   per layer W_l [out, in] and b_l [out] as float32, BatchNorm folded in
    feature_names     optional list of F names
    grid              optional (strikes_pct, maturities) of the calls the price row holds, maturity
                      outer and strike inner; where it is set, calibrate_batch(x0s=model) refuses
                      another grid

    ``widths`` is (F, h_1 ... h_L, 13) with 1 <= L <= 6 hidden widths, each a multiple of 32 in
    [32, 512]; F, M <= 64."""

    def __init__(self, features, x_mean, x_std, y_mean, y_std, weights, biases,
                 feature_names=None, grid=None):
        self.features = np.ascontiguousarray(features, dtype=np.float64)
        self.x_mean = np.ascontiguousarray(x_mean, dtype=np.float64).reshape(-1)
        self.x_std = np.ascontiguousarray(x_std, dtype=np.float64).reshape(-1)
        self.y_mean = np.ascontiguousarray(y_mean, dtype=np.float64).reshape(-1)
        self.y_std = np.ascontiguousarray(y_std, dtype=np.float64).reshape(-1)
        self.weights = [np.ascontiguousarray(w, dtype=np.float32) for w in weights]
        self.biases = [np.ascontiguousarray(b, dtype=np.float32).reshape(-1) for b in biases]
        self.feature_names = None if feature_names is None else [str(n) for n in feature_names]
        self.grid = None if grid is None else tuple(
            np.ascontiguousarray(g, dtype=np.float64).reshape(-1) for g in grid)
        self._devices = {}                 # Context -> _native.FFN
        self._validate()

    def _validate(self):
        C = self.features
        if C.ndim != 2 or not (1 <= C.shape[0] <= _native.FFN_MAX_IN
                               and 1 <= C.shape[1] <= _native.FFN_MAX_IN):
            raise ValueError(f"features must be [F, M] with F, M in [1, {_native.FFN_MAX_IN}], "
                             f"got {C.shape}")
        F = C.shape[0]
        if len(self.weights) != len(self.biases) or len(self.weights) < 2:
            raise ValueError("one weight matrix and one bias per layer, two layers at least")
        if any(w.ndim != 2 for w in self.weights):
            raise ValueError("every weight matrix must be [out, in]")
        widths = (self.weights[0].shape[1],) + tuple(w.shape[0] for w in self.weights)
        if widths[0] != F or widths[-1] != N_PARAMS:
            raise ValueError(f"widths must run from F = {F} to {N_PARAMS}, got {widths}")
        _check_hidden(widths[1:-1])
        for l, (w, b) in enumerate(zip(self.weights, self.biases)):
            if w.shape != (widths[l + 1], widths[l]) or b.shape != (widths[l + 1],):
                raise ValueError(f"layer {l}: W {w.shape}, b {b.shape} do not chain")
            if not (np.all(np.isfinite(w)) and np.all(np.isfinite(b))):
                raise ValueError(f"layer {l}: weights must be finite")
        if self.x_mean.shape != (F,) or self.x_std.shape != (F,):
            raise ValueError(f"x_mean and x_std must be [{F}]")
        if self.y_mean.shape != (N_PARAMS,) or self.y_std.shape != (N_PARAMS,):
            raise ValueError(f"y_mean and y_std must be [{N_PARAMS}]")
        stats = np.concatenate([self.x_mean, self.x_std, self.y_mean, self.y_std, C.reshape(-1)])
        if not np.all(np.isfinite(stats)) or not np.all(self.x_std > 0):
            raise ValueError("features and statistics must be finite, x_std > 0")
        if self.feature_names is not None and len(self.feature_names) != F:
            raise ValueError(f"feature_names must hold {F} names")
        if self.grid is not None and (len(self.grid) != 2 or
                                      self.grid[0].size * self.grid[1].size != C.shape[1]):
            raise ValueError(f"grid must be (strikes_pct, maturities) of {C.shape[1]} options")

    @property
    def widths(self):
        return (self.weights[0].shape[1],) + tuple(w.shape[0] for w in self.weights)

    @property
    def n_features(self):
        return self.features.shape[0]

    @property
    def n_prices(self):
        return self.features.shape[1]

    # ---- files ----------------------------------------------------------------------------
    def save(self, path):
        """Write the model as an .npz of plain arrays (no pickled objects)."""
        arrays = dict(version=np.array(_NPZ_VERSION), features=self.features, x_mean=self.x_mean,
                      x_std=self.x_std, y_mean=self.y_mean, y_std=self.y_std,
                      n_layers=np.array(len(self.weights)))
        for l, (w, b) in enumerate(zip(self.weights, self.biases)):
            arrays[f"W{l}"], arrays[f"b{l}"] = w, b
        if self.feature_names is not None:
            arrays["feature_names"] = np.array(self.feature_names, dtype=np.str_)
        if self.grid is not None:
            arrays["grid_strikes_pct"], arrays["grid_maturities"] = self.grid
        with open(path, "wb") as fh:
            np.savez(fh, **arrays)

    @classmethod
    def load(cls, path):
        """Read a model written by ``save``; a file with pickled (object) content is refused
        (``allow_pickle=False``: ValueError)."""
        with np.load(path, allow_pickle=False) as z:
            n = int(z["n_layers"])
            names = [str(s) for s in z["feature_names"]] if "feature_names" in z.files else None
            return cls(z["features"], z["x_mean"], z["x_std"], z["y_mean"], z["y_std"],
                       [z[f"W{l}"] for l in range(n)], [z[f"b{l}"] for l in range(n)], names,
                       (z["grid_strikes_pct"], z["grid_maturities"])
                       if "grid_strikes_pct" in z.files else None)

    # ---- evaluation -----------------------------------------------------------------------
    def _check_inputs(self, market_prices, spots):
        p = np.ascontiguousarray(market_prices, dtype=np.float64)
        if p.ndim != 2 or p.shape[1] != self.n_prices:
            raise ValueError(f"market_prices must be [B, {self.n_prices}], got {p.shape}")
        s = np.ascontiguousarray(spots, dtype=np.float64)
        if s.ndim == 0:
            s = np.full(p.shape[0], float(s))
        if s.shape != (p.shape[0],):
            raise ValueError(f"spots must be [{p.shape[0]}], got {s.shape}")
        if not (np.all(np.isfinite(p)) and np.all(p > 0)):
            raise ValueError("every market price must be finite and > 0")
        if not (np.all(np.isfinite(s)) and np.all(s > 0)):
            raise ValueError("every spot must be finite and > 0")
        return p, s

    def input_features(self, market_prices, spots) -> np.ndarray:
        """f = (C p) / S0 of every market, float64 [B, F] (not standardised)."""
        p, s = self._check_inputs(market_prices, spots)
        return (p @ self.features.T) / s[:, None]

    def forward_reference(self, market_prices, spots, want_raw=False):
        """The NumPy float64 forward of the stored float32 weights: the truth the device and its
        host twin are held to.  -> x0 [B, 13] (and the standardised output [B, 13] in float64)."""
        z = (self.input_features(market_prices, spots) - self.x_mean) / self.x_std
        raw = mlp_forward(self.weights, self.biases, z)
        x0 = self.y_mean + self.y_std * raw
        return (x0, raw) if want_raw else x0

    def on_device(self, device=None) -> "_native.FFN":
        """The network resident on ``device``'s default context (uploaded once, cached)."""
        ctx = _native.default_context(device)
        dev = self._devices.get(ctx)
        if dev is None or dev.handle is None or ctx.handle is None:
            dev = self._devices[ctx] = _native.FFN(ctx, self.widths, self.weights, self.biases,
                                                   self.features, self.x_mean, self.x_std,
                                                   self.y_mean, self.y_std)
        return dev

    def predict(self, market_prices, spots, device=None, want_raw=False):
        """x0 [B, 13], the optimiser-space start point of every market, from one launch of the
        device kernel.  ValueError before any launch for a wrong shape, a non-finite or
        non-positive price, or a non-positive spot."""
        p, s = self._check_inputs(market_prices, spots)
        return self.on_device(device).forward(p, s, want_raw=want_raw)

    def predict_parameters(self, market_prices, spots, device=None) -> np.ndarray:
        """``predict`` through x_to_model: [B, 13] model parameters."""
        return x_to_model(self.predict(market_prices, spots, device))


# ---- training (PyTorch-ROCm: plumbing) --------------------------------------------------------
def build_stack(widths, dropout=0.0):
    """The torch.nn stack of widths (F, h_1 ... h_L, out): Linear -> BatchNorm1d -> ReLU
    (-> Dropout) per hidden layer, then Linear."""
    import torch.nn as nn
    layers = []
    for i, o in zip(widths[:-2], widths[1:-1]):
        layers += [nn.Linear(i, o), nn.BatchNorm1d(o), nn.ReLU()]
        if dropout > 0.0:
            layers.append(nn.Dropout(dropout))
    layers.append(nn.Linear(widths[-2], widths[-1]))
    return nn.Sequential(*layers)


def fold_batchnorm(stack):
    """The stack's Linear layers with the following BatchNorm1d's evaluation statistics folded in,
    in float64: W' = s W, b' = s (b - running_mean) + beta with s = gamma / sqrt(running_var +
    eps).  -> (weights, biases), float64 arrays, not yet rounded."""
    import torch.nn as nn
    mods = list(stack)
    Ws, bs = [], []
    for i, m in enumerate(mods):
        if not isinstance(m, nn.Linear):
            continue
        W = m.weight.detach().cpu().double().numpy().copy()
        b = m.bias.detach().cpu().double().numpy().copy()
        bn = mods[i + 1] if i + 1 < len(mods) and isinstance(mods[i + 1], nn.BatchNorm1d) else None
        if bn is not None:
            var = bn.running_var.detach().cpu().double().numpy()
            mean = bn.running_mean.detach().cpu().double().numpy()
            gamma = bn.weight.detach().cpu().double().numpy()
            beta = bn.bias.detach().cpu().double().numpy()
            s = gamma / np.sqrt(var + float(bn.eps))
            W = s[:, None] * W
            b = s * (b - mean) + beta
        Ws.append(W)
        bs.append(b)
    return Ws, bs


def _load_folded(stack, model, z):
    """Start the stack from a folded model so that it is the model's function in evaluation mode
    and close to it in training mode.  The Linear layers take the folded W and b.  Each
    BatchNorm1d takes the statistics of its own input under the model on the training rows z
    (standardised float32 [n, F]): running_mean = mu, running_var = var (the biased variance a
    training batch normalises by), gamma = sqrt(var + eps) and beta = mu.  In evaluation mode the
    layer is then the identity exactly as far as float32 allows, and in training mode a batch's own
    statistics differ from mu and var by sampling noise only, where identity statistics (mean 0,
    variance 1) would re-normalise the pre-activations into a different function."""
    import torch
    import torch.nn as nn
    mods = list(stack)
    lin = [m for m in mods if isinstance(m, nn.Linear)]
    was_training = stack.training
    stack.eval()
    with torch.no_grad():
        for m, W, b in zip(lin, model.weights, model.biases):
            m.weight.copy_(torch.from_numpy(W.astype(np.float32)))
            m.bias.copy_(torch.from_numpy(b.astype(np.float32)))
        a = z
        for m in mods:
            if isinstance(m, nn.BatchNorm1d):
                mu = a.mean(dim=0)
                var = a.var(dim=0, unbiased=False)
                m.running_mean.copy_(mu)
                m.running_var.copy_(var)
                m.weight.copy_(torch.sqrt(var + float(m.eps)))
                m.bias.copy_(mu)
            a = m(a)
    stack.train(was_training)


def train_ffn(features, targets, *, widths=DEFAULT_HIDDEN, epochs=200, batch_size=256, lr=1e-3,
              patience=15, val_fraction=0.15, dropout=0.0, seed=0, init=None, device=None,
              feature_matrix=None, feature_names=None, grid=None):
    """Train the warm-start network: features [n, F] (the network's inputs f = (C p) / S0),
    targets [n, 13] (the optimiser's x) -> (FFNModel, history).

    widths: the hidden widths.  Adam on the MSE of the standardised targets; the last
    ``val_fraction`` of a seeded shuffle is held out and early stopping watches its loss
    (``patience`` epochs without a new best); the best epoch's weights are the result -- the
    state before the first step counts, so continuing from ``init`` never returns a model whose
    validation loss is above its starting value.  ``init=model`` continues from a model (its
    widths and its standardisation are kept, and every BatchNorm1d starts from the statistics of
    its own input under the model, so the first training step already sees the model's function; lr=1e-5, batch_size=32, epochs=50, patience=10 is the
    documented stage 2).  device=None trains on the GPU when torch sees one, on the CPU otherwise.
    feature_matrix is the model's C [F, M] (default: the identity, a model over the features
    themselves with S0 = 1); grid the (strikes_pct, maturities) its price row stands for, kept in
    the model.  history: per-epoch ``train`` and ``val`` losses, ``initial_val``,
    ``best_val``, ``best_epoch`` (0 = the starting state) and ``seconds``."""
    import torch
    t0 = time.perf_counter()
    X = np.ascontiguousarray(features, dtype=np.float64)
    Y = np.ascontiguousarray(targets, dtype=np.float64)
    if X.ndim != 2 or Y.ndim != 2 or X.shape[0] != Y.shape[0] or Y.shape[1] != N_PARAMS:
        raise ValueError(f"features [n, F] and targets [n, {N_PARAMS}], got {X.shape}, {Y.shape}")
    if not (np.all(np.isfinite(X)) and np.all(np.isfinite(Y))):
        raise ValueError("features and targets must be finite")
    n, F = X.shape
    C = np.eye(F) if feature_matrix is None else np.asarray(feature_matrix, dtype=np.float64)
    if C.ndim != 2 or C.shape[0] != F:
        raise ValueError(f"feature_matrix must be [{F}, M], got {C.shape}")
    n_val = int(round(n * float(val_fraction)))
    if not 0 < n_val < n:
        raise ValueError("val_fraction leaves no training or no validation sample")
    if init is not None:
        if init.n_features != F:
            raise ValueError(f"init has {init.n_features} features, the data {F}")
        hidden = init.widths[1:-1]
        x_mean, x_std, y_mean, y_std = init.x_mean, init.x_std, init.y_mean, init.y_std
        if feature_matrix is None:
            C = init.features
        if feature_names is None:
            feature_names = init.feature_names
        if grid is None:
            grid = init.grid
    else:
        hidden = _check_hidden(widths)
    rs = np.random.RandomState(int(seed))
    order = rs.permutation(n)
    tr, va = order[:n - n_val], order[n - n_val:]
    if init is None:
        x_mean, x_std = X[tr].mean(axis=0), X[tr].std(axis=0)
        y_mean, y_std = Y[tr].mean(axis=0), Y[tr].std(axis=0)
        x_std = np.where(x_std > 0, x_std, 1.0)
        y_std = np.where(y_std > 0, y_std, 1.0)
    dev = torch.device(device if device is not None
                       else ("cuda" if torch.cuda.is_available() else "cpu"))
    Z = torch.from_numpy(((X - x_mean) / x_std).astype(np.float32)).to(dev)
    T = torch.from_numpy(((Y - y_mean) / y_std).astype(np.float32)).to(dev)
    tr_t, va_t = torch.from_numpy(tr).to(dev), torch.from_numpy(va).to(dev)
    torch.manual_seed(int(seed))
    net = build_stack((F,) + tuple(hidden) + (N_PARAMS,), dropout).to(dev)
    if init is not None:
        _load_folded(net, init, Z[tr_t])
    opt = torch.optim.Adam(net.parameters(), lr=float(lr))
    loss_fn = torch.nn.MSELoss()

    def val_loss():
        net.eval()
        with torch.no_grad():
            return float(loss_fn(net(Z[va_t]), T[va_t]))

    def snapshot():
        return {k: v.detach().clone() for k, v in net.state_dict().items()}

    hist = {"train": [], "val": [], "initial_val": val_loss(), "best_epoch": 0}
    best, best_state, since = hist["initial_val"], snapshot(), 0
    if init is None:
        best = float("inf")               # a fresh network's starting state is no candidate
    bs = max(2, int(batch_size))          # BatchNorm needs two samples per batch
    for epoch in range(1, int(epochs) + 1):
        net.train()
        perm = torch.from_numpy(rs.permutation(tr.size)).to(dev)
        total, seen = 0.0, 0
        for i in range(0, tr.size, bs):
            idx = tr_t[perm[i:i + bs]]
            if idx.numel() < 2:
                continue
            opt.zero_grad(set_to_none=True)
            loss = loss_fn(net(Z[idx]), T[idx])
            loss.backward()
            opt.step()
            total += float(loss.detach()) * idx.numel()
            seen += idx.numel()
        v = val_loss()
        hist["train"].append(total / max(seen, 1))
        hist["val"].append(v)
        if v < best:
            best, best_state, since = v, snapshot(), 0
            hist["best_epoch"] = epoch
        else:
            since += 1
            if since >= int(patience):
                break
    net.load_state_dict(best_state)
    net.eval()
    Ws, bs_ = fold_batchnorm(net)
    model = FFNModel(C, x_mean, x_std, y_mean, y_std, [w.astype(np.float32) for w in Ws],
                     [b.astype(np.float32) for b in bs_], feature_names, grid)
    hist["best_val"] = best
    hist["seconds"] = time.perf_counter() - t0
    return model, hist


def _grid_features(market_prices, spots, strikes_pct, maturities):
    C, names = price_features(strikes_pct, maturities)
    p = np.asarray(market_prices, dtype=np.float64)
    s = np.asarray(spots, dtype=np.float64).reshape(-1)
    if p.ndim != 2 or p.shape[1] != C.shape[1] or s.size != p.shape[0]:
        raise ValueError(f"market_prices must be [B, {C.shape[1]}] and spots [B]")
    return C, names, (p @ C.T) / s[:, None]


def train_ffn_on_generator(n_samples=100_000, *, gen_seed=None, N=128, gen_device=None, **train):
    """``train_ffn`` on ``generate_synthetic_calibrations(n_samples, None, as_arrays=True)``: the
    features from its market_prices and spot (``price_features`` of the generator's grid), the
    targets from its params.  gen_seed (None: the global RNG as it stands) seeds NumPy's global
    RNG, which the generator consumes.  The other keywords are ``train_ffn``'s."""
    from .generator import MATURITIES, STRIKES_PCT, generate_synthetic_calibrations
    if gen_seed is not None:
        np.random.seed(int(gen_seed))
    g = generate_synthetic_calibrations(int(n_samples), None, N=N, device=gen_device,
                                        as_arrays=True, verbose=False)
    C, names, f = _grid_features(g["market_prices"], g["spot"], STRIKES_PCT, MATURITIES)
    return train_ffn(f, model_to_x(np.asarray(g["params"])), feature_matrix=C,
                     feature_names=names, grid=(STRIKES_PCT, MATURITIES), **train)


def fine_tune_ffn(model, result, *, lr=1e-5, batch_size=32, epochs=50, patience=10, **train):
    """Stage 2: continue ``model`` on the calibrated markets of a BatchCalibrationResult -- its
    market_prices and spots as the input, its x as the target, the successful markets only."""
    ok = np.asarray(result.success, dtype=bool)
    if ok.sum() < 4:
        raise ValueError("fine_tune_ffn needs a few successfully calibrated markets")
    f = model.input_features(result.market_prices[ok], result.spots[ok])
    return train_ffn(f, result.x[ok], init=model, lr=lr, batch_size=batch_size, epochs=epochs,
                     patience=patience, **train)
