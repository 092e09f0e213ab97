"""Shared material of the warm-start network's tests (tests/test_ffn.py, tests/test_gpu_ffn.py):
the host twin's binding, the models and markets under test, and the derived forward error bound.

The bound (float32 unit roundoff u = 2^-24, gamma_K = K u / (1 - K u)): the standardised feature
is rounded once to float32, delta_0 = u |z|; a layer of K inputs is, per neuron, one fmaf chain of
K + 1 terms started from the bias, so with a the truth's input of the layer and delta the bound
on the computed input's error,

    delta' = |W| delta + gamma_{K+1} (|b| + |W| (|a| + delta)),

and ReLU, being 1-Lipschitz, keeps delta.  The epilogue is one fp64 fma, the truth's two fp64
operations and the prologue's few: 4 * 2^-52 (|y_mean| + |y_std raw|) covers them.  The bar on x0
is |y_std| delta_L + that.  Everything is computed in float64 from the stored float32 weights.
"""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 2.0 ** -24
WIDTH_SETS = ((11, 32, 13), (11, 64, 32, 13), (11, 512, 256, 128, 64, 13))
TM = 32
BATCHES = (1, TM, TM + 1, 3 * TM - 1)          # the tail cases

_D = C.POINTER(C.c_double)
_F = C.POINTER(C.c_float)
_I = C.POINTER(C.c_int)


def ffnhost():
    lib = C.CDLL(os.path.join(ROOT, "tests", "native", "libffnhost.so"))
    lib.ffnh_forward.restype = C.c_int
    lib.ffnh_forward.argtypes = [C.c_int, _I, _F, _F, _D, C.c_int, _D, _D, _D, _D, _D, _D,
                                 C.c_int64, _D, _F]
    return lib


def twin_forward(model, market, spots, weights=None, biases=None):
    """The host twin (tests/native/libffnhost.so) on a model -> (x0 float64 [B, 13], raw float32
    [B, 13]); weights / biases override the model's (the injected-slip checks)."""
    lib = ffnhost()
    weights = model.weights if weights is None else weights
    biases = model.biases if biases is None else biases
    widths = np.ascontiguousarray(model.widths, dtype=np.int32)
    w = np.concatenate([np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in weights])
    b = np.concatenate([np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in biases])
    market = np.ascontiguousarray(market, dtype=np.float64)
    spots = np.ascontiguousarray(spots, dtype=np.float64)
    B = market.shape[0]
    x0, raw = np.empty((B, 13)), np.empty((B, 13), dtype=np.float32)
    d = lambda a: a.ctypes.data_as(_D)      # noqa: E731
    rc = lib.ffnh_forward(len(weights), widths.ctypes.data_as(_I), w.ctypes.data_as(_F),
                          b.ctypes.data_as(_F), d(model.features), model.n_prices,
                          d(model.x_mean), d(model.x_std), d(model.y_mean), d(model.y_std),
                          d(market), d(spots), B, d(x0), raw.ctypes.data_as(_F))
    assert rc == 0
    return x0, raw


def markets(B, seed=5):
    """B markets on the generator's 5 x 3 grid: decreasing-in-strike positive prices, spots near
    100 -> (market [B, 15], spots [B])."""
    rs = np.random.RandomState(seed)
    spots = 100.0 * (1.0 + 0.05 * rs.randn(B))
    k = np.tile(np.array([0.9, 0.95, 1.0, 1.05, 1.1]), 3)
    t = np.repeat(np.array([0.25, 0.5, 1.0]), 5)
    vol = 0.15 + 0.15 * rs.rand(B, 1)
    level = np.maximum(1.0 - k, 0.0) + 0.4 * vol * np.sqrt(t) * np.exp(-((k - 1.0) / (vol * np.sqrt(t))) ** 2)
    market = spots[:, None] * level * (1.0 + 0.02 * rs.randn(B, 15))
    assert np.all(market > 0)
    return market, spots


def random_model(widths, seed=0, first_scale=1.0):
    """A model of ``widths`` on the documented eleven features: weights N(0, 2 / in) (He), biases
    N(0, 0.1^2), as float32; the input statistics those of ``markets(512)``'s features, the
    output statistics of the generator's order of magnitude.  first_scale multiplies the first
    layer's weights and bias (1e-39: its activations are float32 subnormals)."""
    from dhcos.ffn import FFNModel, price_features
    assert widths[0] == 11 and widths[-1] == 13
    rs = np.random.RandomState(seed)
    C_mat, names = price_features([90, 95, 100, 105, 110], [0.25, 0.5, 1.0])
    mkt, sp = markets(512, seed=99)
    f = (mkt @ C_mat.T) / sp[:, None]
    Ws, bs = [], []
    for l, (i, o) in enumerate(zip(widths[:-1], widths[1:])):
        scale = first_scale if l == 0 else 1.0
        Ws.append((scale * np.sqrt(2.0 / i) * rs.randn(o, i)).astype(np.float32))
        bs.append((scale * 0.1 * rs.randn(o)).astype(np.float32))
    y_mean = rs.uniform(-3.0, 0.5, 13)
    y_std = rs.uniform(0.1, 0.5, 13)
    return FFNModel(C_mat, f.mean(axis=0), f.std(axis=0), y_mean, y_std, Ws, bs, names)


def integer_model(widths, seed=0):
    """Exact-integer data: C the identity on 11 'prices', no standardisation (mean 0, std 1, both
    ways), integer weights in [-2, 2] (asymmetric: drawn at random and checked), biases 0 or 1.
    With integer prices in [1, 4] and S0 = 1 every partial sum is an integer of magnitude at most
    11 * 4 * 2 + 1 = 89, then 64 * 89 * 2 + 1, then 32 * 11393 * 2 + 1 < 2^24."""
    from dhcos.ffn import FFNModel
    rs = np.random.RandomState(seed)
    Ws, bs = [], []
    for i, o in zip(widths[:-1], widths[1:]):
        W = rs.randint(-2, 3, size=(o, i))
        n = min(o, i)
        assert not np.array_equal(W[:n, :n], W[:n, :n].T)
        Ws.append(W.astype(np.float32))
        bs.append(rs.randint(0, 2, size=o).astype(np.float32))
    F = widths[0]
    return FFNModel(np.eye(F), np.zeros(F), np.ones(F), np.zeros(13), np.ones(13), Ws, bs)


def integer_forward(model, prices):
    """NumPy int64 arithmetic of an integer model on integer prices [B, F] (S0 = 1)."""
    a = np.asarray(prices, dtype=np.int64)
    for l, (W, b) in enumerate(zip(model.weights, model.biases)):
        a = a @ W.astype(np.int64).T + b.astype(np.int64)
        assert np.abs(a).max() < 2 ** 24
        if l + 1 < len(model.weights):
            a = np.maximum(a, 0)
    return a


def gamma(K):
    return K * U32 / (1.0 - K * U32)


def forward_bound(model, market, spots):
    """-> (x0 truth [B, 13], bound [B, 13]): FFNModel.forward_reference and the bar derived in
    this module's docstring."""
    z = (model.input_features(market, spots) - model.x_mean) / model.x_std
    a = z
    delta = U32 * np.abs(z)
    n = len(model.weights)
    for l, (W, b) in enumerate(zip(model.weights, model.biases)):
        W64, b64 = W.astype(np.float64), b.astype(np.float64)
        K = W.shape[1]
        aW = np.abs(W64)
        delta = delta @ aW.T + gamma(K + 1) * (np.abs(b64) + (np.abs(a) + delta) @ aW.T)
        a = a @ W64.T + b64
        if l + 1 < n:
            a = np.maximum(a, 0.0)
    x0 = model.y_mean + model.y_std * a
    bound = (np.abs(model.y_std) * delta
             + 4.0 * 2.0 ** -52 * (np.abs(model.y_mean) + np.abs(model.y_std * a)))
    return x0, bound
