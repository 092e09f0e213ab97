"""NumPy restatement of the price objective and its analytic gradient against a market row per
set (dh_surface_loss_grad_rows): tests/param_grad_reference.py's loss_grad called
per set with that set's market prices, spot and rate.  With one market it is loss_grad itself."""
import numpy as np

import param_grad_reference as R


def market_of_row(K, T, is_call, prices):
    """One market row as loss_grad's option dicts: absolute strikes K [M], maturities T [M], flags
    [M] and market prices [M]."""
    return [{"strike": float(k), "maturity": float(t), "price": float(p),
             "option_type": "call" if c else "put"} for k, t, c, p in zip(K, T, is_call, prices)]


def loss_grad_rows(X, markets, spots, rates, row, N=128):
    """(f [S], g [S, 13]) of the points X [S, 13]: set s against markets[row[s]] (a list of option
    dicts per market) under spots[row[s]] and rates[row[s]]; 1e10 and zeros for an invalid set."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 13)
    f, g = np.empty(len(X)), np.empty((len(X), 13))
    for s, x in enumerate(X):
        b = int(row[s])
        f[s], g[s] = R.loss_grad(x, markets[b], float(spots[b]), float(rates[b]), N)
    return f, g
