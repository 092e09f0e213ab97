"""Price and loss requests through the fused and the split path on the smallest surfaces that take
each index path of the tile sums (csrc/dh_index.h; N = 128, 2 param sets per case): both paths
bitwise equal, and every price within the 1e-10 bar of the oracle.

Maturity-group sizes per case (one tile per group; a launch's options per lane group follow its
largest tile):
* (3,), (5, 5, 5): one option per lane group (C1's shape), in-wave butterflies;
* (32, 32): C2's tile, one option per lane group on 8 lanes;
* (100, 100): block-wide tiles, 4 options per group on G = 10 lanes, reduced through LDS;
* (101,): a prime option count: 26 groups, the last of one option, G = 9;
* (3, 5, 100): 4 options per group with a tile of fewer than 4 options and one whose count is no
  multiple of 4.
"""
import numpy as np
import pytest

from conftest import rel_close
from oracle import dh_oracle as O

pytestmark = pytest.mark.gpu

N = 128
S0, R = 100.0, 0.03
CASES = [(3,), (5, 5, 5), (32, 32), (100, 100), (101,), (3, 5, 100)]


@pytest.fixture(scope="module")
def native():
    from dhcos import _native
    if _native.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return _native


def _case(groups, seed):
    rs = np.random.RandomState(seed)
    lo = np.array([0.025, 1.5, 0.025, 0.2, -0.85, 0.02, 0.3, 0.025, 0.1, -0.7, 0.05, -0.08, 0.03])
    hi = np.array([0.08, 4.5, 0.065, 0.5, -0.4, 0.07, 1.2, 0.07, 0.35, -0.2, 0.25, -0.01, 0.12])
    params = lo + (hi - lo) * rs.rand(2, 13)
    Ts = np.linspace(0.25, 1.5, len(groups)) if len(groups) > 1 else np.array([0.75])
    T = np.repeat(Ts, groups)
    M = T.size
    K = S0 * rs.uniform(0.8, 1.2, M)
    call = rs.rand(M) < 0.5
    rec = np.empty((2, 16))
    rec[:, :13], rec[:, 13], rec[:, 14], rec[:, 15] = params, S0, R, 0.0
    return params, rec, K, T, call


def _with_path(ctx, path, fn):
    ctx.set_path(path)
    try:
        return fn()
    finally:
        ctx.set_path(0)


@pytest.mark.parametrize("groups", CASES, ids=lambda g: "x".join(map(str, g)))
def test_index_paths_fused_equals_split_and_oracle(native, groups):
    params, rec, K, T, call = _case(groups, 60 + len(groups) + groups[0])
    want = np.stack([O.price_many(params[p], S0, K, T, R, call, N) for p in range(2)])
    ctx = native.default_context()
    surf = native.Surface(ctx, K, T, call, np.abs(want[0]) + 1e-3)
    res = {}
    for path in (native.PATH_SPLIT, native.PATH_FUSED):
        pr = _with_path(ctx, path, lambda: surf.price(rec, N))
        assert ctx.last_path == path
        sse, bad, lp = _with_path(ctx, path, lambda: surf.loss_terms(rec, N, want_prices=True))
        sse0, bad0, _ = _with_path(ctx, path, lambda: surf.loss_terms(rec, N))   # no price columns
        res[path] = (pr, sse, bad, lp, sse0, bad0)
    s, f = res[native.PATH_SPLIT], res[native.PATH_FUSED]
    for a, b in zip(s, f):
        assert np.array_equal(a, b), np.max(np.abs(np.asarray(a, float) - np.asarray(b, float)))
    assert np.array_equal(f[0], f[3])
    err = np.max(np.abs(f[0] - want) / (1e-10 * np.abs(want) + 1e-10))
    print(f"groups {groups}: max error / bar {err:.3g}")
    assert rel_close(f[0], want, 1e-10, 1e-10).all(), err
