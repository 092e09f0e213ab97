"""CPU-side checks of the implied-volatility feature: the invariants of the truth fixture
(tests/golden/iv_truth.npz, written by tests/golden/make_iv_truth.py) and the C-ABI boundary of
dh_implied_vol, dh_implied_vol_dev and dh_surface_implied_vol without a device."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

EPS = float(np.finfo(np.float64).eps)


@pytest.fixture(scope="module")
def truth():
    with np.load(os.path.join(GOLDEN, "iv_truth.npz")) as z:
        return {k: z[k] for k in z.files}


def test_fixture_invariants(truth):
    t = truth
    n = t["price"].size
    assert n == 1250
    for k in ("S0", "K", "T", "r", "q", "is_call", "sigma_true", "vega", "lower", "scale", "keep"):
        assert t[k].shape == (n,), k
    assert np.all(t["S0"] == 100.0) and np.all(t["K"] > 0) and np.all(t["sigma_true"] > 0)
    assert set(np.unique(t["T"])) == {0.1, 1.0, 2.0}
    assert set(np.unique(t["r"])) == {0.0, 0.03, 0.05} and set(np.unique(t["q"])) == {0.0, 0.02}
    s = t["sigma_true"] * np.sqrt(t["T"])
    assert np.isclose(s.min(), 1e-3) and np.isclose(s.max(), 4.0)
    # a call and a put at every point
    assert np.all(t["is_call"][0::2] == 1) and np.all(t["is_call"][1::2] == 0)
    for k in ("S0", "K", "T", "r", "q", "sigma_true"):
        assert np.array_equal(t[k][0::2], t[k][1::2]), k
    # the bounds and the scale as the library forms them in fp64
    A = t["S0"] * np.exp(-t["q"] * t["T"])
    B = t["K"] * np.exp(-t["r"] * t["T"])
    lower = np.where(t["is_call"] != 0, np.maximum(A - B, 0.0), np.maximum(B - A, 0.0))
    assert np.array_equal(lower, t["lower"])
    scale = np.where(lower == 0.0, t["price"], np.maximum(t["price"], np.maximum(A, B)))
    assert np.array_equal(scale, t["scale"])
    keep = t["price"] - lower >= 1000.0 * EPS * scale
    assert np.array_equal(keep, t["keep"])
    assert keep.mean() >= 0.8
    assert np.all(keep[lower == 0.0])                 # every out-of-the-money quote is kept
    assert np.all(t["vega"][keep] > 0) and np.all(np.isfinite(t["price"]))
    assert np.isfinite(t["yardstick"]) and t["yardstick"] >= 1.0


def test_implied_vol_arguments_are_rejected():
    """Null and negative arguments give DH_E_ARG before any device work."""
    from dhcos import _native
    lib = _native.load()
    a = np.ones(4)
    ic = np.ones(4, dtype=np.int8)
    p, c = a.ctypes.data, ic.ctypes.data
    assert lib.dh_implied_vol(None, p, p, p, p, p, p, c, 4, p) == -1
    assert b"null" in lib.dh_last_error()
    assert lib.dh_implied_vol(None, None, None, None, None, None, None, None, 4, None) == -1
    assert lib.dh_implied_vol(None, p, p, p, p, p, p, c, -1, p) == -1
    assert lib.dh_implied_vol_dev(None, p, p, p, p, p, p, c, 4, p, None) == -1
    assert lib.dh_implied_vol_dev(None, None, None, None, None, None, None, None, -1, None,
                                  None) == -1
    assert lib.dh_surface_implied_vol(None, None, None, 1, 128, 10.0, None, None) == -1
    assert b"null" in lib.dh_last_error()


def test_implied_vol_fails_loudly_without_device():
    import dhcos
    from dhcos import DoubleHeston, NativeError, _native
    if _native.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(NativeError):
        dhcos.implied_vol(10.45, 100.0, 100.0, 1.0, 0.05)
    dh = DoubleHeston(100, 100, 1.0, 0.05, 0.04, 2.0, 0.04, 0.3, -0.5, 0.04, 1.5, 0.04, 0.2, -0.3,
                      0.5, -0.05, 0.1)
    with pytest.raises(NativeError):
        dh.implied_vol()
    with pytest.raises(NativeError):
        DoubleHeston.implied_vol_batch([[0.04, 2.0, 0.04, 0.3, -0.5, 0.04, 1.5, 0.04, 0.2, -0.3,
                                         0.5, -0.05, 0.1]], 100.0, [90.0, 110.0], 1.0, 0.05)


def test_generator_flag_needs_arrays():
    """implied_vols=True with the pickled records raises before any work."""
    from dhcos import generate_synthetic_calibrations
    with pytest.raises(ValueError):
        generate_synthetic_calibrations(3, None, as_arrays=False, implied_vols=True, verbose=False)
