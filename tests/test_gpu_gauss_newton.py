"""GPU tests of the Gauss-Newton rows reduction (csrc/dh_gauss_newton.h:
dh_surface_gauss_newton_rows*, Surface.gauss_newton_rows*), at M = 15 (one pass), 64
(a full wave), 65 (a one-lane tail) and 130 (three passes), two markets, S = 5:

  1. f, g and n_bad are Surface.loss_grad_rows's bits;
  2. H is exactly symmetric;
  3. H against the sum over the device's own planes (Surface.param_sens), each entry to
         2 (ceil(M / 64) + 6 + 4) 2^-53 (2 / M) |dt_i dt_j| sum_m |a_im a_jm|:
     the additions on the longest path of the lane sums and the butterfly plus the roundings of the
     two quotients, the product and the three scalings, doubled.  The reference is the exactly
     rounded sum (math.fsum) of NumPy's products.  This bar holds where the records the planes are
     taken at are the device's own: sets 0 and 1 have x_i = 0 wherever the transform is exp or tanh
     (exp(0) = 1 and tanh(0) = 0 exactly on any libm) and differ in mu_j, market, spot and rate.
     Sets 2 and 3 are generator-range parameters, whose host records may differ from the device's by
     an ulp of exp: they are held to tests/test_gpu_param_grad.py's loss bar, 1e-9 of the same sum;
  4. the bits do not depend on S, on the order of the sets, or on the _dev against the host form;
  5. an invalid set gives 1e10 / 0 / 0 and a NaN market price NaN."""
import math

import numpy as np
import pytest

from oracle import dh_oracle as O

pytestmark = pytest.mark.gpu

LO = np.array([0.025, 1.5, 0.025, 0.2, -0.85, 0.02, 0.3, 0.025, 0.1, -0.7, 0.05, -0.08, 0.03])
HI = np.array([0.08, 4.5, 0.065, 0.5, -0.4, 0.07, 1.2, 0.07, 0.35, -0.2, 0.25, -0.01, 0.12])
N = 128
GRIDS = {15: None, 64: (8, 8), 65: (13, 5), 130: (13, 10)}


@pytest.fixture(scope="module")
def native():
    from dhcos import _native
    if _native.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return _native


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def make_surface(native, M):
    from dhcos.generator import MATURITIES, STRIKES_PCT
    ctx = native.default_context()
    if M == 15:
        k, t = np.asarray(STRIKES_PCT, dtype=np.float64), np.asarray(MATURITIES, dtype=np.float64)
        mode = native.STRIKE_PCT_SPOT
    else:
        nk, nt = GRIDS[M]
        k, t, mode = np.linspace(82.0, 118.0, nk), np.linspace(0.2, 2.0, nt), native.STRIKE_ABSOLUTE
    Kg, Tg = np.tile(k, t.size), np.repeat(t, k.size)
    assert Kg.size == M
    return native.Surface(ctx, Kg, Tg, np.ones(M, dtype=bool), strike_mode=mode), ctx


def inputs(surf, M):
    rs = np.random.RandomState(100 + M)
    spots, rates = np.array([97.0, 103.5]), np.array([0.02, 0.04])
    row = np.array([0, 1, 1, 0, 1], dtype=np.int32)
    X = np.zeros((5, 13))
    X[0, 11], X[1, 11] = -0.05, -0.02                   # exact records: 1, 0 and mu_j itself
    X[2] = O.from_params(LO + (HI - LO) * rs.rand(13))
    X[3] = O.from_params(LO + (HI - LO) * rs.rand(13))
    X[4] = 5.0                                          # NaN prices: an invalid set
    base = np.zeros((2, 16))
    base[:, :13] = LO + (HI - LO) * rs.rand(2, 13)
    base[:, 13], base[:, 14] = spots, rates
    mkt = surf.price(base, N) * (1 + 0.02 * rs.randn(2, M))
    return X, mkt, spots, rates, row


def records(X, spots, rates, row):
    from dhcos.calibrator import x_to_model
    rec = np.zeros((X.shape[0], 16))
    rec[:, :13] = x_to_model(X)
    rec[:, 13], rec[:, 14] = spots[row], rates[row]
    return rec


def hessian_reference(planes, rec, mkt_rows, M):
    """-> (H [S, 13, 13] with exactly rounded sums, the bar's sum (2 / M) |dt dt| sum |a a|)."""
    S = rec.shape[0]
    H, mag = np.zeros((S, 13, 13)), np.zeros((S, 13, 13))
    for s in range(S):
        a = planes[1:, s, :] / mkt_rows[s][None, :]
        dt = rec[s, :13].copy()
        dt[[4, 9]] = 1.0 - rec[s, [4, 9]] ** 2
        dt[11] = 1.0
        for i in range(13):
            for j in range(13):
                prod = a[i] * a[j]
                H[s, i, j] = (2.0 / M) * dt[i] * dt[j] * math.fsum(prod)
                mag[s, i, j] = (2.0 / M) * abs(dt[i] * dt[j]) * math.fsum(np.abs(prod))
    return H, mag


@pytest.mark.parametrize("M", [15, 64, 65, 130])
def test_gauss_newton_rows(native, M):
    import torch
    surf, ctx = make_surface(native, M)
    try:
        X, mkt, spots, rates, row = inputs(surf, M)
        S = X.shape[0]
        want = surf.loss_grad_rows(X, mkt, spots, rates, row, N)
        f, g, bad, H = surf.gauss_newton_rows(X, mkt, spots, rates, row, N)
        rec = records(X, spots, rates, row)
        planes = surf.param_sens(rec, N)
        # any S, any order: permuted with set 2 twice, and set 3 alone against its market as row 0
        perm = np.array([3, 0, 2, 4, 1, 2])
        fp, gp, bp, Hp = surf.gauss_newton_rows(X[perm], mkt, spots, rates, row[perm], N)
        f1, g1, b1, H1 = surf.gauss_newton_rows(X[3:4], mkt[0:1], spots[0:1], rates[0:1], [0], N)
        # the device-pointer form
        dev = torch.device("cuda", ctx.device)
        d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (X, mkt, spots, rates, row)]
        d_f = torch.empty(S, dtype=torch.float64, device=dev)
        d_g = torch.empty((S, 13), dtype=torch.float64, device=dev)
        d_bad = torch.empty(S, dtype=torch.int32, device=dev)
        d_H = torch.empty((S, 13, 13), dtype=torch.float64, device=dev)
        stream = torch.cuda.Stream(device=dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream):
            surf.gauss_newton_rows_dev(*(a.data_ptr() for a in d), S, d_f.data_ptr(),
                                       d_g.data_ptr(), d_bad.data_ptr(), d_H.data_ptr(), N=N,
                                       stream=stream.cuda_stream)
        stream.synchronize()
        # a NaN market price in market 1
        bad_mkt = mkt.copy()
        bad_mkt[1, M // 2] = np.nan
        fn, gn, bn, Hn = surf.gauss_newton_rows(X[:2], bad_mkt, spots, rates, row[:2], N)
        wn = surf.loss_grad_rows(X[:2], bad_mkt, spots, rates, row[:2], N)
        with pytest.raises(native.NativeError):
            surf.gauss_newton_rows(X, mkt, spots, rates, np.full(S, 2, dtype=np.int32), N)
    finally:
        surf.close()
    # 1. loss_grad_rows's bits
    assert same_bits(f, want[0]) and same_bits(g, want[1]) and np.array_equal(bad, want[2])
    assert np.array_equal(bad, [0, 0, 0, 0, M])
    # 2. symmetric, and 5. the invalid set
    assert same_bits(H, np.transpose(H, (0, 2, 1)))
    assert f[4] == 1e10 and not g[4].any() and not H[4].any() and np.signbit(H[4]).sum() == 0
    assert np.all(np.isfinite(H[:4])) and np.all(np.einsum("sii->si", H[:4]) > 0.0)
    # 3. against the device's own planes
    ref, mag = hessian_reference(planes[:, :4], rec[:4], mkt[row[:4]], M)
    eps = 2.0 ** -53
    tight = 2.0 * (math.ceil(M / 64) + 6 + 4) * eps * mag
    err = np.abs(H[:4] - ref)
    print(f"M {M}: exact-record sets worst err / bar {np.max(err[:2] / tight[:2]):.3f}; "
          f"generator-range sets worst err / (1e-9 sum) {np.max(err[2:] / (1e-9 * mag[2:])):.3e}")
    assert np.all(err[:2] <= tight[:2])
    assert np.all(err[2:] <= 1e-9 * mag[2:])
    assert not same_bits(H[0], H[1]) and not same_bits(H[2], H[3])
    # 4. independent of S, order and form
    assert same_bits(fp, f[perm]) and same_bits(gp, g[perm]) and np.array_equal(bp, bad[perm])
    assert same_bits(Hp, H[perm])
    assert f1[0] == f[3] and same_bits(g1[0], g[3]) and same_bits(H1[0], H[3]) and b1[0] == 0
    assert same_bits(d_f.cpu().numpy(), f) and same_bits(d_g.cpu().numpy(), g)
    assert same_bits(d_H.cpu().numpy(), H) and np.array_equal(d_bad.cpu().numpy(), bad)
    # 5. NaN market price: NaN where loss_grad_rows gives NaN, market 0's set untouched
    assert np.isnan(wn[0][1]) and np.isnan(fn[1]) and np.all(np.isnan(gn[1]))
    assert np.all(np.isnan(Hn[1])) and bn[1] == 0
    assert fn[0] == f[0] and same_bits(Hn[0], H[0])
