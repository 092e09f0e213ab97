"""CPU tests of the warm-start network (dhcos/ffn.py, csrc/dh_ffn.h's host twin).

  1. price_features on the generator's 5 x 3 grid: eleven rows, entry by entry; F = 3 n_T + 2;
  2. the BatchNorm fold in float64 against torch's own .double().eval() forward, to 1e-12 of each
     output's absolute term sum; save / load round trip; pickled content refused;
  3. the host twin (tests/native/libffnhost.so: the kernel's prologue and epilogue and a plain
     fmaf chain per neuron) against the float64 truth, within the forward error bound derived in
     tests/ffn_reference.py -- and the two injected slips (a transposed W, a dropped bias), applied
     to the twin's copy of the weights, each miss that bound;
  4. train_ffn learns a random linear map (validation MSE < 0.25 in standardised units; the mean
     predictor scores 1.0) and repeats itself under one seed; init= starts from the model's own
     function, improves a half-trained model at the documented stage-2 settings, and never returns
     a model whose validation loss is above its starting value; fine_tune_ffn on a
     calibration result;
  5. predict's argument errors are raised without a device.
"""
import numpy as np
import pytest

import ffn_reference as R


# ---- 1. features ---------------------------------------------------------------------------------

def test_price_features_on_the_generator_grid():
    from dhcos.ffn import price_features
    C, names = price_features([90, 95, 100, 105, 110], [0.25, 0.5, 1.0])
    assert C.shape == (11, 15) and C.dtype == np.float64 and len(names) == 11
    want = np.zeros((11, 15))
    for i in range(3):
        lo, atm, hi = 5 * i, 5 * i + 2, 5 * i + 4
        want[3 * i, atm] = 1.0                                   # ATM price
        want[3 * i + 1, hi], want[3 * i + 1, lo] = 1.0, -1.0     # skew
        want[3 * i + 2, lo] = want[3 * i + 2, hi] = 1.0          # convexity
        want[3 * i + 2, atm] = -2.0
    want[9, 12], want[9, 2] = 1.0, -1.0                          # term slope
    want[10, [2, 7, 12]] = 1.0                                   # sum of the ATM prices
    assert np.array_equal(C, want)
    p = np.arange(1.0, 16.0) ** 1.5
    f = C @ p
    assert f[0] == p[2] and f[1] == p[4] - p[0] and f[2] == p[0] + p[4] - 2 * p[2]
    assert f[9] == p[12] - p[2] and f[10] == p[2] + p[7] + p[12]


def test_price_features_on_other_grids():
    from dhcos.ffn import price_features
    C, names = price_features([97, 104, 99], [0.5, 2.0])        # ATM is the strike nearest 100
    assert C.shape == (3 * 2 + 2, 6) and len(names) == 8
    assert np.array_equal(C[0], [0, 0, 1, 0, 0, 0])              # ATM(T0) = the 99 % strike
    assert np.array_equal(C[1], [-1, 1, 0, 0, 0, 0])             # highest (104) - lowest (97)
    assert np.array_equal(C[6], [0, 0, -1, 0, 0, 1])
    with pytest.raises(ValueError):
        price_features([], [1.0])


# ---- 2. fold, files ------------------------------------------------------------------------------

def trained_stack():
    import torch
    from dhcos.ffn import build_stack
    torch.manual_seed(3)
    net = build_stack((11, 64, 32, 13), dropout=0.1)
    opt = torch.optim.Adam(net.parameters(), lr=1e-2)
    x = 2.0 + 3.0 * torch.randn(512, 11)
    y = torch.randn(512, 13)
    net.train()
    for i in range(0, 512, 64):                     # a few steps: non-trivial BatchNorm statistics
        opt.zero_grad()
        torch.nn.functional.mse_loss(net(x[i:i + 64]), y[i:i + 64]).backward()
        opt.step()
    return net, x


def test_fold_matches_torch_double_eval():
    import torch
    from dhcos.ffn import fold_batchnorm, mlp_forward
    net, x = trained_stack()
    bn = [m for m in net if isinstance(m, torch.nn.BatchNorm1d)]
    assert all(float(m.running_mean.abs().max()) > 1e-3 for m in bn)
    assert all(float((m.running_var - 1).abs().max()) > 1e-3 for m in bn)
    Ws, bs = fold_batchnorm(net)
    assert all(w.dtype == np.float64 for w in Ws)
    z = x[:64].double().numpy()
    with torch.no_grad():
        want = net.double().eval()(torch.from_numpy(z)).numpy()
    got = mlp_forward(Ws, bs, z)
    # each output's absolute term sum: |b| + |W| |a| of the last layer
    a = z
    for W, b in zip(Ws[:-1], bs[:-1]):
        a = np.maximum(a @ W.T + b, 0.0)
    scale = np.abs(bs[-1]) + np.abs(a) @ np.abs(Ws[-1]).T
    err = np.abs(got - want) / scale
    print("fold: max error / term sum", err.max())
    assert err.max() <= 1e-12


def test_save_load_round_trip_and_pickle_refused(tmp_path):
    from dhcos.ffn import FFNModel
    m = R.random_model(R.WIDTH_SETS[1], seed=4)
    path = tmp_path / "m.npz"
    m.save(path)
    got = FFNModel.load(path)
    assert got.widths == m.widths and got.feature_names == m.feature_names
    for name in ("features", "x_mean", "x_std", "y_mean", "y_std"):
        assert np.array_equal(getattr(got, name), getattr(m, name)), name
    for a, b in zip(got.weights + got.biases, m.weights + m.biases):
        assert a.dtype == np.float32 and np.array_equal(a, b)
    # the same file with one object (pickled) entry is refused
    with np.load(path) as z:
        arrays = {k: z[k] for k in z.files}
    arrays["W0"] = np.array([{"not": "an array"}], dtype=object)
    bad = tmp_path / "bad.npz"
    np.savez(bad, **arrays)
    with pytest.raises(ValueError):
        FFNModel.load(bad)


def test_model_shape_rules():
    from dhcos.ffn import FFNModel
    m = R.random_model(R.WIDTH_SETS[0])
    args = (m.features, m.x_mean, m.x_std, m.y_mean, m.y_std)
    with pytest.raises(ValueError):                 # a hidden width that is no multiple of 32
        FFNModel(*args, [np.zeros((40, 11), np.float32), np.zeros((13, 40), np.float32)],
                 [np.zeros(40, np.float32), np.zeros(13, np.float32)])
    with pytest.raises(ValueError):                 # no hidden layer
        FFNModel(*args, [np.zeros((13, 11), np.float32)], [np.zeros(13, np.float32)])
    with pytest.raises(ValueError):                 # x_std of zero
        FFNModel(m.features, m.x_mean, np.zeros(11), m.y_mean, m.y_std, m.weights, m.biases)


# ---- 3. the host twin against the truth ----------------------------------------------------------

@pytest.fixture(scope="module")
def tail_markets():
    return R.markets(R.BATCHES[-1])


@pytest.mark.parametrize("widths", R.WIDTH_SETS, ids=lambda w: "x".join(map(str, w)))
def test_host_twin_within_the_derived_bound(widths, tail_markets):
    model = R.random_model(widths, seed=len(widths))
    mkt, sp = tail_markets
    truth, bound = R.forward_bound(model, mkt, sp)
    assert np.allclose(truth, model.forward_reference(mkt, sp), rtol=1e-14, atol=0)
    x0, raw = R.twin_forward(model, mkt, sp)
    err = np.abs(x0 - truth)
    print(f"{widths}: max |x0 - truth| {err.max():.3e}, max bound {bound.max():.3e}, "
          f"max ratio {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
    # x0 is the epilogue's one fma of the twin's float32 output
    ref = model.y_std * raw.astype(np.float64) + model.y_mean
    assert np.all(np.abs(x0 - ref) <= 2.0 ** -52 * (np.abs(model.y_mean) + np.abs(ref)))
    # the injected slips, on the twin's copy of the weights: each misses the bound
    # (the chains started from zero, as a kernel that forgot the bias would start them)
    slips = {"dropped bias": (model.weights, [np.zeros_like(b) for b in model.biases])}
    # a transposed W keeps its shape only where it is square: transpose the leading square block
    l, W = max(enumerate(model.weights), key=lambda e: min(e[1].shape))
    n = min(W.shape)
    Wt = W.copy()
    Wt[:n, :n] = W[:n, :n].T
    slips["transposed W"] = ([Wt if i == l else w for i, w in enumerate(model.weights)],
                             model.biases)
    for name, (Ws, bs) in slips.items():
        bad, _ = R.twin_forward(model, mkt, sp, Ws, bs)
        miss = np.abs(bad - truth) > bound
        print(f"{widths}: {name}: {miss.mean():.0%} of the outputs miss the bound")
        assert miss.any(), name
        if len(widths) <= 4:           # the bound is sharp on the shallow networks
            assert miss.mean() > 0.5, name


# ---- 4. training ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def linear_task():
    rs = np.random.RandomState(11)
    X = rs.randn(2048, 11)
    A = rs.randn(11, 13) / np.sqrt(11)
    return X, X @ A + 0.3 * rs.randn(13)


def test_training_learns_and_repeats(linear_task):
    from dhcos.ffn import train_ffn
    X, Y = linear_task
    kw = dict(widths=(32,), epochs=60, seed=0, device="cpu")
    model, hist = train_ffn(X, Y, **kw)
    print("validation MSE", hist["best_val"], "best epoch", hist["best_epoch"],
          "epochs run", len(hist["val"]))
    assert model.widths == (11, 32, 13)
    assert all(w.dtype == np.float32 for w in model.weights + model.biases)
    assert hist["best_val"] < 0.25
    # the exported (folded, float32) model scores the same on the held-out rows
    order = np.random.RandomState(0).permutation(2048)
    va = order[-int(round(2048 * 0.15)):]
    from dhcos.ffn import mlp_forward
    raw = mlp_forward(model.weights, model.biases, (X[va] - model.x_mean) / model.x_std)
    mse = np.mean((raw - (Y[va] - model.y_mean) / model.y_std) ** 2)
    assert abs(mse - hist["best_val"]) < 1e-3 * max(hist["best_val"], 1e-3) + 1e-5
    again, hist2 = train_ffn(X, Y, **kw)
    assert hist2["val"] == hist["val"]
    for a, b in zip(again.weights + again.biases, model.weights + model.biases):
        assert np.array_equal(a, b)


def test_init_continues_from_the_models_function_and_improves(linear_task):
    """Stage 2 at the documented settings (lr=1e-5, batch_size=32) on a half-trained model: the
    starting state is the model's own function -- in evaluation mode and, through the BatchNorm
    statistics it starts from, in training mode -- so the first epochs go down from the model's
    loss instead of re-normalising it into another network, and the result is a strictly better
    model, not the input handed back."""
    from dhcos.ffn import train_ffn
    X, Y = linear_task
    model, hist = train_ffn(X, Y, widths=(32,), epochs=3, seed=0, device="cpu")
    cont, h2 = train_ffn(X, Y, init=model, lr=1e-5, batch_size=32, epochs=10, patience=10, seed=0,
                         device="cpu")
    print("stage 1", hist["best_val"], "stage 2 from", h2["initial_val"], "->", h2["val"])
    assert cont.widths == model.widths
    assert np.array_equal(cont.x_mean, model.x_mean) and np.array_equal(cont.y_std, model.y_std)
    # the starting state is the model's own evaluation: same split, same loss as stage 1 ended on
    assert abs(h2["initial_val"] - hist["best_val"]) <= 1e-5 * hist["best_val"] + 1e-6
    # the first epoch stays at the model's loss: training mode did not change the function
    # (identity BatchNorm statistics moved it by tens of percent)
    assert abs(h2["val"][0] - h2["initial_val"]) < 0.05 * h2["initial_val"]
    assert h2["best_epoch"] > 0 and h2["best_val"] < h2["initial_val"]
    assert any(not np.array_equal(a, b) for a, b in zip(cont.weights, model.weights))


def test_init_never_ends_above_its_start(linear_task):
    """A learning rate that wrecks the model: the starting state is kept."""
    from dhcos.ffn import train_ffn
    X, Y = linear_task
    model, hist = train_ffn(X, Y, widths=(32,), epochs=30, seed=0, device="cpu")
    cont, h2 = train_ffn(X, Y, init=model, lr=3.0, batch_size=32, epochs=3, patience=3, seed=0,
                         device="cpu")
    assert h2["best_val"] <= h2["initial_val"]
    if h2["best_epoch"] == 0:
        for a, b in zip(cont.weights + cont.biases, model.weights + model.biases):
            assert np.allclose(a, b, rtol=1e-5, atol=1e-6)


def test_fine_tune_on_a_calibration_result():
    """fine_tune_ffn on a BatchCalibrationResult-shaped object whose x is the first stage's target
    shifted: the successful markets alone are used (the others carry NaN, which train_ffn would
    refuse), the model keeps its features, grid and standardisation, and stage 2 at its default
    (documented) settings ends strictly below where it started."""
    from types import SimpleNamespace
    from dhcos.ffn import fine_tune_ffn, price_features, train_ffn
    grid = ([90, 95, 100, 105, 110], [0.25, 0.5, 1.0])
    C, names = price_features(*grid)
    mkt, sp = R.markets(1024, seed=3)
    f = (mkt @ C.T) / sp[:, None]
    rs = np.random.RandomState(4)
    z = (f - f.mean(axis=0)) / f.std(axis=0)
    target = z @ (rs.randn(11, 13) / np.sqrt(11)) + rs.randn(13)
    model, _ = train_ffn(f, target, widths=(32,), epochs=20, seed=0, device="cpu",
                         feature_matrix=C, feature_names=names, grid=grid)
    ok = rs.rand(1024) > 0.1
    x = np.where(ok[:, None], target + 0.5 * target.std(axis=0), np.nan)
    result = SimpleNamespace(success=ok, market_prices=mkt, spots=sp, x=x)
    tuned, h = fine_tune_ffn(model, result, epochs=8, seed=0, device="cpu")
    print("fine tune from", h["initial_val"], "->", h["val"])
    assert h["best_epoch"] > 0 and h["best_val"] < h["initial_val"]
    assert np.array_equal(tuned.features, model.features) and tuned.feature_names == names
    assert all(np.array_equal(a, b) for a, b in zip(tuned.grid, model.grid))
    assert np.array_equal(tuned.y_mean, model.y_mean)
    with pytest.raises(ValueError):
        fine_tune_ffn(model, SimpleNamespace(success=np.zeros(1024, bool), market_prices=mkt,
                                             spots=sp, x=x))


# ---- 5. argument errors --------------------------------------------------------------------------

def test_predict_argument_errors_need_no_device():
    model = R.random_model(R.WIDTH_SETS[0])
    mkt, sp = R.markets(4)
    for bad_mkt, bad_sp in [(mkt[:, :14], sp), (mkt, sp[:3]), (mkt.reshape(-1), sp)]:
        with pytest.raises(ValueError):
            model.predict(bad_mkt, bad_sp)
    for v in (np.nan, np.inf, 0.0, -1.0):
        m2 = mkt.copy()
        m2[2, 7] = v
        with pytest.raises(ValueError):
            model.predict(m2, sp)
        with pytest.raises(ValueError):
            model.predict_parameters(m2, sp)
    for v in (0.0, -100.0, np.nan):
        s2 = sp.copy()
        s2[1] = v
        with pytest.raises(ValueError):
            model.predict(mkt, s2)


def test_calibrate_batch_checks_the_models_inputs_before_the_device():
    from dhcos import calibrate_batch
    model = R.random_model(R.WIDTH_SETS[0])
    mkt, sp = R.markets(3)
    mkt[1, 0] = -1.0
    with pytest.raises(ValueError):
        calibrate_batch(mkt, sp, 0.03, x0s=model, maxiter=1)


def test_calibrate_batch_refuses_another_grid_than_the_models():
    """A model that carries its grid is not fed prices of another one with the same M."""
    from dhcos import calibrate_batch
    from dhcos.ffn import FFNModel
    m = R.random_model(R.WIDTH_SETS[0])
    assert m.grid is None                                   # the grid is the caller's promise
    g = FFNModel(m.features, m.x_mean, m.x_std, m.y_mean, m.y_std, m.weights, m.biases,
                 m.feature_names, grid=([90, 95, 100, 105, 110], [0.25, 0.5, 1.0]))
    mkt, sp = R.markets(3)
    for kw in (dict(strikes_pct=[80, 90, 100, 110, 120]), dict(maturities=[0.5, 1.0, 2.0]),
               dict(strikes=[90.0, 95.0, 100.0, 105.0, 110.0]), dict(is_call=False)):
        with pytest.raises(ValueError, match="grid"):
            calibrate_batch(mkt, sp, 0.03, x0s=g, maxiter=1, **kw)
    with pytest.raises(ValueError):                         # 14 options: not the model's
        FFNModel(m.features, m.x_mean, m.x_std, m.y_mean, m.y_std, m.weights, m.biases,
                 grid=([90, 100], [0.25, 0.5, 1.0]))


def test_model_file_keeps_the_grid(tmp_path):
    from dhcos.ffn import FFNModel
    m = R.random_model(R.WIDTH_SETS[0])
    g = FFNModel(m.features, m.x_mean, m.x_std, m.y_mean, m.y_std, m.weights, m.biases,
                 grid=([90, 95, 100, 105, 110], [0.25, 0.5, 1.0]))
    g.save(tmp_path / "g.npz")
    got = FFNModel.load(tmp_path / "g.npz")
    assert all(np.array_equal(a, b) for a, b in zip(got.grid, g.grid))
