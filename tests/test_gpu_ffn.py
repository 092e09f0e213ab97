"""GPU tests of the warm-start network's inference kernel (ffn_forward_kernel, csrc/dh_ffn.h) and
of the hybrid calibrate_batch(x0s=model); DESIGN.md 3.22.  Numbering follows the CPU tests'
(tests/test_ffn.py holds 1-5).

   6. exact integers: small integer weights (asymmetric in every layer), biases 0 or 1, integer
      features -- every partial sum an integer below 2^24 -- so the device's raw output is NumPy's
      integer arithmetic exactly; a swapped operand or a wrong C/D map cannot pass;
   7. the device equals the host twin (tests/native/libffnhost.so) bit for bit on raw (float32)
      and x0 (float64): three width sets x B = 1, TM, TM + 1, 3 TM - 1, and a model whose first
      hidden layer's activations are float32 subnormals;
   8. the device against the float64 truth within the derived forward bound
      (tests/ffn_reference.py), same cases;
   9. batch independence and repeatability: a row of the B = 3 TM - 1 call has the bits of the
      B = 1 call on that market; the same call twice gives the same bits; dh_ffn_forward_dev on a
      side stream equals the host-array form;
  10. end to end, small: 4,096 generator samples, hidden widths (64, 32), 30 epochs on the GPU,
      64 held-out markets -> validation MSE < 1.0; calibrate_batch(x0s=model, maxiter=10,
      gradient="analytic") starts from model.predict ([64, 1, 13]), ends at or below each start's
      own loss, equals the call with the predicted array, leaves the global RNG alone, and at
      least 60 of the 64 markets end finite.
"""
import numpy as np
import pytest

import ffn_reference as R

pytestmark = pytest.mark.gpu

WIDTH_IDS = ["x".join(map(str, w)) for w in R.WIDTH_SETS]


@pytest.fixture(scope="module")
def native():
    from dhcos import _native
    if _native.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return _native


@pytest.fixture(scope="module")
def cases(native):
    """Per width set (and the subnormal model): the model, the 3 TM - 1 markets, and -- computed
    once -- the twin's and the truth's outputs on them; every smaller B takes their leading rows
    (the twin and the truth work row by row)."""
    mkt, sp = R.markets(R.BATCHES[-1])
    out = {}
    models = {i: R.random_model(w, seed=len(w)) for i, w in zip(WIDTH_IDS, R.WIDTH_SETS)}
    models["subnormal"] = R.random_model(R.WIDTH_SETS[1], seed=8, first_scale=1e-39)
    for name, model in models.items():
        x0_t, raw_t = R.twin_forward(model, mkt, sp)
        truth, bound = R.forward_bound(model, mkt, sp)
        out[name] = dict(model=model, mkt=mkt, sp=sp, twin_x0=x0_t, twin_raw=raw_t, truth=truth,
                         bound=bound)
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ---- 6. exact integers ---------------------------------------------------------------------------

@pytest.mark.parametrize("widths", R.WIDTH_SETS[:2], ids=WIDTH_IDS[:2])
def test_exact_integers(native, widths):
    model = R.integer_model(widths, seed=21)
    rs = np.random.RandomState(2)
    B = R.TM + 5                                     # two blocks, a partial one
    prices = rs.randint(1, 5, size=(B, widths[0]))
    want = R.integer_forward(model, prices)
    assert np.abs(want).max() > 100                  # not a trivial network
    x0, raw = model.predict(prices.astype(np.float64), np.ones(B), want_raw=True)
    wrong = np.argwhere(raw.astype(np.int64) != want)
    assert wrong.size == 0 and np.array_equal(raw, want.astype(np.float32)), \
        (f"{len(wrong)} of {want.size} outputs differ; first (market, output) {wrong[:4].tolist()}: "
         f"device {raw[tuple(wrong[0])] if len(wrong) else None}, "
         f"integers {want[tuple(wrong[0])] if len(wrong) else None}")
    assert np.array_equal(x0, want.astype(np.float64))       # y_mean 0, y_std 1: one exact fma


# ---- 7. / 8. the twin bit for bit, the truth within the bound ------------------------------------

def one_product_report(case, b, o, got_raw):
    """The failure message of a bit difference: the last layer's operands of output o of market b
    (the twin's activations are not exported, so the truth's are printed beside the two
    results)."""
    model = case["model"]
    z = (model.input_features(case["mkt"][b:b + 1], case["sp"][b:b + 1]) - model.x_mean) / model.x_std
    a = z
    for W, bias in zip(model.weights[:-1], model.biases[:-1]):
        a = np.maximum(a @ W.astype(np.float64).T + bias, 0.0)
    def hx(v):
        return hex(int(np.float32(v).view(np.uint32)))

    return (f"market {b} output {o}: device raw {got_raw!r} ({hx(got_raw)}), "
            f"twin {case['twin_raw'][b, o]!r} ({hx(case['twin_raw'][b, o])}); last layer: "
            f"bias {model.biases[-1][o]!r}, W row {model.weights[-1][o].tolist()}, "
            f"input (float64 truth) {a[0].tolist()}")


@pytest.mark.parametrize("B", R.BATCHES)
@pytest.mark.parametrize("name", WIDTH_IDS + ["subnormal"])
def test_device_equals_twin_and_truth(native, cases, name, B):
    c = cases[name]
    model = c["model"]
    x0, raw = model.predict(c["mkt"][:B], c["sp"][:B], want_raw=True)
    assert x0.shape == (B, 13) and raw.shape == (B, 13) and raw.dtype == np.float32
    if name == "subnormal":
        # the premise: the first hidden layer's activations are float32 subnormals, not zeros
        z = ((model.input_features(c["mkt"][:B], c["sp"][:B]) - model.x_mean) / model.x_std)
        a1 = np.maximum(z @ model.weights[0].astype(np.float64).T + model.biases[0], 0.0)
        tiny = (a1 > 0) & (a1 < 2.0 ** -126)
        assert tiny.mean() > 0.25
    # 8. the truth, within the derived bound
    err = np.abs(x0 - c["truth"][:B])
    print(f"{name} B={B}: max |x0 - truth| {err.max():.3e}, max error / bound "
          f"{np.max(err / c['bound'][:B]):.4f}")
    assert np.all(err <= c["bound"][:B])
    # 7. the twin, bit for bit
    diff = np.argwhere(bits(raw) != bits(c["twin_raw"][:B]))
    assert diff.size == 0, one_product_report(c, *diff[0], raw[tuple(diff[0])])
    assert np.array_equal(bits(x0), bits(c["twin_x0"][:B]))


# ---- 9. batch independence, repeatability, the device-pointer form -------------------------------

def test_rows_do_not_depend_on_the_batch(native, cases):
    c = cases[WIDTH_IDS[2]]
    model, mkt, sp = c["model"], c["mkt"], c["sp"]
    B = R.BATCHES[-1]
    x0, raw = model.predict(mkt, sp, want_raw=True)
    again = model.predict(mkt, sp, want_raw=True)
    assert np.array_equal(bits(x0), bits(again[0])) and np.array_equal(bits(raw), bits(again[1]))
    for i in (0, B // 2, B - 1):
        xi, ri = model.predict(mkt[i:i + 1], sp[i:i + 1], want_raw=True)
        assert np.array_equal(bits(xi[0]), bits(x0[i])), i
        assert np.array_equal(bits(ri[0]), bits(raw[i])), i


def test_device_pointer_form_on_a_side_stream(native, cases):
    import torch
    c = cases[WIDTH_IDS[1]]
    model, mkt, sp = c["model"], c["mkt"], c["sp"]
    x0, raw = model.predict(mkt, sp, want_raw=True)
    ctx = native.default_context()
    ffn = model.on_device()
    dev = torch.device("cuda", ctx.device)
    d_mkt = torch.from_numpy(mkt).to(dev)
    d_sp = torch.from_numpy(sp).to(dev)
    d_raw = torch.empty((mkt.shape[0], 13), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    d_x0 = ctx.ffn_forward_dev(ffn, d_mkt, d_sp, raw=d_raw, stream=side)
    side.synchronize()
    assert np.array_equal(bits(d_x0.cpu().numpy()), bits(x0))
    assert np.array_equal(bits(d_raw.cpu().numpy()), bits(raw))
    with pytest.raises(ValueError):
        ctx.ffn_forward_dev(ffn, d_mkt[:, :14].contiguous(), d_sp, stream=side)
    with pytest.raises(ValueError):
        ctx.ffn_forward_dev(ffn, d_mkt.float(), d_sp, stream=side)


def test_closing_the_context_closes_its_networks(native, cases):
    """A context destroys what lives on it: after Context.close() the network's handle is gone, its
    later collection touches nothing, and the model is uploaded again on the next use."""
    m = cases[WIDTH_IDS[0]]["model"]
    ctx = native.Context(0)
    ffn = native.FFN(ctx, m.widths, m.weights, m.biases, m.features, m.x_mean, m.x_std, m.y_mean,
                     m.y_std)
    x0 = ffn.forward(cases[WIDTH_IDS[0]]["mkt"][:3], cases[WIDTH_IDS[0]]["sp"][:3])
    assert np.array_equal(bits(x0), bits(cases[WIDTH_IDS[0]]["twin_x0"][:3]))
    ctx.close()
    assert ffn.handle is None and ctx.handle is None
    ffn.close()                                      # a second close is nothing
    del ffn


# ---- 10. end to end ------------------------------------------------------------------------------

def test_train_predict_and_hybrid_calibration(native):
    from dhcos import calibrate_batch, generate_synthetic_calibrations, train_ffn_on_generator
    from dhcos.generator import MATURITIES, STRIKES_PCT, grid_surface
    model, hist = train_ffn_on_generator(4096, gen_seed=123, widths=(64, 32), epochs=30, seed=0)
    print(f"validation MSE {hist['best_val']:.4f} after {len(hist['val'])} epochs, "
          f"{hist['seconds']:.2f} s")
    assert model.widths == (11, 64, 32, 13) and model.n_prices == 15
    assert np.array_equal(model.grid[0], STRIKES_PCT) and np.array_equal(model.grid[1], MATURITIES)
    assert hist["best_val"] < 1.0                    # the mean predictor's score
    np.random.seed(456)                              # held-out markets: another stretch of the RNG
    g = generate_synthetic_calibrations(64, None, as_arrays=True, verbose=False)
    mkt, sp, r = g["market_prices"], g["spot"], float(g["risk_free"])
    x0 = model.predict(mkt, sp)
    assert x0.shape == (64, 13) and np.all(np.isfinite(x0))
    state = np.random.get_state()
    res = calibrate_batch(mkt, sp, r, x0s=model, maxiter=10, gradient="analytic")
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
    assert res.start_x.shape == (64, 1, 13)
    assert np.all(res.nit <= 10)
    surf = grid_surface(native.default_context(), STRIKES_PCT, MATURITIES)[0]
    f0, _, bad0 = surf.loss_grad_rows(x0, mkt, sp, np.full(64, r), np.arange(64, dtype=np.int32))
    fun = res.fun[:, 0]
    finite = np.isfinite(fun)
    print(f"finite {finite.sum()} of 64; median loss at x0 {np.median(f0):.3e}, after 10 "
          f"iterations {np.median(fun[finite]):.3e}")
    assert finite.sum() >= 60
    assert np.all(fun[finite] <= f0[finite])
    same = calibrate_batch(mkt, sp, r, x0s=x0[:, None, :], maxiter=10, gradient="analytic")
    for name in ("x", "parameters", "final_loss", "fun", "nit", "nfev", "start_task", "start_x",
                 "model_prices", "best_start", "success"):
        assert np.array_equal(getattr(res, name), getattr(same, name), equal_nan=True), name
