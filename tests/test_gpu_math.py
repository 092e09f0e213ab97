"""GPU tests of the fp64 elementary functions of csrc/dh_device.h, one by one, through
dh_math_probe (csrc/dh_math_probe.h: the inline functions themselves, one lane per element, the LDS
tables filled as the production kernels fill them).

Truth: tests/golden/math_truth.npz (tests/golden/make_math_truth.py: mpmath at 60 digits, stored as
double-doubles), so the error |(got - hi) - lo| / unit has sub-ulp resolution in plain float64.
Each function is measured in the metric its header comment states (tools/math_accuracy.py holds
the shared code and records the measured maxima in profiles/math_accuracy.json):
  ulp     ulps of the true result (units of 2^-1074 in the subnormal range)
  abs53   units of 2^-53 absolute (dsincos_t), plus ulps of the result where |result| >= 2^-5
  logabs  ulps of max(|log x|, 2^-8) (dlog_t)
  cabs    componentwise, in ulps of |z| (complex helpers)
Bound: DESIGN.md 3's contract for the lean primitives, 2 units of the function's metric (BOUND).
Three outputs exceed it on the GPU; each is held to the worst-case error budget written in its
header comment in dh_device.h (BOUNDS), which follows from the arithmetic and the seed's stated
precision, not from a measurement: dsqrt_rsqrt's rs output (193 ulp: 1.5 e0^2 of a 2^-23 seed;
measured 17.6), datan2 just above its pi/8 switch (6 ulp; measured 2.1) and cdiv_rcp (6 ulp of
|z|; measured 2.2).  No bound comes from a measurement of the code under test.
"""
import importlib.util
import math
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("math_accuracy",
                                               os.path.join(ROOT, "tools", "math_accuracy.py"))
MA = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MA)

BOUND = 2.0                       # every lean primitive within 2 ulp of its metric
# the rs output of dsqrt_rsqrt*: 1.5 e0^2 of the v_rsq_f64 seed's e0 <= 2^-23 (AMD's ISA manuals:
# 2^29 ulp) is 1.5 * 2^-46 = 192 ulp, plus one for the roundings (dh_device.h)
kRsqrtUlpBudget = 1.5 * 2.0 ** -46 / 2.0 ** -53 + 1.0
# (function, output) -> the budget of its header comment, where that is above BOUND
BOUNDS = {("dsqrt_rsqrt", "rsqrt"): kRsqrtUlpBudget, ("dsqrt_rsqrt_pos", "rsqrt"): kRsqrtUlpBudget,
          ("datan2", "atan2"): 6.0, ("cdiv_rcp", "re"): 6.0, ("cdiv_rcp", "im"): 6.0}
PI_2 = 1.5707963267948966         # the double nearest pi/2


@pytest.fixture(scope="module")
def native():
    from dhcos import _native
    if _native.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return _native


@pytest.fixture(scope="module")
def truth():
    T = MA.load_truth()
    for v in T.values():
        v.setflags(write=False)
    return T


@pytest.fixture(scope="module")
def probed(native, truth):
    """fn -> (indices into its group, outputs): one probe launch per function, shared."""
    cache = {}

    def get(fn):
        if fn not in cache:
            idx = MA.select(fn, truth)
            cache[fn] = (idx, MA.probe(fn, truth, idx, native.math_probe))
        return cache[fn]
    return get


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def fam(T, fn, idx, *names):
    return MA.family(T, MA.SPEC[fn][0], *names)[idx]


@pytest.mark.parametrize("fn", list(MA.SPEC))
def test_accuracy(truth, probed, fn):
    """Every counted point within the bound in the function's metric; where the truth is NaN or
    infinite (libm's special values, overflow) the result is NaN or that infinity; the sign of the
    truth is the sign of the result."""
    idx, outs = probed(fn)
    g, metric, labels, outside = MA.SPEC[fn]
    rep = MA.worst(fn, truth, idx, outs)
    err, counted = MA.errors(fn, truth, idx, outs)
    assert counted.sum() > 500
    for lab, e in zip(labels, err):
        r = rep["outputs"][lab]
        print(f"{fn} {lab}: max {r['max_err']:.4f} {metric} (bound {BOUNDS.get((fn, lab), BOUND)}) "
              f"over {r['points']} points at {r['at_hex']}")
    for k, (lab, e) in enumerate(zip(labels, err)):
        bad = counted & ~(e <= BOUNDS.get((fn, lab), BOUND))
        assert not bad.any(), (fn, lab, rep["outputs"][lab])
        hi = truth[f"{g}__hi{k}"][idx]
        skip = fam(truth, fn, idx, *outside) if outside else np.zeros(idx.size, dtype=bool)
        nan, inf = np.isnan(hi) & ~skip, np.isinf(hi) & ~skip
        assert np.all(np.isnan(outs[k][nan])), (fn, lab)
        assert np.array_equal(outs[k][inf], hi[inf]), (fn, lab)
        if metric == "ulp" and fn != "dsincos":    # sin(-0) = +0 here: no contract on that zero
            nz = counted & ((hi != 0.0) | (g == "atan2"))
            assert np.array_equal(np.signbit(outs[k][nz]), np.signbit(hi[nz])), (fn, lab)


@pytest.mark.parametrize("fn", ["dsincos", "dsincos_t"])
def test_sincos_edges(truth, probed, fn):
    idx, (s, c) = probed(fn)
    x = truth["sincos__x"][idx]
    nf = fam(truth, fn, idx, "nonfinite")
    assert nf.sum() == 3 and np.all(np.isnan(s[nf])) and np.all(np.isnan(c[nf]))
    # beyond the documented domain, 2^20 <= |x| < 2^31: no accuracy bound, but finite and within
    # the unit circle ("degrades gracefully")
    far = fam(truth, fn, idx, "beyond_domain")
    assert far.sum() > 100 and np.all(np.abs(x[far]) >= 2.0 ** 20)
    lim = 1.0 + 2.0 ** -50
    assert np.all(np.isfinite(s[far])) and np.all(np.isfinite(c[far]))
    assert np.all(np.abs(s[far]) <= lim) and np.all(np.abs(c[far]) <= lim)
    err, _ = MA.errors(fn, truth, idx, [s, c])
    print(f"{fn} beyond the domain: worst error {max(err[0][far].max(), err[1][far].max()):.3g} "
          f"{MA.SPEC[fn][1]} (not asserted)")


def test_sincos_t_relative(truth, probed):
    """dsincos_t's accuracy is absolute; relative to the result it holds where |result| >= 2^-5."""
    idx, outs = probed("dsincos_t")
    _, counted = MA.errors("dsincos_t", truth, idx, outs)
    for k, lab in enumerate(("sin", "cos")):
        hi, lo = truth[f"sincos__hi{k}"][idx], truth[f"sincos__lo{k}"][idx]
        m = counted & (np.abs(hi) >= 2.0 ** -5)
        e = np.abs((outs[k] - hi) - lo)[m] / np.spacing(np.abs(hi[m]))
        w = int(np.argmax(e))
        print(f"dsincos_t {lab}: max {e[w]:.4f} ulp of the result over {int(m.sum())} points with "
              f"|result| >= 2^-5, at x = {truth['sincos__x'][idx][m][w].hex()}")
        assert m.sum() > 1000 and np.all(e <= BOUND), (lab, e[w])


def test_sincos_t_at_multiples_of_half_pi(truth, probed):
    """Where the table entry is exactly 0 -- sin at multiples of pi, cos at odd multiples of pi/2 --
    dsincos_t returns the reduced argument's sine alone, so there the result is accurate relative
    to itself, however small: within the common 2 ulp at the doubles that come closest to a
    multiple of pi/2 (reduced arguments down to 1e-6 ulp of x).  This is what the reduction's
    second and third terms are for; the absolute metric cannot see them."""
    idx, outs = probed("dsincos_t")
    m = fam(truth, "dsincos_t", idx, "near_pi2_multiple")
    x = truth["sincos__x"][idx][m]
    k = np.rint(np.abs(x) / (math.pi / 2)).astype(np.int64)
    assert m.sum() == 40 and (k % 2 == 0).sum() >= 5 and (k % 2 == 1).sum() >= 5
    worst = 0.0
    for i in range(x.size):
        o = int(k[i] % 2)                                       # 0: sin is the small one, 1: cos
        hi, lo = truth[f"sincos__hi{o}"][idx][m][i], truth[f"sincos__lo{o}"][idx][m][i]
        assert abs(hi) < 2.0 ** -33
        worst = max(worst, abs((outs[o][m][i] - hi) - lo) / np.spacing(abs(hi)))
    print(f"dsincos_t at the closest multiples of pi/2: worst {worst:.4f} ulp of the small result")
    assert worst <= BOUND


@pytest.mark.parametrize("fn", ["dexp", "dexp_nonpos", "dexp_t", "dexp_t_nonpos"])
def test_exp_edges(truth, probed, fn):
    idx, (e,) = probed(fn)
    x, hi = truth["exp__x"][idx], truth["exp__hi0"][idx]
    low = fam(truth, fn, idx, "select_low", "underflow")
    assert low.sum() >= 25 and np.any(np.isneginf(x[low])) and same_bits(e[low], np.zeros(low.sum()))
    assert np.all(np.isnan(e[np.isnan(x)])) and np.isnan(x).sum() == 1
    if fn.endswith("nonpos"):
        assert np.all(~(x > 0.0))
        return
    # inf only where the truth overflows (dexp_t: or x > 709.8); every finite result is counted
    over = np.isposinf(hi)
    assert over.sum() >= 15 and np.all(np.isposinf(e[over]))
    assert np.all(np.isfinite(e[~over & ~np.isnan(x)]))
    assert np.all(np.isposinf(e[x >= 1024.0])) and (x >= 1024.0).sum() >= 4
    if fn == "dexp_t":
        sel = fam(truth, fn, idx, "select_high_t")
        assert sel.sum() == 4 and np.all(np.isposinf(e[sel & (x > 709.8)]))
        assert np.isfinite(e[x == 709.78][0]) and np.isfinite(hi[x == 709.78][0])


@pytest.mark.parametrize("fn", ["dexp", "dexp_t"])
def test_exp_nonpos_same_bits(truth, probed, fn):
    """'The same bits' as the full form on x <= 0 (and -inf, NaN)."""
    idx, (e,) = probed(fn)
    idx_n, (en,) = probed(fn + "_nonpos")
    assert idx_n.size > 600
    assert same_bits(en, e[np.isin(idx, idx_n)])


def test_log_special_values(truth, probed):
    idx, (lt,) = probed("dlog_t")
    npn = fam(truth, "dlog_t", idx, "not_positive_normal")
    assert npn.sum() == 9 and np.all(np.isnan(lt[npn]))         # its comment: all of these NaN
    idx, (lg,) = probed("dlog")
    x = truth["log__x"][idx]
    with np.errstate(all="ignore"):
        want = np.log(x[npn])                                   # libm's special values
    got = lg[npn]
    sub = (x[npn] > 0.0) & np.isfinite(x[npn])                  # subnormals: in dlog's domain
    assert sub.sum() == 2 and np.all(np.isfinite(got[sub]))
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got[~sub & ~np.isnan(want)], want[~sub & ~np.isnan(want)])
    one = x == 1.0
    assert one.sum() >= 1 and same_bits(lg[one], np.zeros(one.sum()))


@pytest.mark.parametrize("fn", ["datan2", "datan2_t"])
def test_atan2_rules(truth, probed, fn):
    idx, (a,) = probed(fn)
    y, x = truth["atan2__x"][idx], truth["atan2__y"][idx]       # the probe's x is atan2's y
    hi = truth["atan2__hi0"][idx]
    # the one documented deviation from libm: x = -0 with y != 0 gives pi/2 exactly one ulp high
    nz = fam(truth, fn, idx, "x_negative_zero")
    assert nz.sum() == 4
    assert same_bits(a[nz], np.copysign(np.nextafter(PI_2, 4.0), y[nz]))
    assert same_bits(hi[nz], np.copysign(PI_2, y[nz]))
    zz = fam(truth, fn, idx, "zero_zero")
    assert zz.sum() == 4
    if fn == "datan2_t":
        assert np.all(np.isnan(a[zz]))                          # its comment: (0, 0) gives NaN
        return
    # atan2(+-0, -0) = +-pi, atan2(+-0, +0) = +-0
    assert same_bits(a[zz], np.copysign(np.where(np.signbit(x[zz]), math.pi, 0.0), y[zz]))
    ax = fam(truth, fn, idx, "axes")
    assert same_bits(a[ax], np.arctan2(y[ax], x[ax]))           # on the axes: libm's values
    nan = fam(truth, fn, idx, "nan")
    assert nan.sum() == 4 and np.all(np.isnan(a[nan]))
    # outside the documented domain (finite operands): an infinite operand gives NaN
    inf = fam(truth, fn, idx, "infinite")
    assert inf.sum() == 7 and np.all(np.isnan(a[inf]))


def test_datan2_budget_is_local(truth, probed):
    """datan2's 6-ulp budget is for results just above its pi/8 switch (|at| near pi/8 under a
    result below 1/2, of half pi/4's ulp); wherever the reduced argument t = min/max is outside
    (tan(pi/8), tan(1/2)] the common 2 ulp hold."""
    idx, outs = probed("datan2")
    err, counted = MA.errors("datan2", truth, idx, outs)
    ay, ax = np.abs(truth["atan2__x"][idx]), np.abs(truth["atan2__y"][idx])
    with np.errstate(all="ignore"):
        t = np.minimum(ax, ay) / np.maximum(ax, ay)
    away = counted & ~((t > 0.41421356237309503) & (t <= 0.5463024898437906))
    assert away.sum() > 1000 and np.all(err[0][away] <= BOUND), float(err[0][away].max())


def test_atan2_t_table_lo(truth, probed):
    """Where no quadrant step follows the table (x > 0, |y| <= x) and j = rint(64 |y| / x) >= 16,
    datan2_t's result is hi + (at + lo) and its header's budget is 25/32 ulp: 1/2 for the final
    sum, and (2^-57 for at, off by <= 8 * 2^-53 of |at| <= 2^-7, plus 2^-60 for at + lo) <= 9/32 ulp
    of a result > 2^-3.  The table's lo, up to half an ulp of hi, is inside that budget only if it
    is added: this is the assertion that sees kAtanJ64's lo column on the device."""
    idx, outs = probed("datan2_t")
    err, counted = MA.errors("datan2_t", truth, idx, outs)
    y, x = truth["atan2__x"][idx], truth["atan2__y"][idx]       # the probe's x is atan2's y
    with np.errstate(all="ignore"):
        m = counted & (x > 0) & (np.abs(y) <= x) & (np.abs(y) >= (16.5 / 64) * x)
    m &= fam(truth, "datan2_t", idx, "index_flip", "index_exact", "first_octant", "octants",
             "random", "diagonal", "pi8_switch")
    j = np.rint(64 * np.abs(y[m]) / x[m]).astype(int)
    assert m.sum() >= 300 and set(range(17, 65)) <= set(j)
    assert np.all(np.abs(truth["atan2__hi0"][idx][m]) > 2.0 ** -3)
    w = int(np.argmax(err[0][m]))
    print(f"datan2_t, no quadrant step, j >= 16: max {err[0][m][w]:.4f} ulp (bound 25/32) over "
          f"{int(m.sum())} points at y = {y[m][w].hex()}, x = {x[m][w].hex()}")
    assert np.all(err[0][m] <= 25.0 / 32.0)


def test_rcp_domain(truth, probed):
    """drcp's domain is 2^-1023 <= |x| < inf (its header comment).  A subnormal below 2^-1024,
    whose reciprocal overflows, gives NaN; the subnormals from 2^-1023 up and |x| > 2^1022, where
    1/x is subnormal, are within the common bound (in units of 2^-1074)."""
    idx, (r,) = probed("drcp")
    x = truth["rcp__x"][idx]
    assert np.all(np.isnan(r[np.isnan(x)]))
    err, _ = MA.errors("drcp", truth, idx, [r])
    sub = fam(truth, "drcp", idx, "subnormal")
    huge = fam(truth, "drcp", idx, "huge")
    assert sub.sum() == 8 and huge.sum() == 8
    over = sub & (np.abs(x) < 2.0 ** -1024)
    assert over.sum() == 4 and np.all(np.isnan(r[over]))
    rest = (sub & ~over) | huge
    assert np.abs(x[sub & ~over]).min() == 2.0 ** -1023
    for xv, rv in zip(x[rest], r[rest]):
        print(f"drcp: x = {xv.hex()} -> {rv.hex()}")
    assert np.all(err[0][rest] <= BOUND) and np.all(np.signbit(r[rest]) == np.signbit(x[rest]))


@pytest.mark.parametrize("fn", ["dsqrt_rsqrt", "dsqrt_rsqrt_pos"])
def test_sqrt_edges(truth, probed, fn):
    idx, (sq, rs) = probed(fn)
    x = truth["sqrt__x"][idx]
    assert np.all(np.isnan(sq[np.isnan(x)])) and np.all(np.isnan(rs[np.isnan(x)]))
    four = fam(truth, fn, idx, "four_minus_ulp")
    assert four.sum() == 1 and same_bits(sq[four], [np.nextafter(2.0, 0.0)])
    if fn == "dsqrt_rsqrt":                                     # sq = x at 0 and +inf
        zi = fam(truth, fn, idx, "zero_inf")
        assert zi.sum() == 2 and same_bits(sq[zi], x[zi])


def test_csqrt_signs_and_zeros(truth, probed):
    """The sign and zero cases against NumPy's complex128 sqrt: (0, +-0), the negative real axis
    with +-0 imaginary part, pure imaginary inputs."""
    idx, (re, im) = probed("csqrt_p")
    m = fam(truth, "csqrt_p", idx, "zero", "negative_real", "positive_real", "pure_imaginary")
    assert m.sum() == 44
    z = np.empty(int(m.sum()), dtype=np.complex128)             # part by part: keeps every -0
    z.real, z.imag = truth["csqrt__x"][idx][m], truth["csqrt__y"][idx][m]
    want = np.sqrt(z)
    for got, w in ((re[m], want.real), (im[m], want.imag)):
        assert np.array_equal(np.signbit(got), np.signbit(w))
        assert np.array_equal(got == 0.0, w == 0.0)
        assert np.all(np.abs(got - w) <= BOUND * np.spacing(np.abs(want)))
    assert np.all(re >= 0.0) and not np.any(np.signbit(re))     # the principal root


def test_cdiv_numpy_bits(truth, probed):
    """cdiv is NumPy's scalar complex division (Smith's algorithm with a reciprocal scale),
    zero divisor included: the same bits."""
    idx, (re, im) = probed("cdiv")
    m = np.flatnonzero(~fam(truth, "cdiv", idx, "random"))
    assert m.size > 300
    T = truth
    diff = []
    with np.errstate(all="ignore"):
        for i in m:
            a = np.complex128(complex(T["cdiv__x"][idx][i], T["cdiv__y"][idx][i]))
            b = np.complex128(complex(T["cdiv__bx"][idx][i], T["cdiv__by"][idx][i]))
            q = a / b
            for got, w in ((re[i], q.real), (im[i], q.imag)):
                if not (same_bits(got, w) or (np.isnan(got) and np.isnan(w))):
                    diff.append((int(i), complex(a), complex(b), float(got), float(w)))
    print(f"cdiv: {len(diff)} of {2 * m.size} components differ from NumPy's bits")
    assert not diff, diff[:5]
    zd = fam(truth, "cdiv", idx, "zero_divisor")
    assert zd.sum() == 9 and not np.any(np.isfinite(re[zd]))


def test_cdiv_rcp_domain(truth):
    """The fixture probes cdiv_rcp on 2^-100 <= |z2| <= 2^100, where its comment says it is used."""
    r = np.hypot(truth["cdiv_rcp__bx"], truth["cdiv_rcp__by"])
    assert r.min() >= 2.0 ** -100 * (1 - 1e-12) and r.max() <= 2.0 ** 100 * (1 + 1e-12)
    assert r.min() < 2.0 ** -99 and r.max() > 2.0 ** 99


def test_probe_arguments(native):
    lib, ctx = native.load(), native.default_context()
    x = np.ones(4)
    o = np.empty(4)
    for fn in (-1, len(native.MATH_PROBE_FNS), 1000):
        assert lib.dh_math_probe(ctx.handle, fn, x.ctypes.data, x.ctypes.data, 4, o.ctypes.data,
                                 o.ctypes.data) == -1
    assert lib.dh_math_probe(ctx.handle, 8, x.ctypes.data, None, 4, o.ctypes.data,
                             o.ctypes.data) == -1              # atan2 needs y
    assert lib.dh_math_probe(ctx.handle, 0, None, None, 0, None, None) == 0     # n == 0: no-op
    with pytest.raises(native.NativeError):
        native.math_probe("dtan", x)
    assert native.math_probe("dexp", []).shape == (0,)
    # more than one block, a ragged tail, and position independence
    xs = np.linspace(-3.0, 3.0, 1000)
    full = native.math_probe("dexp_t", xs)
    for n in (1, 255, 256, 257, 1000):
        assert same_bits(native.math_probe("dexp_t", xs[:n]), full[:n])
    s, c = native.math_probe("dsincos_t", xs[::-1])
    s2, c2 = native.math_probe("dsincos_t", xs)
    assert same_bits(s[::-1], s2) and same_bits(c[::-1], c2)
