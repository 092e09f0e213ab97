"""CPU checks of what the GPU math tests stand on (tests/test_gpu_math.py):

* tests/golden/math_truth.npz: a sample of every function's stored truth re-derived with mpmath,
  independently of the generator's code, and every structured family of inputs present, so that a
  regenerated fixture cannot quietly lose its edges;
* the math tables of csrc (dh_sincos_table.h, dh_exp_table.h, dh_logatan_table.h): every hex
  literal against the value its generator's rule gives, bit for bit, and the LDS layout constants
  of dh_device.h against the table lengths.
"""
import math
import os
import re
import struct

import numpy as np
import pytest

from conftest import GOLDEN, PKG

CSRC = os.path.join(PKG, "csrc")
INF = float("inf")


@pytest.fixture(scope="module")
def mp():
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 60
    return mpmath


@pytest.fixture(scope="module")
def T():
    with np.load(os.path.join(GOLDEN, "math_truth.npz")) as z:
        return {k: z[k] for k in z.files}


def fam(T, g, name):
    fams = list(T[g + "__families"])
    assert name in fams, (g, name, fams)
    return T[g + "__fam"] == fams.index(name)


def has(col, values):
    """Every value (by bits) among the column's entries."""
    bits = set(np.ascontiguousarray(col, dtype=np.float64).view(np.uint64).tolist())
    return all(struct.unpack("<Q", struct.pack("<d", v))[0] in bits for v in values)


def near(v):
    return [math.nextafter(v, -INF), v, math.nextafter(v, INF)]


# ---- the fixture --------------------------------------------------------------------------------

def test_fixture_is_small_and_complete(T):
    # ~0.4 MB: nine input groups of 0.7k - 2.6k points, and every point costs 3 - 9 doubles that do
    # not compress (inputs, hi, and the lo that gives the GPU test its sub-ulp resolution); the
    # structured families alone are ~7k points (3 x 3 x 129 log edges, 3 points per k pi/2, k pi/64
    # and index flip).  Half the limit for a committed file, and at most 3k points per group.
    assert os.path.getsize(os.path.join(GOLDEN, "math_truth.npz")) < (1 << 19)
    assert all(T[k].size <= 3000 for k in T if k.endswith("__x"))
    for g, nout, cols in (("sincos", 2, "x"), ("exp", 1, "x"), ("log", 1, "x"), ("atan2", 1, "xy"),
                          ("rcp", 1, "x"), ("sqrt", 2, "x"), ("csqrt", 2, "xy"),
                          ("cdiv", 2, ("x", "y", "bx", "by")),
                          ("cdiv_rcp", 2, ("x", "y", "bx", "by"))):
        n = T[g + "__x"].size
        assert n >= 600, g
        for c in cols:
            assert T[f"{g}__{c}"].shape == (n,) and T[f"{g}__{c}"].dtype == np.float64
        for k in range(nout):
            hi, lo = T[f"{g}__hi{k}"], T[f"{g}__lo{k}"]
            assert hi.shape == lo.shape == (n,)
            f = np.isfinite(hi)
            # lo is a remainder: at most half an ulp of hi
            assert np.all(np.abs(lo[f]) <= 0.5 * np.spacing(np.abs(hi[f]))), g
        assert T[g + "__fam"].shape == (n,) and T[g + "__fam"].max() < T[g + "__families"].size


def test_sincos_families(T):
    x = T["sincos__x"]
    tiny, sub = 2.2250738585072014e-308, 12345 * 5e-324
    assert has(x[fam(T, "sincos", "zero_tiny")], [0.0, -0.0, 2.0 ** -30, tiny, sub])
    for k in (1, 2, 3, 4, 2 ** 10, 2 ** 19):       # float(k pi/2) is the nearest double for these
        assert has(np.abs(x[fam(T, "sincos", "kpi2")]), near(k * math.pi / 2)), k
    for k in (1, 2, 4, 2 ** 10, 2 ** 24):
        assert has(np.abs(x[fam(T, "sincos", "kpi64")]), near(k * math.pi / 64)), k
    assert fam(T, "sincos", "kpi2").sum() >= 3 * 150 and fam(T, "sincos", "kpi64").sum() >= 3 * 150
    assert np.abs(x[fam(T, "sincos", "kpi2")]).max() > 2.0 ** 19
    fl = np.abs(x[fam(T, "sincos", "index_flip")])
    assert fl.size >= 3 * 128
    j = fl * (64 / math.pi) - 0.5                   # every point within a few ulps of (j + 1/2) pi/64
    assert np.all(np.abs(j - np.rint(j)) < 1e-6) and set(range(128)) <= set(np.rint(j).astype(int))
    close = x[fam(T, "sincos", "near_pi2_multiple")]
    k = np.rint(np.abs(close) / (math.pi / 2))
    nm = fam(T, "sincos", "near_pi2_multiple")
    small = np.where(k % 2 == 0, T["sincos__hi0"][nm], T["sincos__hi1"][nm])
    assert close.size == 40 and np.all(np.abs(small) < 1e-3 * np.spacing(np.abs(close)))
    assert has(x[fam(T, "sincos", "domain_edge")], [math.nextafter(2.0 ** 20, 0.0)])
    nf = x[fam(T, "sincos", "nonfinite")]
    assert np.isnan(nf).sum() == 1 and has(nf, [INF, -INF])
    far = np.abs(x[fam(T, "sincos", "beyond_domain")])
    assert far.size > 100 and far.min() == 2.0 ** 20 and far.max() == math.nextafter(2.0 ** 31, 0)
    rest = ~(fam(T, "sincos", "beyond_domain") | fam(T, "sincos", "nonfinite"))
    assert np.abs(x[rest]).max() < 2.0 ** 20 and fam(T, "sincos", "random").sum() >= 500


def test_exp_families(T):
    x = T["exp__x"]
    assert has(x[fam(T, "exp", "zero_tiny")], [0.0, -0.0, 2.0 ** -30, -2.0 ** -60])
    ln2 = math.log(2.0)
    for name, step, count in (("index_flip64", ln2 / 64, 100), ("index_flip1", ln2, 40)):
        v = x[fam(T, "exp", name)]
        q = v / step - 0.5
        assert v.size >= 3 * count and np.all(np.abs(q - np.rint(q)) < 1e-6), name
        assert np.ptp(np.rint(q)) > (1500 if name == "index_flip1" else 60000)
    sr = x[fam(T, "exp", "subnormal_result")]
    assert sr.size >= 100 and sr.min() == -745.13 and sr.max() == -708.4
    assert has(x[fam(T, "exp", "rounds_to_zero")], [-745.2])
    assert T["exp__hi0"][fam(T, "exp", "rounds_to_zero")][0] == 0.0
    assert has(x[fam(T, "exp", "select_low")], [-1075.0, math.nextafter(-1075.0, -INF), -INF])
    assert has(x[fam(T, "exp", "select_high_t")], [709.78, 709.8, math.nextafter(709.8, INF)])
    assert has(x[fam(T, "exp", "overflow")], [1024.0, math.nextafter(1024.0, INF), INF])
    assert np.isnan(x[fam(T, "exp", "nan")]).all()
    assert (x <= 0).sum() > 600 and fam(T, "exp", "random").sum() >= 800


def test_log_families(T):
    x = T["log__x"]
    edges = x[fam(T, "log", "subinterval_edge")]
    for k in (0, -300, 700):
        for i in (0, 1, 64, 127, 128):
            e = math.ldexp(struct.unpack("<d", struct.pack("<Q", 0x3FE6000000000000 + (i << 45)))[0], k)
            assert has(edges, near(e)), (k, i)
    assert edges.size == 3 * 3 * 129
    assert has(x[fam(T, "log", "near_one")], near(1.0) + [1 - 2.0 ** -30, 1 + 2.0 ** -30])
    assert has(x[fam(T, "log", "range_wrap")], near(0.6875 * 2.0 ** 1000) + near(1.375 / 2))
    assert has(x[fam(T, "log", "extremes")], [2.2250738585072014e-308, 1.7976931348623157e308])
    npn = x[fam(T, "log", "not_positive_normal")]
    assert has(npn, [0.0, -0.0, 5e-324, -1.5, INF, -INF]) and np.isnan(npn).sum() == 1
    assert fam(T, "log", "random").sum() >= 800


def test_atan2_families(T):
    y, x = T["atan2__x"], T["atan2__y"]
    o = fam(T, "atan2", "octants")
    octant = np.floor(np.arctan2(y[o], x[o]) / (math.pi / 4)).astype(int)
    assert set(octant) == set(range(-4, 4)) and np.bincount(octant + 4).min() >= 30
    d = fam(T, "atan2", "diagonal")
    assert d.sum() >= 8 and np.all(np.abs(y[d]) == np.abs(x[d]))
    assert len({(a, b) for a, b in zip(np.sign(y[d]), np.sign(x[d]))}) == 4
    for name, off in (("index_flip", 0.5), ("index_exact", 0.0)):
        m = fam(T, "atan2", name)
        mn, mx = np.minimum(np.abs(x[m]), np.abs(y[m])), np.maximum(np.abs(x[m]), np.abs(y[m]))
        j = 64 * mn / mx - off
        assert np.all(np.abs(j - np.rint(j)) < 1e-9), name
        assert set(np.rint(j).astype(int)) >= set(range(0 if off else 1, 64)), name
        assert len({(a, b, c) for a, b, c in zip(np.signbit(y[m]), np.signbit(x[m]),
                                                 np.abs(y[m]) > np.abs(x[m]))}) == 8, name
    m = fam(T, "atan2", "pi8_switch")
    t = np.minimum(np.abs(x[m]), np.abs(y[m])) / np.maximum(np.abs(x[m]), np.abs(y[m]))
    assert (t > 0.41421356237309503).any() and (t <= 0.41421356237309503).any()
    assert np.all(np.abs(t - 0.41421356237309503) < 1e-15)
    m = fam(T, "atan2", "ratios")
    lr = np.rint(np.abs(np.log2(np.abs(y[m] / 1.25)) - np.log2(np.abs(x[m] / 1.25)))).astype(int)
    assert {30, 300, 1000} <= set(lr)
    assert fam(T, "atan2", "axes").sum() == 12 and fam(T, "atan2", "zero_zero").sum() == 4
    m = fam(T, "atan2", "x_negative_zero")
    assert m.sum() == 4 and np.all(x[m] == 0) and np.all(np.signbit(x[m])) and np.all(y[m] != 0)
    assert fam(T, "atan2", "nan").sum() == 4 and fam(T, "atan2", "infinite").sum() == 7
    assert fam(T, "atan2", "random").sum() >= 500
    m = fam(T, "atan2", "first_octant")
    assert m.sum() >= 200 and np.all(x[m] > 0) and np.all(np.abs(y[m]) <= x[m])
    assert np.all(np.abs(y[m]) > 0.2578125 * x[m]) and np.signbit(y[m]).any()


def test_rcp_sqrt_families(T):
    for g in ("rcp", "sqrt"):
        x = np.abs(T[g + "__x"][fam(T, g, "mantissa_exponent")])
        m, e = np.frexp(x)
        assert {0.5, math.nextafter(0.5, 1.0), math.nextafter(1.0, 0.0)} <= set(m)
        assert e.min() == -1021 and e.max() >= 1022 and (e % 2 == 0).any() and (e % 2 == 1).any()
        assert np.isnan(T[g + "__x"][fam(T, g, "nan")]).all()
    assert has(T["sqrt__x"][fam(T, "sqrt", "four_minus_ulp")], [math.nextafter(4.0, 0.0)])
    assert has(T["sqrt__x"][fam(T, "sqrt", "zero_inf")], [0.0, INF])
    sub = np.abs(T["rcp__x"][fam(T, "rcp", "subnormal")])
    assert sub.size == 8 and sub.max() < 2.2250738585072014e-308 and sub.min() == 5e-324
    huge = np.abs(T["rcp__x"][fam(T, "rcp", "huge")])
    assert huge.size == 8 and huge.min() > 2.0 ** 1022
    rest = np.abs(T["rcp__x"][~(fam(T, "rcp", "subnormal") | fam(T, "rcp", "huge"))])
    assert np.nanmin(rest) >= 2.0 ** -1022 and np.nanmax(rest) <= 2.0 ** 1022


def test_complex_families(T):
    x, y = T["csqrt__x"], T["csqrt__y"]
    z = fam(T, "csqrt", "zero")
    assert z.sum() == 4 and len(set(zip(np.signbit(x[z]), np.signbit(y[z])))) == 4
    m = fam(T, "csqrt", "negative_real")
    assert np.all(x[m] < 0) and np.all(y[m] == 0) and set(np.signbit(y[m])) == {True, False}
    m = fam(T, "csqrt", "pure_imaginary")
    assert np.all(x[m] == 0) and np.all(y[m] != 0) and set(np.signbit(x[m])) == {True, False}
    assert fam(T, "csqrt", "random").sum() >= 500
    bx, by = T["cdiv__bx"], T["cdiv__by"]
    m = fam(T, "cdiv", "zero_divisor")
    assert m.sum() >= 8 and np.all(bx[m] == 0) and np.all(by[m] == 0)
    assert (~fam(T, "cdiv", "random")).sum() > 300 and fam(T, "cdiv", "random").sum() >= 500
    assert np.all(np.abs(bx[fam(T, "cdiv", "equal_parts")]) == np.abs(by[fam(T, "cdiv", "equal_parts")]))
    r = np.hypot(T["cdiv_rcp__bx"], T["cdiv_rcp__by"])
    assert r.size >= 600 and r.min() < 2.0 ** -99 and r.max() > 2.0 ** 99


def test_truth_rederived(T, mp):
    """Every 7th point of every group (and so of every family with 7 or more points) against mpmath,
    evaluated here: hi + lo agrees with the truth to 2^-100 of its size (lo's own rounding)."""
    mpf, mpc = mp.mpf, mp.mpc

    def agree(hi, lo, want, where):
        if not math.isfinite(hi):
            return
        got = mpf(float(hi)) + mpf(float(lo))
        tol = max(abs(want) * mpf(2) ** -100, mpf(2) ** -1075)
        assert abs(got - want) <= tol, where
        assert float(hi) == float(want) or abs(want) < mpf(2) ** -1021, where   # hi is the nearest

    fns = {"sincos": lambda x: (mp.sin(x), mp.cos(x)), "exp": lambda x: (mp.exp(x),),
           "log": lambda x: (mp.log(x),), "rcp": lambda x: (1 / x,),
           "sqrt": lambda x: (mp.sqrt(x), 1 / mp.sqrt(x))}
    checked = 0
    for g, f in fns.items():
        for i in range(0, T[g + "__x"].size, 7):
            x = float(T[g + "__x"][i])
            if not math.isfinite(x) or (g in ("log", "sqrt", "rcp") and x <= 0 and g != "rcp") \
                    or x == 0:
                continue
            for k, want in enumerate(f(mpf(x))):
                agree(T[f"{g}__hi{k}"][i], T[f"{g}__lo{k}"][i], want, (g, i, x))
                checked += 1
    for i in range(0, T["atan2__x"].size, 7):
        y, x = float(T["atan2__x"][i]), float(T["atan2__y"][i])
        if math.isfinite(x) and math.isfinite(y) and x != 0 and y != 0:
            agree(T["atan2__hi0"][i], T["atan2__lo0"][i], mp.atan2(mpf(y), mpf(x)), ("atan2", i))
            checked += 1
    for i in range(0, T["csqrt__x"].size, 7):
        x, y = float(T["csqrt__x"][i]), float(T["csqrt__y"][i])
        if y != 0:
            r = mp.sqrt(mpc(mpf(x), mpf(y)))
            agree(T["csqrt__hi0"][i], T["csqrt__lo0"][i], r.real, ("csqrt re", i))
            agree(T["csqrt__hi1"][i], T["csqrt__lo1"][i], r.imag, ("csqrt im", i))
            checked += 2
    for g in ("cdiv", "cdiv_rcp"):
        for i in range(0, T[g + "__x"].size, 7):
            a = mpc(mpf(float(T[g + "__x"][i])), mpf(float(T[g + "__y"][i])))
            b = mpc(mpf(float(T[g + "__bx"][i])), mpf(float(T[g + "__by"][i])))
            if b != 0:
                agree(T[g + "__hi0"][i], T[g + "__lo0"][i], (a / b).real, (g, i))
                agree(T[g + "__hi1"][i], T[g + "__lo1"][i], (a / b).imag, (g, i))
                checked += 2
    assert checked > 1500


def test_truth_special_values(T):
    """The non-finite expectations stored in hi follow libm."""
    x = T["log__x"]
    with np.errstate(all="ignore"):
        want = np.log(x)
    sp = ~np.isfinite(want)
    assert sp.sum() == 7 and np.array_equal(T["log__hi0"][sp], want[sp], equal_nan=True)
    x = T["exp__x"]
    assert np.all(np.isposinf(T["exp__hi0"][x > 709.79])) and np.all(T["exp__hi0"][x < -746] == 0)
    ax = fam(T, "atan2", "axes") | fam(T, "atan2", "zero_zero") | fam(T, "atan2", "infinite")
    want = np.arctan2(T["atan2__x"][ax], T["atan2__y"][ax])
    assert np.array_equal(T["atan2__hi0"][ax].view(np.uint64), want.view(np.uint64))


# ---- the tables are what their generators say ---------------------------------------------------

def table(header, name, csrc=CSRC):
    """The hex literals of array `name` in csrc/<header>, as doubles, and its declared length."""
    txt = open(os.path.join(csrc, header)).read()
    m = re.search(r"const double %s\[(\d+)\] = \{(.*?)\};" % name, txt, flags=re.S)
    assert m, (header, name)
    body = re.sub(r"//[^\n]*", "", m.group(2))
    vals = [float.fromhex(t) for t in re.findall(r"-?0x[0-9a-fA-F.]+p[+-]?\d+", body)]
    assert len(vals) == int(m.group(1)), (header, name, len(vals))
    return vals


def table_mismatches(mp, csrc=CSRC):
    """(table, index, stored, wanted) for every entry that is not what its generator's rule gives."""
    mpf = mp.mpf
    bad = []

    def check(tab, i, got, want):
        if struct.pack("<d", got) != struct.pack("<d", float(want)):
            bad.append((tab, i, got.hex(), float(want).hex()))

    sc = table("dh_sincos_table.h", "kSinCosPi64", csrc)
    assert len(sc) == 256
    for j in range(128):                           # correctly rounded sin / cos (j pi/64)
        check("sin", j, sc[2 * j], mp.sinpi(mpf(j) / 64))
        check("cos", j, sc[2 * j + 1], mp.cospi(mpf(j) / 64))
    ex = table("dh_exp_table.h", "kExp2J64", csrc)
    assert len(ex) == 64
    for j in range(64):                            # correctly rounded 2^(j/64)
        check("exp2", j, ex[j], mpf(2) ** (mpf(j) / 64))
    at = table("dh_logatan_table.h", "kAtanJ64", csrc)
    assert len(at) == 130
    for j in range(65):                            # atan(j/64) = hi + lo
        a = mp.atan(mpf(j) / 64)
        check("atan hi", j, at[2 * j], a)
        check("atan lo", j, at[2 * j + 1], a - mpf(float(a)))
    lg = table("dh_logatan_table.h", "kLogInvcLogc", csrc)
    assert len(lg) == 256
    for i in range(128):
        invc, logc = lg[2 * i], lg[2 * i + 1]
        check("logc", i, logc, -mp.log(mpf(invc)))  # logc = -log(invc), rounded
        # invc by the generator's own rule: |z invc - 1| < 2^-8 over the subinterval (the extremes
        # are at its ends)
        zlo = struct.unpack("<d", struct.pack("<Q", 0x3FE6000000000000 + (i << 45)))[0]
        zhi = struct.unpack("<d", struct.pack("<Q", 0x3FE6000000000000 + ((i + 1) << 45)))[0]
        for z in (zlo, zhi):
            if not abs(mpf(z) * mpf(invc) - 1) < mpf(2) ** -8:
                bad.append(("invc", i, invc.hex(), None))
        check("invc", i, invc, 1 / ((mpf(zlo) + mpf(zhi)) / 2))
    return bad


def test_tables_match_their_generators(mp):
    assert table_mismatches(mp) == []


def test_table_check_sees_one_hex_digit(mp, tmp_path):
    """The check above fails when one hex digit of one entry changes (each table in turn, on a
    copy)."""
    import shutil
    for header, old in (("dh_sincos_table.h", "0x1.91f65f10dd814p-5"),
                        ("dh_exp_table.h", "0x1.02c9a3e778061p+0"),
                        ("dh_logatan_table.h", "-0x1.7cc7f7db46a0ep-2")):
        for h in ("dh_sincos_table.h", "dh_exp_table.h", "dh_logatan_table.h"):
            shutil.copy(os.path.join(CSRC, h), tmp_path / h)
        txt = (tmp_path / header).read_text()
        assert old in txt
        new = old[:-5] + ("5" if old[-5] != "5" else "6") + old[-4:]
        (tmp_path / header).write_text(txt.replace(old, new, 1))     # one entry
        bad = table_mismatches(mp, str(tmp_path))
        assert len(bad) == 1, (header, bad)


def test_layout_constants_match_the_tables():
    txt = open(os.path.join(CSRC, "dh_device.h")).read()
    k = {n: int(v) for n, v in re.findall(r"constexpr int (kTab\w+|kMathTab) = (\d+);", txt)}
    sincos = len(table("dh_sincos_table.h", "kSinCosPi64")) // 2     # double2 entries of each
    log = len(table("dh_logatan_table.h", "kLogInvcLogc")) // 2
    atan = len(table("dh_logatan_table.h", "kAtanJ64")) // 2
    exp = len(table("dh_exp_table.h", "kExp2J64")) // 2
    assert (sincos, log, atan, exp) == (128, 128, 65, 32)
    assert k["kTabLog"] == sincos
    assert k["kTabAtan"] == k["kTabLog"] + log
    assert k["kTabExp"] == k["kTabAtan"] + atan
    assert k["kMathTab"] == k["kTabExp"] + exp
