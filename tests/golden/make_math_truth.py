"""Generate tests/golden/math_truth.npz: inputs and high-precision truth for the fp64 elementary
functions of csrc/dh_device.h (tests/test_gpu_math.py probes them through dh_math_probe;
tests/test_math_truth.py re-derives a sample and checks that every family below is present).

Every truth is evaluated with mpmath at 60 digits and stored as a double-double: hi = the nearest
double, lo = the nearest double of (truth - hi).  The GPU test forms |(got - hi) - lo| / ulp in
plain float64, with sub-ulp resolution and without mpmath.  (Below 2^-1021 the remainder is itself
rounded to a multiple of 2^-1074, so results there resolve to half a unit of 2^-1074.)

Layout: one input group per family of functions; the functions of a group share its points.
  <group>__x, <group>__y     inputs (y: atan2's second argument / imaginary parts)
  <group>__bx, <group>__by   the divisor of the complex divisions
  <group>__hi0, __lo0        first result (sin, exp, log, atan2, 1/x, sqrt, Re)
  <group>__hi1, __lo1        second result (cos, 1/sqrt, Im)
  <group>__fam               family index of each point into <group>__families (names)
Non-finite expectations (NaN, +-inf) and signed zeros are stored in hi with lo = 0; they follow
libm, and the test states where a function's documented contract differs.

Usage: python tests/golden/make_math_truth.py   (writes math_truth.npz next to itself)
"""
import math
import os
import struct

import mpmath
import numpy as np

mpmath.mp.dps = 60
mpf = mpmath.mpf
SEED = 20240607
NAN, INF = float("nan"), float("inf")
TINY = 2.2250738585072014e-308          # smallest normal
SUB = 12345 * 5e-324                    # a subnormal
HUGE = 1.7976931348623157e308
LOG_OFF = 0x3FE6000000000000            # dlog_t's z range starts at 0.6875

GROUPS = {                              # group -> functions probed on it
    "sincos": ("dsincos", "dsincos_t"),
    "exp": ("dexp", "dexp_nonpos", "dexp_t", "dexp_t_nonpos"),
    "log": ("dlog", "dlog_t"),
    "atan2": ("datan2", "datan2_t"),
    "rcp": ("drcp",),
    "sqrt": ("dsqrt_rsqrt", "dsqrt_rsqrt_pos"),
    "csqrt": ("csqrt_p",),
    "cdiv": ("cdiv",),
    "cdiv_rcp": ("cdiv_rcp",),
}


def bits_to_double(u):
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def nearest(v):
    """The double nearest the mpf v, correctly rounded in the subnormal range too (Python's
    integer true division rounds once)."""
    v = mpf(v)
    if v == 0:
        return 0.0
    sign, man, exp, bc = v._mpf_
    if exp + bc < -1080:                           # below half the smallest subnormal
        return -0.0 if sign else 0.0
    try:
        f = float(man << exp) if exp >= 0 else man / (1 << -exp)
    except OverflowError:
        f = INF
    return -f if sign else f


def dd(v):
    """(hi, lo) of the mpf v."""
    hi = nearest(v)
    if math.isinf(hi) or hi == 0.0 and v == 0:
        return hi, 0.0
    return hi, nearest(mpf(v) - mpf(hi))


def around(v):
    """The double nearest v and its two neighbours."""
    c = nearest(v) if not isinstance(v, float) else v
    return [math.nextafter(c, -INF), c, math.nextafter(c, INF)]


class Points:
    def __init__(self, ncol):
        self.cols = [[] for _ in range(ncol)]
        self.fam = []
        self.names = []

    def add(self, family, *rows):
        if family not in self.names:
            self.names.append(family)
        k = self.names.index(family)
        for row in rows:
            row = row if isinstance(row, tuple) else (row,)
            assert len(row) == len(self.cols)
            for c, v in zip(self.cols, row):
                c.append(float(v))
            self.fam.append(k)


def pm(vals):
    return [s * v for v in vals for s in (1.0, -1.0)]


# ---- truths (mpmath; special values follow libm) ------------------------------------------------

def t_sincos(x):
    if math.isnan(x) or math.isinf(x):
        return (NAN, 0.0), (NAN, 0.0)
    if x == 0.0:
        return (x, 0.0), (1.0, 0.0)
    return dd(mpmath.sin(mpf(x))), dd(mpmath.cos(mpf(x)))


def t_exp(x):
    if math.isnan(x):
        return (NAN, 0.0)
    if math.isinf(x):
        return (INF if x > 0 else 0.0, 0.0)
    return dd(mpmath.exp(mpf(x)))


def t_log(x):
    if math.isnan(x) or x < 0.0:
        return (NAN, 0.0)
    if x == 0.0:
        return (-INF, 0.0)
    if math.isinf(x):
        return (INF, 0.0)
    return dd(mpmath.log(mpf(x)))


def t_atan2(y, x):
    if math.isnan(x) or math.isnan(y):
        return (NAN, 0.0)
    if math.isinf(x) or math.isinf(y):            # libm: multiples of pi/4
        ay = mpmath.pi / 4 * (1 if x > 0 else 3) if math.isinf(x) and math.isinf(y) else (
            mpmath.pi / 2 if math.isinf(y) else (mpf(0) if x > 0 else mpmath.pi))
    elif x == 0.0:
        ay = mpmath.pi / 2 if y != 0.0 else (mpmath.pi if math.copysign(1.0, x) < 0 else mpf(0))
    else:
        ay = mpmath.atan2(mpf(abs(y)), mpf(x))
    hi, lo = dd(ay)
    s = math.copysign(1.0, y)
    return (s * hi, s * lo)


def t_rcp(x):
    if math.isnan(x):
        return (NAN, 0.0)
    return dd(1 / mpf(x))


def t_sqrt(x):
    if math.isnan(x):
        return (NAN, 0.0), (NAN, 0.0)
    if x == 0.0 or math.isinf(x):
        return (x, 0.0), (INF if x == 0.0 else 0.0, 0.0)
    r = mpmath.sqrt(mpf(x))
    return dd(r), dd(1 / r)


def t_csqrt(x, y):
    """Principal root; the imaginary part carries the sign of y (signed zeros as C99 / NumPy)."""
    r = mpmath.sqrt(mpmath.mpc(mpf(x), mpf(abs(y))))
    re, im = dd(r.real), dd(r.imag)
    s = math.copysign(1.0, y)
    return re, (s * im[0], s * im[1])


def t_cdiv(ax, ay, bx, by):
    if bx == 0.0 and by == 0.0:
        return (NAN, 0.0), (NAN, 0.0)             # the test compares this row with NumPy's bits
    q = mpmath.mpc(mpf(ax), mpf(ay)) / mpmath.mpc(mpf(bx), mpf(by))
    return dd(q.real), dd(q.imag)


# ---- inputs -------------------------------------------------------------------------------------

def build_sincos(rng):
    P = Points(1)
    P.add("zero_tiny", *pm([0.0, 2.0 ** -30, TINY, SUB]))
    for name, step, kmax, pow_max in (("kpi64", mpmath.pi / 64, 21361414, 24),
                                      ("kpi2", mpmath.pi / 2, 667544, 19)):
        ks = [1, 2, 3] + [2 ** p for p in range(2, pow_max + 1)]
        ks += [int(k) for k in rng.randint(4, kmax + 1, size=150)]
        for n, k in enumerate(ks):
            s = -1.0 if n % 4 == 3 else 1.0
            P.add(name, *[s * v for v in around(k * step)])
    js = list(range(128)) + [int(j) for j in rng.randint(128, 21361000, size=60)]
    for n, j in enumerate(js):
        s = -1.0 if n % 3 == 2 else 1.0
        P.add("index_flip", *[s * v for v in around((j + mpf(0.5)) * mpmath.pi / 64)])
    # the doubles that come closest, in their own ulps, to a multiple of pi/2 below 2^20: the reduced
    # argument there is far below an ulp of x, so it is the reduction's low terms that give the
    # small result (sin at even k, cos at odd k) its leading bits
    close = []
    for k in range(1, 667545):
        v = k * step
        c = nearest(v)
        close.append((abs(v - mpf(c)) / mpf(math.ulp(c)), c))
    close.sort()
    P.add("near_pi2_multiple", *[c * (1.0 if i % 2 else -1.0) for i, (_, c) in enumerate(close[:40])])
    P.add("domain_edge", *pm([math.nextafter(2.0 ** 20, 0.0)]))
    P.add("nonfinite", NAN, INF, -INF)
    beyond = [2.0 ** 20, math.nextafter(2.0 ** 31, 0.0)] + list(2.0 ** rng.uniform(20, 31, 150))
    P.add("beyond_domain", *[v * (1.0 if i % 2 else -1.0) for i, v in enumerate(beyond)])
    P.add("random", *rng.uniform(-2.0 ** 20, 2.0 ** 20, 500))
    P.add("random", *(2.0 ** rng.uniform(-40, 20, 300) * rng.choice([-1.0, 1.0], 300)))
    return P


def build_exp(rng):
    P = Points(1)
    P.add("zero_tiny", *pm([0.0, 2.0 ** -30, 2.0 ** -60, TINY, SUB]))
    ln2 = mpmath.log(2)
    qs = list(range(-3, 4)) + [int(q) for q in rng.randint(-65400, 65500, size=120)]
    for q in qs:                                   # |x| <= 709.4: finite, normal results
        P.add("index_flip64", *around((q + mpf(0.5)) * ln2 / 64))
    qs = [-1022, -3, -2, -1, 0, 1, 2, 1022] + [int(q) for q in rng.randint(-1021, 1022, size=40)]
    for q in qs:
        P.add("index_flip1", *around((q + mpf(0.5)) * ln2))
    P.add("subnormal_result", -745.13, -708.4, *rng.uniform(-745.13, -708.4, 150))
    P.add("rounds_to_zero", -745.2)
    P.add("underflow", *rng.uniform(-1075.0, -746.0, 20))
    P.add("select_low", -1075.0, math.nextafter(-1075.0, -INF), -2000.0, -1e300, -INF)
    P.add("select_high_t", 709.78, 709.782712893384, 709.8, math.nextafter(709.8, INF))
    P.add("overflow", *rng.uniform(709.81, 1024.0, 10), 1024.0, math.nextafter(1024.0, INF), 1e4,
          1e300, INF)
    P.add("nan", NAN)
    P.add("random", *rng.uniform(-708.0, 709.7, 600))
    P.add("random", *rng.uniform(-40.0, 40.0, 200))
    P.add("random", *-(2.0 ** rng.uniform(-50, 9.4, 200)))
    return P


def build_log(rng):
    P = Points(1)
    for k in (0, -300, 700):
        for i in range(129):
            P.add("subinterval_edge", *[math.ldexp(v, k)
                                        for v in around(bits_to_double(LOG_OFF + (i << 45)))])
    one = [1.0, math.nextafter(1.0, 0.0), math.nextafter(1.0, 2.0), 1.0 - 2.0 ** -30,
           1.0 + 2.0 ** -30]
    P.add("near_one", *one)
    for k in (-1000, -1, 1, 1000):
        for z in (0.6875, 1.375):
            P.add("range_wrap", *around(math.ldexp(z, k)))
    P.add("extremes", TINY, HUGE)
    P.add("not_positive_normal", 0.0, -0.0, SUB, 5e-324, -1.5, -TINY, INF, -INF, NAN)
    P.add("random", *(2.0 ** rng.uniform(-1022, 1024, 600)))
    P.add("random", *rng.uniform(0.5, 2.0, 300))
    return P


def build_atan2(rng):
    P = Points(2)                                  # (y, x)
    for o in range(8):                             # octant o: angle in (o, o + 1) pi/4
        th = (o + rng.uniform(0.02, 0.98, 40)) * math.pi / 4
        rad = 2.0 ** rng.uniform(-8, 8, 40)
        P.add("octants", *zip(rad * np.sin(th), rad * np.cos(th)))
    for m in (1.0, 3.0, 2.0 ** -700, 1.2345e200):
        P.add("diagonal", *[(sy * m, sx * m) for sy in (1, -1) for sx in (1, -1)])

    def place(n, mn, mx):                          # the 8 arrangements of (mn, mx) in turn
        sy, sx = (1, -1)[n & 1], (1, -1)[(n >> 1) & 1]
        return (sy * mx, sx * mn) if (n >> 2) & 1 else (sy * mn, sx * mx)
    n = 0
    for mx in (1.0, 1.3720703125):
        for j in range(64):
            for mn in around(mpf(mx) * (j + mpf(0.5)) / 64):
                P.add("index_flip", place(n, mn, mx))
                n += 1
        for j in range(1, 65):
            P.add("index_exact", place(n, 1.0 * j / 64, 1.0))
            n += 1
    for mx in (1.0, 3.0, 1.7 * 2.0 ** 40):
        for mn in around(mpf(mx) * mpf(0.41421356237309503)):
            for k in range(4):
                P.add("pi8_switch", place(n + 2 * k, mn, mx))
            n += 1
    for e in (30, 300, 1000):
        a, b = 2.0 ** (e // 2), 2.0 ** (e // 2 - e)
        for k in range(8):
            P.add("ratios", place(k, 1.25 * b, a))
    P.add("axes", *[(sy * 0.0, sx) for sy in (1, -1) for sx in (1.0, -1.0, 2.5e10, -3e-200)])
    P.add("axes", *[(sy, 0.0) for sy in (1.0, -1.0, 4e100, -TINY)])
    P.add("zero_zero", *[(sy * 0.0, sx * 0.0) for sy in (1, -1) for sx in (1, -1)])
    P.add("x_negative_zero", *[(sy, -0.0) for sy in (1.0, -1.0, 4e100, -TINY)])
    P.add("nan", (NAN, 1.0), (1.0, NAN), (NAN, NAN), (NAN, 0.0))
    P.add("infinite", (INF, INF), (INF, -INF), (-INF, INF), (1.0, INF), (1.0, -INF), (INF, 1.0),
          (-INF, -2.0))
    mag = 2.0 ** rng.uniform(-20, 20, (500, 2)) * rng.choice([-1.0, 1.0], (500, 2))
    P.add("random", *zip(mag[:, 0], mag[:, 1]))
    # first octant away from the axis (x > 0, 1/4 < |y| / x <= 1): datan2_t's result there is the
    # table's hi + (atan t' + lo) with no quadrant step after it, so the table's lo shows
    t = rng.uniform(0.26, 1.0, 240)
    xs = 2.0 ** rng.uniform(-10, 10, 240)
    P.add("first_octant", *zip(t * xs * rng.choice([-1.0, 1.0], 240), xs))
    return P


def mantissas(rng, n):
    return [1.0, math.nextafter(1.0, 2.0), math.nextafter(2.0, 1.0)] + list(rng.uniform(1, 2, n))


def build_rcp(rng):
    P = Points(1)
    for e in (-1022, -1021, -500, -1, 0, 1, 500, 1021):
        P.add("mantissa_exponent", *pm([math.ldexp(m, e) for m in mantissas(rng, 12)]))
    P.add("mantissa_exponent", *pm([2.0 ** 1022]))
    P.add("random", *(2.0 ** rng.uniform(-1022, 1022, 400) * rng.choice([-1.0, 1.0], 400)))
    P.add("subnormal", *pm([5e-324, SUB, 2.0 ** -1023, math.nextafter(TINY, 0.0)]))
    P.add("huge", *pm([math.nextafter(2.0 ** 1022, INF), 1.5 * 2.0 ** 1022, 2.0 ** 1023, HUGE]))
    P.add("nan", NAN)
    return P


def build_sqrt(rng):
    P = Points(1)
    for e in (-1022, -1021, -501, -500, -1, 0, 1, 2, 500, 501, 1022, 1023):
        P.add("mantissa_exponent", *[math.ldexp(m, e) for m in mantissas(rng, 12)])
    P.add("four_minus_ulp", math.nextafter(4.0, 0.0))
    P.add("random", *(2.0 ** rng.uniform(-1022, 1024, 500)))
    P.add("zero_inf", 0.0, INF)
    P.add("nan", NAN)
    return P


def build_csqrt(rng):
    P = Points(2)                                  # (re, im)
    P.add("zero", (0.0, 0.0), (0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0))
    for a in (1.0, 2.0, 1e-300, 7.5e299, 0.3):
        P.add("negative_real", (-a, 0.0), (-a, -0.0))
        P.add("positive_real", (a, 0.0), (a, -0.0))
        P.add("pure_imaginary", (0.0, a), (0.0, -a), (-0.0, a), (-0.0, -a))
    for e in (30, 200, 600):                       # one part dominates
        P.add("lopsided", *[(sx * 1.3 * 2.0 ** (k * e), sy * 1.7 * 2.0 ** ((1 - k) * e - e // 2))
                            for k in (0, 1) for sx in (1, -1) for sy in (1, -1)])
    mag = 2.0 ** rng.uniform(-50, 50, (500, 2)) * rng.choice([-1.0, 1.0], (500, 2))
    P.add("random", *zip(mag[:, 0], mag[:, 1]))
    mag = rng.uniform(-4, 4, (200, 2))
    P.add("random", *zip(mag[:, 0], mag[:, 1]))
    return P


def build_cdiv(rng):
    P = Points(4)                                  # (a.re, a.im, b.re, b.im)
    a = rng.uniform(-3, 3, (40, 2))
    P.add("zero_divisor", *[(x, y, sx * 0.0, sy * 0.0) for (x, y), sx, sy in
                            zip(a[:8], (1, 1, -1, -1) * 2, (1, -1) * 4)], (0.0, 0.0, 0.0, 0.0))
    P.add("equal_parts", *[(x, y, s * 1.5 * (1 + i), 1.5 * (1 + i))
                           for i, ((x, y), s) in enumerate(zip(a[8:16], (1, -1) * 4))])
    P.add("real_divisor", *[(x, y, 0.7 * (i - 3.5), 0.0) for i, (x, y) in enumerate(a[16:24])])
    P.add("imaginary_divisor", *[(x, y, 0.0, 0.7 * (i - 3.5)) for i, (x, y) in enumerate(a[24:32])])
    m = rng.uniform(-4, 4, (300, 4))
    P.add("unit_scale", *map(tuple, m))
    m = 2.0 ** rng.uniform(-100, 100, (500, 4)) * rng.choice([-1.0, 1.0], (500, 4))
    P.add("random", *map(tuple, m))
    return P


def build_cdiv_rcp(rng):
    P = Points(4)
    th = rng.uniform(0, 2 * math.pi, 600)
    rad = 2.0 ** rng.uniform(-100, 100, 600)
    rad[:4] = 2.0 ** -100, 2.0 ** 100, 2.0 ** -99.5, 2.0 ** 99.5
    a = 2.0 ** rng.uniform(-60, 60, (600, 2)) * rng.choice([-1.0, 1.0], (600, 2))
    P.add("random", *zip(a[:, 0], a[:, 1], rad * np.cos(th), rad * np.sin(th)))
    m = rng.uniform(-4, 4, (200, 4))
    P.add("unit_scale", *map(tuple, m))
    return P


BUILDERS = {"sincos": (build_sincos, ("x",), t_sincos, 2), "exp": (build_exp, ("x",), t_exp, 1),
            "log": (build_log, ("x",), t_log, 1), "atan2": (build_atan2, ("x", "y"), t_atan2, 1),
            "rcp": (build_rcp, ("x",), t_rcp, 1), "sqrt": (build_sqrt, ("x",), t_sqrt, 2),
            "csqrt": (build_csqrt, ("x", "y"), t_csqrt, 2),
            "cdiv": (build_cdiv, ("x", "y", "bx", "by"), t_cdiv, 2),
            "cdiv_rcp": (build_cdiv_rcp, ("x", "y", "bx", "by"), t_cdiv, 2)}


def main():
    out = {}
    for g, (build, cols, truth, nout) in BUILDERS.items():
        P = build(np.random.RandomState(SEED + sum(map(ord, g))))
        rows = list(zip(*P.cols))
        res = [truth(*r) for r in rows]
        if nout == 1:
            res = [(r,) for r in res]
        for c, name in zip(P.cols, cols):
            out[f"{g}__{name}"] = np.array(c, dtype=np.float64)
        for k in range(nout):
            out[f"{g}__hi{k}"] = np.array([r[k][0] for r in res], dtype=np.float64)
            out[f"{g}__lo{k}"] = np.array([r[k][1] for r in res], dtype=np.float64)
        out[f"{g}__fam"] = np.array(P.fam, dtype=np.uint8)
        out[f"{g}__families"] = np.array(P.names)
        print(f"{g}: {len(rows)} points, families {P.names}")
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "math_truth.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
