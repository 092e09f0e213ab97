"""GPU checks of the analytic COS Greeks (csrc/dh_greeks.h) against the 50+-digit
truth of tests/golden/greeks_truth.json: every case and plane through dh_greeks_pairs, the clamp
groups through a surface tile that mixes the table pass with the per-term way, strikes within a few
ulps of the clamp's boundary, the dynamic-LDS cap on fresh contexts, and gamma's call/put symmetry.

Unit.  Every bar is in the fixture's `unit` of the case and plane: the series' absolute term sum
e^{-rT} sum_k |term_k| (tests/golden/make_greeks_truth.py), so a value at rounding level is held to
the rounding of the sum that made it.

Bar (device_bar).  The reference is the NumPy restatement's own fp64 error against the truth,
restatement_worst[plane][N] of the fixture, measured by the generator.  The device gets 16x that --
the factor tests/test_gpu_param_grad.py grants the device over the restatement's fp64 error: the
device's table-driven primitives are good to a few ulp where libm gives under one, and its sums run
in another order -- and never less than 16 * 2^-52 of the unit, so that a plane on which the
restatement happens to be exact does not demand exactness.  Nothing here is set from the device's
output.  Measured on an MI355X (worst |device - truth| / unit over the cases of each N):

    N            1        2        65       128      256      1080, 1081, 2048
    price        1.8e-16  1.7e-16  7.4e-17  1.5e-15  4.3e-15  1.8e-16
    delta        2.0e-16  1.4e-16  1.9e-16  1.5e-15  1.2e-15  1.4e-16
    gamma        0        0        6.0e-16  1.2e-15  2.3e-15  8.0e-16
    dual_delta   1.2e-16  1.2e-16  3.4e-16  1.2e-15  1.4e-15  2.7e-16
    vega1        0        8.6e-16  8.4e-16  1.4e-14  5.5e-15  8.4e-16
    vega2        0        1.9e-16  1.8e-15  1.7e-15  3.2e-15  1.6e-15

against bars of 3.6e-15 (the floor) to 1.3e-13: the device is inside every one by a factor of 4 or
more, and no bar was moved (Accuracy, has the restatement's figures beside these).
"""
import functools
import json
import os

import numpy as np
import pytest

import greeks_reference as G

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
MARGIN = 16.0


@pytest.fixture(scope="module")
def native():
    from dhcos import _native
    if _native.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return _native


@functools.lru_cache(maxsize=None)
def fixture():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                           "greeks_truth.json")) as fh:
        return json.load(fh)


def device_bar(N):
    """[6]: the bar per plane at series length N, in units of the case's `unit`."""
    worst = fixture()["restatement_worst"]
    return np.array([max(MARGIN * worst[name][str(N)], MARGIN * EPS) for name in G.PLANES])


def select(pred):
    """(indices, records [n, 16], K, T, is_call, truth [6, n], unit [6, n]) of the cases pred picks."""
    fix = fixture()
    idx = [i for i, c in enumerate(fix["cases"]) if pred(c)]
    cs = [fix["cases"][i] for i in idx]
    rec = np.array([fix["sets"][c["set"]] + [c["S0"], c["r"], c["q"]] for c in cs])
    return (idx, rec, np.array([c["K"] for c in cs]), np.array([c["T"] for c in cs]),
            np.array([c["is_call"] for c in cs]), np.array([c["truth"] for c in cs]).T,
            np.array([c["unit"] for c in cs]).T)


def same_bits(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a).tobytes() == \
        np.ascontiguousarray(b).tobytes()


def assert_truth(got, truth, unit, N, label):
    """got, truth, unit [6, n]: |got - truth| <= device_bar(N) * unit, the worst printed first."""
    bar = device_bar(N)
    err = np.abs(got - truth)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(unit > 0, err / unit, np.where(err == 0, 0.0, np.inf))
    print(f"{label} N={N}: worst |device - truth| / unit  " + "  ".join(
        f"{name} {rel[g].max():.2e} (bar {bar[g]:.2e})" for g, name in enumerate(G.PLANES)))
    ok = err <= bar[:, None] * unit
    assert ok.all(), (label, N, [(G.PLANES[g], int(i), got[g, i], truth[g, i], unit[g, i])
                                 for g, i in np.argwhere(~ok)])


_PAIRS = {}


def pairs_of(native, N):
    """The device's planes [6, n] of every fixture case of series length N, in the fixture's order:
    one Context.greeks_pairs call per N, shared among the tests."""
    if N not in _PAIRS:
        _, rec, K, T, call, _, _ = select(lambda c: c["N"] == N)
        _PAIRS[N] = native.default_context().greeks_pairs(rec, K, T, call, N)
    return _PAIRS[N]


# ---- d. the LDS cap (first in the file: see the docstring) ---------------------------------------
def test_lds_cap_is_raised_on_a_fresh_context_in_either_order(native):
    """greeks_lds_bytes is 49,104 B at N = 1080 and 49,184 B at N = 1081: the launch crosses the
    48 KiB default cap of dynamic LDS between them, and the first request past it raises the
    kernel's cap, once per context.  On a fresh Context the first Greeks request is N = 1081, then
    1080, then 128; on a second fresh Context the order is reversed.  Each result is held to the
    truth (group D), and N = 128 and N = 1080 give the same bits on both.  The kernel's attribute
    belongs to the process, so the raise itself is new only in the first such request of a process;
    this test stands first in its file so that it makes that request when the file runs alone or
    first.  The N = 1080 and 1081 requests are group D's four options, the N = 128 request is the
    88 pairs of groups A and B."""
    sel = {N: select(lambda c, N=N: c["N"] == N) for N in (128, 1080, 1081)}
    results = []
    for order in ((1081, 1080, 128), (128, 1080, 1081)):
        ctx = native.Context(native.default_context().device)
        try:
            results.append({N: ctx.greeks_pairs(*sel[N][1:5], N) for N in order})
        finally:
            ctx.close()
    for which, res in enumerate(results):
        for N in (128, 1080, 1081):
            assert_truth(res[N], sel[N][5], sel[N][6], N, f"fresh context {which}")
    for N in (128, 1080, 1081):
        assert same_bits(results[0][N], results[1][N]), N


# ---- a. device against truth ---------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 65, 128, 256, 1080, 1081, 2048])
def test_pairs_match_truth_on_every_case_and_plane(native, N):
    """Groups A and B at N = 128 (88 pairs, per-pair market data among them), C at 256 (36, clamped
    and not), D at each of its six lengths (4 each)."""
    idx, _, _, _, _, truth, unit = select(lambda c: c["N"] == N)
    assert len(idx) == {128: 88, 256: 36}.get(N, 4)
    assert_truth(pairs_of(native, N), truth, unit, N, "pairs")


@pytest.mark.parametrize("s", [0, 1, 2])
def test_surface_tile_of_clamped_and_unclamped_options(native, s):
    """Groups A's and C's T = 0.1 options of one parameter set on one surface: 18 options in one
    tile, of which the table pass takes those on the tile's range and the per-term way the
    clamp-widened ones (the restatement's flags are asserted mixed).  At N = 128 and at N = 256 the
    surface gives the bits of the pairs form; the A options are held to truth at 128, C's at 256."""
    idx, rec, K, T, call, truth, unit = select(
        lambda c: c["set"] == s and c["T"] == 0.1 and c["group"] in "AC")
    cases = [fixture()["cases"][i] for i in idx]
    flags = [c["clamp"] for c in cases]
    assert len(cases) == 18 and any(flags) and not all(flags)
    ctx = native.default_context()
    surf = native.Surface(ctx, K, T, call)
    try:
        assert surf.n_tiles == 1
        for N, group in ((128, "A"), (256, "C")):
            got = surf.greeks(rec[:1], N)
            assert got.shape == (6, 1, 18)
            assert same_bits(got[:, 0], ctx.greeks_pairs(rec, K, T, call, N)), N
            m = np.array([c["group"] == group for c in cases])
            assert m.sum() == (6 if group == "A" else 12)
            assert_truth(got[:, 0][:, m], truth[:, m], unit[:, m], N, f"surface set {s} group {group}")
    finally:
        surf.close()


# ---- c. the clamp's boundary ---------------------------------------------------------------------
def test_strikes_within_ulps_of_the_clamp_boundary(native):
    """The clamp decision is xK - 0.1 < a0 || xK + 0.1 > b0, with xK from the device's own log and
    (a0, b0) from its own cumulants: a strike a few ulps from the boundary may take the table pass
    on the device and count as clamped in the restatement, or the reverse.  Both must still agree,
    because there a = a0 (b = b0) either way.  Under the demo set at T = 0.1, N = 256: the strikes
    S0 exp(a0 + 0.1) and S0 exp(b0 - 0.1) moved by j ulps, j = -4 ... 4, each as a call and as a put:
    36 options in one tile.  The restatement's flag is asserted mixed over each group of nine.
    Every device plane is within device_bar(256) of the restatement, in the fp64 unit
    greeks_reference.term_sums (held to the fixture's by tests/test_greeks_truth.py); and
    neighbouring strikes of one type differ by no more than that bar plus the restatement's own
    neighbour difference -- which fails if the two branches disagree."""
    fix = fixture()
    prm, S0, r, T, N = fix["sets"][0], 100.0, 0.03, 0.1, 256
    a0, b0 = G.unclamped_range(prm, T, r)
    groups = []
    for centre in (S0 * np.exp(a0 + 0.1), S0 * np.exp(b0 - 0.1)):
        ks = [centre]
        for _ in range(4):
            ks = [np.nextafter(ks[0], 0.0)] + ks + [np.nextafter(ks[-1], np.inf)]
        groups.append(np.array(ks))
    for ks in groups:
        flags = [G.clamp_active(prm, S0, k, T, r) for k in ks]
        print("clamp_active over the nine strikes:", "".join("x" if f else "." for f in flags))
        assert len(ks) == 9 and any(flags) and not all(flags), flags
    K = np.tile(np.concatenate(groups), 2)                      # 18 calls, then 18 puts
    call = np.repeat([True, False], 18)
    want = np.array([[G.greeks_vec(prm, S0, k, T, r, c, N)[n] for k, c in zip(K, call)]
                     for n in G.PLANES])
    unit = np.array([[G.term_sums(prm, S0, k, T, r, c, N)[n] for k, c in zip(K, call)]
                     for n in G.PLANES])
    rec = np.array([prm + [S0, r, 0.0]])
    surf = native.Surface(native.default_context(), K, np.full(36, T), call)
    try:
        assert surf.n_tiles == 1
        got = surf.greeks(rec, N)[:, 0]
    finally:
        surf.close()
    bar = device_bar(N)[:, None] * unit
    err = np.abs(got - want)
    print("boundary: worst |device - restatement| / unit  " + "  ".join(
        f"{n} {np.max(err[g] / unit[g]):.2e}" for g, n in enumerate(G.PLANES)))
    assert (err <= bar).all(), [(G.PLANES[g], int(i)) for g, i in np.argwhere(~(err <= bar))]
    for lo in range(0, 36, 9):                                  # a group of nine of one type
        sl = slice(lo, lo + 9)
        step = np.abs(np.diff(got[:, sl], axis=1))
        allowed = np.maximum(bar[:, sl][:, 1:], bar[:, sl][:, :-1]) + \
            np.abs(np.diff(want[:, sl], axis=1))
        assert (step <= allowed).all(), (lo, [(G.PLANES[g], int(i))
                                              for g, i in np.argwhere(~(step <= allowed))])


# ---- e. gamma does not know the option's type ----------------------------------------------------
@pytest.mark.parametrize("N, group", [(128, "A"), (256, "C")])
def test_gamma_has_the_same_bits_for_a_call_and_a_put(native, N, group):
    """Gamma's accumulator (sum of Re(w_k) cos(u_k (xK - a))) and its output factor do not depend on
    the option's type: for equal (set, K, T) the device's gamma is bit-equal between call and put,
    on the table pass (group A, and C's unclamped strikes) and the per-term way (C's clamped)."""
    cases = fixture()["cases"]
    idx = [i for i, c in enumerate(cases) if c["N"] == N]
    gamma = pairs_of(native, N)[G.PLANES.index("gamma")]
    at = {}
    for j, i in enumerate(idx):
        c = cases[i]
        if c["group"] == group:
            at.setdefault((c["set"], c["K"], c["T"]), {})[c["is_call"]] = (j, c["clamp"])
    assert len(at) == (36 if group == "A" else 18)
    ways = set()
    for key, both in at.items():
        (jc, clamp), (jp, _) = both[True], both[False]
        ways.add(clamp)
        assert gamma[jc].tobytes() == gamma[jp].tobytes(), (key, gamma[jc], gamma[jp])
    assert ways == ({False} if group == "A" else {False, True})
