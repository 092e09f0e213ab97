"""CPU checks of the analytic COS Greeks against a 50+-digit truth: the NumPy restatement
(tests/greeks_reference.py) on every case and plane of tests/golden/greeks_truth.json (written by
tests/golden/make_greeks_truth.py: the COS series in mpmath, every Greek a term-by-term central
difference at fixed [a, b], no derivative formula), the fixture's shape, and the clamped values
DESIGN.md 3.17 quotes.

The unit of every bar is the fixture's `unit`: the series' absolute term sum of that case and plane
(e^{-rT} sum_k |term_k|).  A value at rounding level (the clamped put K = 40: delta -9.08e-10, unit
0.17) is thereby held to the rounding of the sum that produced it, not to a floor picked by hand.

Bar: |restatement - truth| <= 64 * 2^-52 * unit.  A condition, not a measurement: the fp64
restatement sums N products of a few correctly rounded library calls each, so it stays within a few
2^-52 of the unit (measured: 37 * 2^-52 at worst, vega1 at N = 128, where the reference's
(beta - d) / sigma^2 cancels; 6 * 2^-52 on delta, gamma and dual delta), while a wrong sign or
factor in any plane is an error of order 1 in this unit."""
import functools
import json
import os

import numpy as np
import pytest

import greeks_reference as G
from oracle import dh_oracle as O

BAR = 64 * 2.0 ** -52


@functools.lru_cache(maxsize=None)
def fixture():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                           "greeks_truth.json")) as fh:
        return json.load(fh)


def case_args(fix, c):
    return fix["sets"][c["set"]], c["S0"], c["K"], c["T"], c["r"], c["is_call"], c["N"], c["q"]


@functools.lru_cache(maxsize=None)
def restatement():
    """[cases, 6]: greeks_vec on every case of the fixture, computed once."""
    fix = fixture()
    out = np.empty((len(fix["cases"]), len(G.PLANES)))
    for i, c in enumerate(fix["cases"]):
        g = G.greeks_vec(*case_args(fix, c))
        out[i] = [g[name] for name in G.PLANES]
    return out


def test_fixture_shape():
    fix = fixture()
    cases = fix["cases"]
    assert tuple(fix["planes"]) == G.PLANES and len(fix["sets"]) == 4
    assert fix["sets"][3][4] == -0.9 and fix["sets"][3][9] == 0.9
    count = {g: sum(c["group"] == g for c in cases) for g in "ABCD"}
    assert count == {"A": 72, "B": 16, "C": 36, "D": 24}
    assert {c["N"] for c in cases if c["group"] in "AB"} == {128}
    assert {c["N"] for c in cases if c["group"] == "C"} == {256}
    assert {c["N"] for c in cases if c["group"] == "D"} == {1, 2, 65, 1080, 1081, 2048}
    assert {(c["S0"], c["r"], c["q"]) for c in cases if c["group"] == "B"} == \
        {(80.0, 0.01, 0.02), (125.0, 0.05, 0.0)}
    for s in range(3):             # each set's tile of group C holds both kinds of option
        flags = [c["clamp"] for c in cases if c["group"] == "C" and c["set"] == s]
        assert len(flags) == 12 and any(flags) and not all(flags), (s, flags)
    assert not any(c["clamp"] for c in cases if c["group"] != "C")
    # the stored range and flag are the oracle's of today (to 4 ulps: another libm may round apart)
    for c in cases:
        prm = fix["sets"][c["set"]]
        a, b = O.trunc_range(prm, c["S0"], c["K"], c["T"], c["r"])
        assert abs(a - c["a"]) <= 4 * np.spacing(abs(a)) and abs(b - c["b"]) <= 4 * np.spacing(b)
        assert c["clamp"] == G.clamp_active(prm, c["S0"], c["K"], c["T"], c["r"])
        assert len(c["truth"]) == len(c["unit"]) == 6
        assert all(abs(t) <= u for t, u in zip(c["truth"], c["unit"]))
    for name in G.PLANES:          # the generator's own condition
        assert set(fix["restatement_worst"][name]) == {str(c["N"]) for c in cases}
        assert max(fix["restatement_worst"][name].values()) <= BAR


def test_restatement_matches_truth_on_every_case_and_plane():
    fix = fixture()
    got = restatement()
    truth = np.array([c["truth"] for c in fix["cases"]])
    unit = np.array([c["unit"] for c in fix["cases"]])
    err = np.abs(got - truth)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(unit > 0, err / unit, np.where(err == 0, 0.0, np.inf))
    ns = np.array([c["N"] for c in fix["cases"]])
    for i, name in enumerate(G.PLANES):
        print(f"{name:10s} worst |restatement - truth| / unit: " + "  ".join(
            f"N={n}: {rel[ns == n, i].max():.2e}" for n in sorted(set(ns))))
    bad = np.argwhere(~(err <= BAR * unit))
    assert bad.size == 0, [(fix["cases"][i], G.PLANES[j], got[i, j], truth[i, j]) for i, j in bad]


def test_term_sums_is_the_fixture_unit():
    """greeks_reference.term_sums, the fp64 sum of |terms| tests/test_gpu_greeks_truth.py uses where
    it leaves the fixture's cases, against the 80-digit one: to 1e-9 relative.  The unit only scales
    a bar, so a part in 1e9 of it is beyond notice; every |term| is a few roundings from its exact
    value relative to the term's amplitude, and the amplitudes sum to the unit's size."""
    fix = fixture()
    worst = 0.0
    for c in fix["cases"]:
        got = G.term_sums(*case_args(fix, c))
        for name, u in zip(G.PLANES, c["unit"]):
            if u == 0.0:
                assert got[name] == 0.0
                continue
            worst = max(worst, abs(got[name] / u - 1))
            assert abs(got[name] - u) <= 1e-9 * u, (c, name, got[name], u)
    print(f"term_sums against the fixture's unit: worst relative difference {worst:.2e}")


def test_greeks_vec_price_is_price_vec_on_every_case():
    fix = fixture()
    got = restatement()
    for i, c in enumerate(fix["cases"]):
        prm, S0, K, T, r, call, N, q = case_args(fix, c)
        assert got[i, 0] == O.price_vec(prm, S0, K, T, r, call, N, q), c      # bit for bit


# The fixed-range caveat's examples: the reference demo's parameters, T = 0.1,
# S0 = 100, N = 256, clamp active.  (K, is_call, plane) -> the value as the document prints it.
QUOTED = [
    (40.0, False, "delta", -9.08e-10),
    (40.0, False, "gamma", 2.30e-10),
    (250.0, True, "delta", 2.04e-12),
    (250.0, True, "gamma", 6.82e-13),
]


@pytest.mark.parametrize("K, is_call, plane, quoted", QUOTED,
                         ids=[f"{'call' if q[1] else 'put'}-K{q[0]:g}-{q[2]}" for q in QUOTED])
def test_clamped_values_quoted_in_the_design_document(K, is_call, plane, quoted):
    """The truth rounds to the three digits DESIGN.md 3.17 prints, and the restatement holds them."""
    fix = fixture()
    (i, c), = [(i, c) for i, c in enumerate(fix["cases"]) if c["group"] == "C" and c["set"] == 0
               and c["K"] == K and c["is_call"] == is_call]
    j = G.PLANES.index(plane)
    assert c["clamp"]
    assert float(f"{c['truth'][j]:.2e}") == quoted
    assert abs(restatement()[i, j] - c["truth"][j]) <= BAR * c["unit"][j]
