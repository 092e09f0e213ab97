"""CPU checks of the parameter sensitivities against the 50-digit term-by-term truth of
tests/golden/param_sens_truth.json (written by tests/golden/make_param_sens_truth.py: the COS series
in mpmath, every parameter plane's term a central difference of the price's term at fixed [a, b], no
derivative formula): the NumPy restatement (tests/param_grad_reference.py) on every case and plane,
the fixture's composition, and four wrong restatements that the bars must refuse.

The unit of every bar is the fixture's `unit`: the series' absolute term sum of that case and plane
(e^{-rT} sum_k |term_k|).  Bar per plane and key (the group for A, B, C, E; N for D):

    |restatement - truth| <= max(10 restatement_worst[plane][key], 10 * 2^-52) unit

10x the restatement's worst error on the machine that generated the fixture, tests/test_param_grad.py's
factor for libm differences between hosts.  The bars are per plane because the restatement's fp64
error is: the kappa/sigma/rho chain cancels inside each term, so kappa2 sits at 37,000 * 2^-52 of
the unit (8.3e-12), the price at 5 to 34 (Accuracy).  The generator's condition keeps
every entry at or below 1e-9; a wrong factor or sign is 1e-3 to 1 in this unit.

At N = 1 the thirteen parameter planes have truth 0 and unit 0 (term 0 does not move with a
parameter: phi(0) = 1), and no entry in restatement_worst: the restatement's residue there is held
to 10 * 2^-52 unit_price plane_ratio[i], the plane's natural size beside the price."""
import functools
import json
import os

import numpy as np
import pytest

import greeks_reference as G
import param_grad_reference as R
from oracle import dh_oracle as O

EPS = 2.0 ** -52
FACTOR = 10.0


@functools.lru_cache(maxsize=None)
def fixture():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                           "param_sens_truth.json")) as fh:
        return json.load(fh)


def key_of(c):
    return str(c["N"]) if c["group"] == "D" else c["group"]


def cpu_bar(c):
    """[14]: the bar of case c per plane in units of its `unit`; nan where the plane has no entry
    (the parameter planes at N = 1)."""
    worst = fixture()["restatement_worst"]
    return np.array([max(FACTOR * worst[name][key_of(c)], FACTOR * EPS)
                     if key_of(c) in worst[name] else np.nan for name in R.PLANES])


def evaluate(cases):
    """[n, 14]: R.sens_vec (looked up at call time: the sensitivity test patches the module) on the
    stored range of each case."""
    fix = fixture()
    return np.array([R.sens_vec(fix["sets"][c["set"]], c["S0"], c["K"], c["T"], c["r"],
                                c["is_call"], c["N"], c["q"], ab=(c["a"], c["b"])) for c in cases])


@functools.lru_cache(maxsize=None)
def restatement():
    return evaluate(fixture()["cases"])


def over_bar(got, cases):
    """[n, 14] bool: where |got - truth| exceeds the CPU bar (planes without one never do)."""
    truth = np.array([c["truth"] for c in cases])
    unit = np.array([c["unit"] for c in cases])
    bar = np.array([cpu_bar(c) for c in cases])
    with np.errstate(invalid="ignore"):
        return ~np.isnan(bar) & ~(np.abs(got - truth) <= bar * unit)


def test_fixture_composition():
    fix = fixture()
    cases, sets = fix["cases"], fix["sets"]
    assert tuple(fix["planes"]) == R.PLANES and len(sets) == 10
    assert abs(sets[6][12] - 1e-3) < 1e-15                                   # sigma_j small
    assert sets[7][4] == -0.9 and sets[7][9] == 0.9                          # |rho| = 0.9
    for s, muj in ((8, -0.05), (9, -0.02)):                                  # x = 0 but mu_j
        assert sets[s] == [1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, muj, 1.0]
    count = {g: sum(c["group"] == g for c in cases) for g in "ABCDE"}
    assert count == {"A": 72, "B": 16, "C": 36, "D": 56, "E": 36}
    assert {c["set"] for c in cases if c["group"] == "A"} == {0, 5, 6, 7}
    assert {c["set"] for c in cases if c["group"] == "C"} == {0, 1, 2}
    assert {c["set"] for c in cases if c["group"] == "D"} == {0, 6}
    assert {c["N"] for c in cases if c["group"] in "ABE"} == {128}
    assert {c["N"] for c in cases if c["group"] == "C"} == {256}
    assert {c["N"] for c in cases if c["group"] == "D"} == {1, 2, 17, 65, 336, 337, 1024}
    assert {(c["set"], c["S0"], c["r"], c["q"]) for c in cases if c["group"] == "B"} == \
        {(1, 80.0, 0.01, 0.02), (2, 125.0, 0.05, 0.0)}
    assert {(c["set"], c["S0"], c["r"], c["q"]) for c in cases if c["group"] == "E"} == \
        {(8, 97.0, 0.02, 0.0), (9, 103.5, 0.04, 0.0)}
    for s in range(3):             # each set's tile of group C holds both kinds of option
        flags = [c["clamp"] for c in cases if c["group"] == "C" and c["set"] == s]
        assert len(flags) == 12 and any(flags) and not all(flags), (s, flags)
    assert not any(c["clamp"] for c in cases if c["group"] != "C")
    # the stored range and flag are the oracle's of today (to 4 ulps: another libm may round apart)
    for c in cases:
        prm = sets[c["set"]]
        a, b = O.trunc_range(prm, c["S0"], c["K"], c["T"], c["r"])
        assert abs(a - c["a"]) <= 4 * np.spacing(abs(a)) and abs(b - c["b"]) <= 4 * np.spacing(b)
        assert c["clamp"] == G.clamp_active(prm, c["S0"], c["K"], c["T"], c["r"])
        assert len(c["truth"]) == len(c["unit"]) == 14
        assert all(abs(t) <= u for t, u in zip(c["truth"], c["unit"]))
        assert c["unit"][0] > 0
        if c["N"] == 1:            # term 0 alone: exactly zero, whatever the parameter
            assert not any(c["truth"][1:]) and not any(c["unit"][1:])
        else:
            assert all(u > 0 for u in c["unit"])
        assert ("mkt" in c) == (c["group"] == "E")
    # group E's market prices: the truth price moved by 2 % of a standard normal draw
    z = np.random.RandomState(77).randn(36)
    e_cases = [c for c in cases if c["group"] == "E"]
    assert [c["mkt"] for c in e_cases] == [c["truth"][0] * (1 + 0.02 * zi)
                                           for c, zi in zip(e_cases, z)]
    # the generator's own condition, and the keys the bars are looked up by
    keys = {key_of(c) for c in cases}
    for i, name in enumerate(R.PLANES):
        assert set(fix["restatement_worst"][name]) == (keys if i == 0 else keys - {"1"}), name
        assert max(fix["restatement_worst"][name].values()) <= 1e-9
    two = [c for c in cases if c["group"] == "D" and c["N"] == 2]
    assert len(two) == 8 and len(fix["plane_ratio"]) == 14 and fix["plane_ratio"][0] == 1.0
    assert fix["plane_ratio"] == [float(np.median([c["unit"][i] / c["unit"][0] for c in two]))
                                  for i in range(14)]


def test_restatement_matches_truth_on_every_case_and_plane():
    fix = fixture()
    cases = fix["cases"]
    got = restatement()
    truth = np.array([c["truth"] for c in cases])
    unit = np.array([c["unit"] for c in cases])
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(got - truth) / unit
    keys = np.array([key_of(c) for c in cases])
    for i, name in enumerate(R.PLANES):
        print(f"{name:9s} worst |restatement - truth| / unit: " + "  ".join(
            f"{k}: {np.nanmax(rel[keys == k, i]):.2e}" for k in dict.fromkeys(keys)
            if not (k == "1" and i > 0)))
    bad = np.argwhere(over_bar(got, cases))
    assert bad.size == 0, [(cases[i], R.PLANES[j], got[i, j], truth[i, j]) for i, j in bad]
    # N = 1: the parameter planes against their natural size beside the price
    ratio = np.array(fix["plane_ratio"])
    for i, c in enumerate(cases):
        if c["N"] == 1:
            assert np.isfinite(got[i]).all(), (c, got[i])
            assert np.all(np.abs(got[i, 1:]) <= FACTOR * EPS * c["unit"][0] * ratio[1:]), (c, got[i])


def test_price_plane_is_price_vec_on_every_case():
    fix = fixture()
    for c, row in zip(fix["cases"], restatement()):
        assert row[0] == O.price_vec(fix["sets"][c["set"]], c["S0"], c["K"], c["T"], c["r"],
                                     c["is_call"], c["N"], c["q"]), c              # bit for bit


# ---- four wrong restatements the bars must refuse ------------------------------------------------
def factor_derivs_copy(u, tau, v0, kappa, theta, sigma, rho, sigma_uu=True):
    """param_grad_reference.factor_derivs, restated so that the sigma chain's (d^2)' can lose its
    2 sigma uu term; with sigma_uu=True it gives the original's bits (asserted below)."""
    B, _ = O._heston_factor(u, tau, kappa, theta, sigma, rho)
    beta = kappa - rho * sigma * 1j * u
    uu = u * (u + 1j)
    d = np.sqrt(beta ** 2 + sigma ** 2 * uu)
    bm, bp = beta - d, beta + d
    e = np.exp(-d * tau)
    D = bp - bm * e
    c = kappa * theta / sigma ** 2
    inner = bm * tau - 2 * np.log(D / (2 * d))

    def chain(bq, d2q, cq):
        dq = d2q / (2 * d)
        bmq, bpq = bq - dq, bq + dq
        eq = -tau * dq * e
        Dq = bpq - bmq * e - bm * eq
        Bq = -uu * (-eq * D - (1 - e) * Dq) / D ** 2
        Aq = cq * inner + c * (bmq * tau - 2 * (Dq / D - dq / d))
        return Aq + Bq * v0

    d_kappa = chain(1.0, 2 * beta, theta / sigma ** 2)
    d2_sigma = 2 * beta * (-1j * rho * u) + (2 * sigma * uu if sigma_uu else 0.0)
    d_sigma = chain(-1j * rho * u, d2_sigma, -2 * kappa * theta / sigma ** 3)
    d_rho = chain(-1j * sigma * u, 2 * beta * (-1j * sigma * u), 0.0)
    return B, d_kappa, (kappa / sigma ** 2) * inner, d_sigma, d_rho


def _sigma_chain_without_uu(monkeypatch):
    monkeypatch.setattr(R, "factor_derivs", functools.partial(factor_derivs_copy, sigma_uu=False))


def _mu_without_compensator(monkeypatch):
    right = R.log_cf_derivs

    def wrong(u, tau, prm):
        out = list(right(u, tau, prm))
        lam, muj, sj = prm[10], prm[11], prm[12]
        out[11] = lam * tau * 1j * u * np.exp(1j * u * muj - 0.5 * sj ** 2 * u ** 2)
        return tuple(out)

    monkeypatch.setattr(R, "log_cf_derivs", wrong)


def _theta_divided_by_theta(monkeypatch):
    right = R.factor_derivs

    def wrong(u, tau, v0, kappa, theta, sigma, rho):
        B, dk, dt, ds, dr = right(u, tau, v0, kappa, theta, sigma, rho)
        return B, dk, dt / theta, ds, dr

    monkeypatch.setattr(R, "factor_derivs", wrong)


def _k0_not_halved(monkeypatch):
    right = R.sens_vec

    def wrong(prm, S0, K, T, r, is_call, N=128, q=0.0, L=10.0, ab=None, extended=False):
        # the N = 1 series is the halved term 0: adding it once more leaves term 0 whole
        return right(prm, S0, K, T, r, is_call, N, q, L, ab, extended) + \
            right(prm, S0, K, T, r, is_call, 1, q, L, ab, extended)

    monkeypatch.setattr(R, "sens_vec", wrong)


WRONG = {
    "sigma-chain-without-2-sigma-uu": (_sigma_chain_without_uu, ("sigma1", "sigma2")),
    "mu_j-without-its-compensator": (_mu_without_compensator, ("mu_j",)),
    "theta-divided-by-theta": (_theta_divided_by_theta, ("theta1", "theta2")),
    "k0-not-halved": (_k0_not_halved, ("price",)),
}


def test_the_copy_the_wrong_sigma_chain_is_made_from_is_the_restatement():
    u = np.arange(1, 40) * 0.37
    for a, b in zip(R.factor_derivs(u, 0.7, 0.04, 2.0, 0.05, 0.3, -0.6),
                    factor_derivs_copy(u, 0.7, 0.04, 2.0, 0.05, 0.3, -0.6)):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()


@pytest.mark.parametrize("name", list(WRONG))
def test_a_wrong_restatement_exceeds_the_bar_on_group_a(monkeypatch, name):
    """Group A under each of four wrong restatements, patched into param_grad_reference: every
    plane the mistake touches leaves its bar on every case of the group, and no other plane does."""
    patch, planes = WRONG[name]
    cases = [c for c in fixture()["cases"] if c["group"] == "A"]
    right = evaluate(cases)
    assert not over_bar(right, cases).any()
    patch(monkeypatch)
    got = evaluate(cases)
    over = over_bar(got, cases)
    truth = np.array([c["truth"] for c in cases])
    unit = np.array([c["unit"] for c in cases])
    touched = [R.PLANES.index(p) for p in planes]
    for i in touched:
        print(f"{name}: {R.PLANES[i]} off by {np.min(np.abs(got[:, i] - truth[:, i]) / unit[:, i]):.2e}"
              f" to {np.max(np.abs(got[:, i] - truth[:, i]) / unit[:, i]):.2e} of the unit, "
              f"bar {cpu_bar(cases[0])[i]:.2e}")
        assert over[:, i].all(), (name, R.PLANES[i])
    others = [i for i in range(14) if i not in touched]
    assert not over[:, others].any()
    if name != "k0-not-halved":    # whose term 0 leaves a rounding residue on the parameter planes
        assert got[:, others].tobytes() == right[:, others].tobytes()
