"""The CPU oracle against tests/golden/special_functions.json (40-digit mpmath values, tools/make_special_goldens.py).

The oracle is the reference of nearly every device test, and it is double precision with hand-written incomplete-gamma
routines of its own: here each of its special-function paths is pinned to values that share nothing with it.  Bounds are the
suite's (tests/test_gpu_parity.py): TOL_QUAD = 1e-12 of M_p1 M_p2 for F, 1e-12 relative for thresholds, 1e-12 of the total for
get_standard_N_q, 1e-13 / 1e-11 relative for the sedimentation / condensation moments, 4 eps for the closure inversion.
(co_gamma_inc_p is reached through moment_source_helper, get_standard_N_q and the inversion.)  Each test prints what it
measured; tests/test_gpu_special_goldens.py quotes these maxima next to its own bounds.

With mpmath installed, every tenth case of every block is regenerated and compared with the file."""
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(np.float64).eps)
TOL_QUAD = 1e-12
TRI = [(p1, p2) for p1 in range(5) for p2 in range(p1, 5)]
MODES = (0, 1, 3, 2)


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(ROOT, "tests", "golden", "special_functions.json")) as f:
        return json.load(f)


def fl(a):
    return np.array([float(v) for v in a])


def oracle_dists(oracle, mom, k_range):
    m = [mom[0:2], mom[2:5], mom[5:8], mom[8:10]]
    return [oracle.update_dist_from_moments(t, mi, k_range) for t, mi in zip(MODES, m)]


def test_moment_source_helper_vs_goldens(oracle, gold):
    worst = 0.0
    for c in gold["F"]["cases"]:
        pl = gold["F"]["plans"][c["plan"]]
        d = oracle.make_dist(pl["dist_types"][c["mode"]], c["n"], c["theta"], c["k"])
        mm, want = fl(c["mm"]), fl(c["F"])
        for t, (p1, p2) in enumerate(TRI):
            h = oracle.moment_source_helper(d, p1, p2, pl["x_t"][c["mode"]], pl["n_bins_per_log_unit"])
            got = min(h, oracle.moment(d, p1) * oracle.moment(d, p2))
            assert np.isfinite(got)
            worst = max(worst, abs(got - want[t]) / mm[t])
    print(f"F: {len(gold['F']['cases'])} cases, oracle max |F - golden| / (M_p1 M_p2) = {worst:.2e}")
    assert worst <= TOL_QUAD


def test_compute_threshold_and_gamma_inc_inv_vs_goldens(oracle, gold):
    worst = 0.0
    for c in gold["thresholds"]["cases"]:
        want = float(c["x"])
        got = oracle.compute_threshold(oracle.make_dist(1, 1.0, c["theta"], c["k"]), c["p"])
        if np.isinf(want):
            assert got == want
            continue
        assert np.isfinite(got)
        worst = max(worst, abs(got - want) / want)
        if want > 1e-18 and c["theta"] * oracle.gamma_inc_inv(c["k"], c["p"]) > 1e-18:
            assert c["theta"] * oracle.gamma_inc_inv(c["k"], c["p"]) == got
    print(f"thresholds: {len(gold['thresholds']['cases'])} cases, oracle max relative error of x = {worst:.2e}")
    assert worst <= 1e-12


def test_standard_N_q_vs_goldens(oracle, gold):
    mp_ = gold["moment_plan"]
    worst = 0.0
    for c in gold["standard_N_q"]["cases"]:
        got = oracle.get_standard_N_q(oracle_dists(oracle, c["mom"], mp_["k_range"]), mp_["size_cutoff"])
        want = fl(c["out"])
        tot = np.array([want[0] + want[1]] * 2 + [want[2] + want[3]] * 2)
        assert np.all(np.isfinite(got))
        worst = max(worst, float((np.abs(got - want) / tot).max()))
    print(f"standard_N_q: {len(gold['standard_N_q']['cases'])} cases, oracle max |diff| / (liq + rai) = {worst:.2e}")
    assert worst <= 1e-12


def test_fractional_moments_vs_goldens(oracle, gold):
    mp_ = gold["moment_plan"]
    ws = wc = 0.0
    for c in gold["fractional_moments"]["cases"]:
        pd = oracle_dists(oracle, c["mom"], mp_["k_range"])
        for key, vel in (("sed", [(1.0, 1 / 6)]), ("sed2", [(1.0, 1 / 6), (1.0, 0.5)])):
            got, want = oracle.get_sedimentation_flux(pd, vel), fl(c[key])
            assert np.all(np.isfinite(got)) and np.all(want < 0.0)
            ws = max(ws, float((np.abs(got - want) / np.abs(want)).max()))
        got, want = oracle.get_cond_evap(pd, 1.0, 1.0), fl(c["cond"])
        nz = want != 0.0
        assert np.all(got[~nz] == 0.0) and np.all(np.isfinite(got)) and nz.sum() == 6
        wc = max(wc, float((np.abs(got[nz] - want[nz]) / np.abs(want[nz])).max()))
    n = len(gold["fractional_moments"]["cases"])
    print(f"fractional moments: {n} cases, oracle max relative error: sedimentation {ws:.2e}, condensation {wc:.2e}")
    assert ws <= 1e-13 and wc <= 1e-11


def test_update_dist_from_moments_vs_goldens(oracle, gold):
    mp_ = gold["moment_plan"]
    worst = 0.0
    for c in gold["closure"]["cases"]:
        pd = oracle_dists(oracle, c["mom"], mp_["k_range"])
        got = np.array([v for i in (0, 1, 3) for v in (pd[i].n, pd[i].theta, pd[i].k)])
        want = fl(c["params"])
        assert np.all(np.isfinite(got)) and np.all(want > 0.0)
        worst = max(worst, float((np.abs(got - want) / np.abs(want)).max()))
    print(f"closure: {len(gold['closure']['cases'])} cases, oracle max relative error of (n, theta, k) = {worst / EPS:.2f} eps")
    assert worst <= 4 * EPS


def test_file_matches_its_generator(gold):
    """every tenth case of every block regenerated (fixed subsample): the file and tools/make_special_goldens.py cannot drift"""
    mp = pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("make_special_goldens", os.path.join(ROOT, "tools", "make_special_goldens.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)

    def same(a, b):
        if isinstance(a, list):
            return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        if isinstance(a, str) and a[0] in "-0123456789i":
            x, y = mp.mpf(a), mp.mpf(b)
            return x == y or abs(x - y) <= mp.mpf(10) ** -30 * abs(y)
        return a == b

    for name, make in gen.BLOCKS.items():
        stored = gold[name]["cases"]
        pick = list(range(0, len(stored), 10))
        fresh = make(only=set(pick))
        assert len(fresh) == len(pick)
        for i, f in zip(pick, fresh):
            assert f.keys() == stored[i].keys()
            assert all(same(f[k], stored[i][k]) for k in f), (name, i)
