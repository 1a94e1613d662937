"""The device special functions (csrc/device_math.hpp, csrc/kernels.hpp: inc_gamma_p_from_E, inc_gamma_inv, exp_fin, log_pos,
recip_fast, lgamma_pos, log_gamma_ratio, early_series) against tests/golden/special_functions.json -- 40-digit mpmath values
(tools/make_special_goldens.py) that share nothing with the CPU oracle -- through the public diagnostic entry points only.

Each golden block is one batch of n = 257 parcels (two workgroups, the second with one live lane) in planes of leading dimension
320; parcel i takes case i mod len(cases) of every mode, so neighbouring lanes sit in different branches and leave the four-term
convergence loops at different trip counts.  The padding columns of every output hold a NaN sentinel that must survive, and the
first 1 and the first 65 parcels run alone must give the bits they have inside the batch.

Bounds are the suite's own (tests/test_gpu_parity.py), none is new; beside each: what the CPU oracle measures against the same
goldens (tests/test_special_goldens_host.py) and what the device measured on an MI355X.

Nine plans, all created without plan-time compilation (specialize = -1: the diagnostics of plans of up to four modes are
ahead-of-time kernels, so a plan costs a constant block and a node table): the threshold x_t, the grid density and the
percentile are plan constants, and the issue's lists hold five x_t, three densities and eleven percentiles."""
import json
import os

import numpy as np
import pytest

from gpu_support import EPS, INF, TOL_QUAD, dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, LD = 257, 320
SUB = (1, 65)
TRI = [(p1, p2) for p1 in range(5) for p2 in range(p1, 5)]

#                                        bound      oracle vs goldens   device vs goldens (MI355X)
TOL_F = TOL_QUAD          # of M_p1 M_p2   1e-12      4.54e-15            5.71e-14
TOL_THR = 1e-12           # relative, x    1e-12      1.37e-13            8.65e-14
TOL_NQ = 1e-12            # of liq + rai   1e-12      2.78e-15            2.78e-15
TOL_SED = 1e-13           # relative       1e-13      9.26e-15            5.68e-15 (all of it in the Gamma mode: log_gamma_ratio)
TOL_COND = 1e-11          # relative       1e-11      9.35e-15            2.89e-15
TOL_CLOSURE = 4 * EPS     # relative       4 eps      1.43 eps            1.43 eps


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(ROOT, "tests", "golden", "special_functions.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def plans(gpu_cloudy, gold):
    """the nine plans of this file, made on first use and kept for the module"""
    cloudy, made = gpu_cloudy, {}

    def get(name):
        if name not in made:
            if name in gold["F"]["plans"]:
                p = gold["F"]["plans"][name]
                made[name] = cloudy.Plan(p["dist_types"], np.ones((3, 3)), p["x_t"] + [INF], (1.0, 1.0), 0,
                                         n_bins_per_log_unit=p["n_bins_per_log_unit"], specialize=-1)
            elif name in gold["thresholds"]["plans"]:
                made[name] = cloudy.Plan([1, 1, 1, 1], [[1.0]], gold["thresholds"]["plans"][name] + [1.0], (1.0, 1.0), 1,
                                         k_range=gold["thresholds"]["k_range"], specialize=-1)
            else:
                mp_ = gold["moment_plan"]
                vel = {"sed": ((1.0, 1 / 6),), "sed2": ((1.0, 1 / 6), (1.0, 0.5))}[name]
                made[name] = cloudy.Plan(mp_["dist_types"], [[1.0]], (INF,) * 4, mp_["norms"], 0, k_range=mp_["k_range"], vel=vel,
                                         specialize=-1)
        return made[name]

    return get


def fl(a):
    return np.array([float(v) for v in a])


def run_padded(cloudy, call, inp, out_rows):
    """call(n, ld, in_ptr, out_ptr) on the whole batch and on its first 1 and 65 parcels, in planes of leading dimension LD whose
    padding holds NaN: -> the (out_rows, N) result, after the sentinel and the sub-batch bits have been asserted"""
    buf = np.full((inp.shape[0], LD), np.nan)
    buf[:, :N] = inp
    src = dev(cloudy, buf)
    res = {}
    for n in (N,) + SUB:
        dst = dev(cloudy, np.full((out_rows, LD), np.nan))
        assert call(n, LD, src.ptr, dst.ptr) == 0, cloudy.lib().cloudy_last_error()
        o = dst.to_numpy()
        assert np.all(np.isnan(o[:, n:])), f"n = {n}: the padding columns were written"
        res[n] = o[:, :n]
    for n in SUB:
        assert np.array_equal(res[n], res[N][:, :n], equal_nan=True), f"the first {n} parcels alone differ from the batch"
    return res[N]


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_finite_2d_integrals_vs_goldens(gpu_cloudy, gold, plans, name):
    """get_finite_2d_integrals of Gamma and Exponential modes: the Simpson node sum in 40 digits (series and continued-fraction
    branches, their switch, the a E < 1e-18 exit, early_series regimes; three grid densities, both arms of the x_lb min)"""
    cloudy, L = gpu_cloudy, gpu_cloudy.lib()
    plan = plans(name)
    slots = [[c for c in gold["F"]["cases"] if c["plan"] == name and c["mode"] == m] for m in range(3)]
    assert all(0 < len(s) <= N for s in slots)
    pick = [[s[i % len(s)] for i in range(N)] for s in slots]
    cols = [tuple(np.array([c[key] for c in pk]) for key in ("n", "theta", "k")) for pk in pick]
    params = cloudy.pack_params(cols + [(np.ones(N), np.ones(N), np.ones(N))])
    F = run_padded(cloudy, lambda n, ld, a, b: L.cloudy_finite_2d_integrals(plan.handle, n, ld, a, b, None), params, 4 * 25)
    F = F.reshape(4, 5, 5, N)
    assert np.all(np.isfinite(F))
    assert np.array_equal(F, F.transpose(0, 2, 1, 3)), "mirrored entries differ"
    worst = 0.0
    for m in range(3):
        want = np.array([fl(c["F"]) for c in pick[m]]).T
        mm = np.array([fl(c["mm"]) for c in pick[m]]).T
        got = np.array([F[m, p1, p2] for p1, p2 in TRI])
        err = np.abs(got - want) / mm
        worst = max(worst, float(err.max()))
        assert np.all(err <= TOL_F), f"mode {m}: {err.max():.3e} at case {pick[m][int(err.max(axis=0).argmax())]['k']}"
    print(f"F plan {name}: {sum(map(len, slots))} cases, device max |F - golden| / (M_p1 M_p2) = {worst:.2e}")


@pytest.mark.parametrize("name", ["T0", "T1", "T2", "T3"])
def test_compute_thresholds_vs_goldens(gpu_cloudy, gold, plans, name):
    """compute_threshold(MovingThreshold) of Gamma modes: inc_gamma_inv from the staged start value and from the generic one,
    both tails, the tiny-k exits to the 1e-18 clamp, percentiles 0 and 1"""
    cloudy, L = gpu_cloudy, gpu_cloudy.lib()
    plan = plans(name)
    slots = [[c for c in gold["thresholds"]["cases"] if c["plan"] == name and c["mode"] == m] for m in range(3)]
    pick = [[s[(i + 5 * m) % len(s)] for i in range(N)] for m, s in enumerate(slots)]
    cols = [(np.ones(N), np.array([c["theta"] for c in pk]), np.array([c["k"] for c in pk])) for pk in pick]
    params = cloudy.pack_params(cols + [(np.ones(N), np.ones(N), np.ones(N))])
    thr = run_padded(cloudy, lambda n, ld, a, b: L.cloudy_compute_thresholds(plan.handle, n, ld, a, b, None), params, 4)
    assert np.all(np.isinf(thr[3]))
    worst = 0.0
    for m in range(3):
        want = np.array([float(c["x"]) for c in pick[m]])
        assert not np.isnan(thr[m]).any() and np.array_equal(np.isinf(thr[m]), np.isinf(want))
        fin = np.isfinite(want)
        err = np.abs(thr[m][fin] - want[fin]) / want[fin]
        if err.size:
            worst = max(worst, float(err.max()))
            i = int(err.argmax())
            assert np.all(err <= TOL_THR), f"p = {pick[m][0]['p']}: {err.max():.3e} at k = {np.array(cols[m][2])[fin][i]}"
    print(f"thresholds plan {name}: {sum(map(len, slots))} cases, device max relative error of x = {worst:.2e}")


def moment_batch(cases):
    return np.ascontiguousarray(np.array([cases[i % len(cases)]["mom"] for i in range(N)]).T), [cases[i % len(cases)] for i in range(N)]


def test_standard_N_q_vs_goldens(gpu_cloudy, gold, plans):
    """get_standard_N_q: P(k+1, z) by inc_gamma_p_from_E across its switch, P(k, z) from it, the erfc closed forms"""
    cloudy, L = gpu_cloudy, gpu_cloudy.lib()
    plan = plans("sed")
    mom, pick = moment_batch(gold["standard_N_q"]["cases"])
    cut = gold["moment_plan"]["size_cutoff"]
    q = run_padded(cloudy, lambda n, ld, a, b: L.cloudy_standard_N_q(plan.handle, n, ld, a, cut, b, None), mom, 4)
    assert np.all(np.isfinite(q))
    want = np.array([fl(c["out"]) for c in pick]).T
    tot = np.stack([want[0] + want[1]] * 2 + [want[2] + want[3]] * 2)
    err = np.abs(q - want) / tot
    print(f"standard_N_q: {len(gold['standard_N_q']['cases'])} cases, device max |diff| / (liq + rai) = {err.max():.2e}")
    assert np.all(err <= TOL_NQ), f"{err.max():.3e} at parcel {int(err.max(axis=0).argmax())}"


@pytest.mark.parametrize("key", ["sed", "sed2"])
def test_sedimentation_moments_vs_goldens(gpu_cloudy, gold, plans, key):
    """moment(dist, j - 1 + 1/6) (and + 1/2) of all four families through get_sedimentation_flux: log_gamma_ratio across its shift
    at k = 10 and down to k = eps.  The relative error of a Gamma moment is the absolute error of log_gamma_ratio plus that of
    exp_fin and of the closure inversion: this is the measurement behind the figures in the comments of device_math.hpp."""
    cloudy, L = gpu_cloudy, gpu_cloudy.lib()
    plan = plans(key)
    mom, pick = moment_batch(gold["fractional_moments"]["cases"])
    fx = run_padded(cloudy, lambda n, ld, a, b: L.cloudy_sedimentation_flux(plan.handle, n, ld, a, b, None), mom, 10)
    assert np.all(np.isfinite(fx))
    want = np.array([fl(c[key]) for c in pick]).T
    err = np.abs(fx - want) / np.abs(want)
    print(f"sedimentation ({key}): {len(gold['fractional_moments']['cases'])} cases, device max relative error = {err.max():.2e}"
          f" (Gamma mode: {err[2:5].max():.2e})")
    assert np.all(err <= TOL_SED), f"{err.max():.3e} at parcel {int(err.max(axis=0).argmax())}"


def test_condensation_moments_vs_goldens(gpu_cloudy, gold, plans):
    """3 (j - 1) moment(dist, j - 1 - 2/3) (4 pi/3)^(2/3) / 1000^(1/3) through get_cond_evap with xi = s = 1"""
    cloudy, L = gpu_cloudy, gpu_cloudy.lib()
    plan = plans("sed")
    mom, pick = moment_batch(gold["fractional_moments"]["cases"])
    ce = run_padded(cloudy, lambda n, ld, a, b: L.cloudy_cond_evap(plan.handle, n, ld, a, None, 1.0, 1.0, b, None), mom, 10)
    assert np.all(np.isfinite(ce))
    want = np.array([fl(c["cond"]) for c in pick]).T
    nz = want != 0.0
    assert np.all(ce[~nz] == 0.0) and nz.sum() == 6 * N
    err = np.abs(ce[nz] - want[nz]) / np.abs(want[nz])
    print(f"condensation: {len(gold['fractional_moments']['cases'])} cases, device max relative error = {err.max():.2e}")
    assert np.all(err <= TOL_COND)


def test_update_dist_from_moments_vs_goldens(gpu_cloudy, gold, plans):
    """the closure inversion of the Exponential, Gamma and Monodisperse modes against the exact inversion of the same moments,
    with the shape below, at and above either clamp"""
    cloudy, L = gpu_cloudy, gpu_cloudy.lib()
    plan = plans("sed")
    mom, pick = moment_batch(gold["closure"]["cases"])
    prm = run_padded(cloudy, lambda n, ld, a, b: L.cloudy_update_dist_from_moments(plan.handle, n, ld, a, b, None), mom, 12)
    got = prm[[0, 1, 2, 3, 4, 5, 9, 10, 11]]
    assert np.all(np.isfinite(prm))
    want = np.array([fl(c["params"]) for c in pick]).T
    err = np.abs(got - want) / want
    print(f"closure: {len(gold['closure']['cases'])} cases, device max relative error of (n, theta, k) = {err.max() / EPS:.2f} eps")
    assert np.all(err <= TOL_CLOSURE), f"{err.max() / EPS:.2f} eps at parcel {int(err.max(axis=0).argmax())}"
