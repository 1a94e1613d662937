"""GPU tests of cloudy_parcel_tsit5_adaptive (csrc/adaptive_thermo.hpp): per-parcel adaptive Tsit5 of the adiabatic parcel.  The
reference is the NumPy restatement tsit5_restated.adaptive_tsit5 (without and with t_save) with plane_norms = (1, 1, 1, 1, the
plan's mom_norms) on the restated right-hand side of test_parcel_host (tests/test_parcel_adaptive_host.py holds the batches and measures the
restatement on them), and a reltol = 1e-11 run of the same restatement.

Run with `-m gpu`.  Batch sizes 1, 65 and 257 in buffers of leading dimension n + 15."""
import functools

import numpy as np
import pytest

import test_parcel_adaptive_host as A
import test_tsit5_adaptive_host as H
from gpu_support import (INF, SENTINEL, SIZES, adaptive_call, bits_equal, dev, driver_case, is_blank, make_case, mass_rows, same_counts,
                         two_gamma_plan)
from tsit5_restated import adaptive_tsit5, plane_norms, save_times

pytestmark = pytest.mark.gpu

KEYS = ("u", "t", "dt", "accepted", "rejected", "status")
COAL, COND = 1, 2


@functools.lru_cache(maxsize=None)
def plan_of(cloudy, oracle, types, kc=((1.0,),), thr=None, norms=A.NORMS, dtype=0, specialize=0):
    types = list(types)
    par, op, _ = make_case(cloudy, oracle, types, [list(r) for r in kc], thr or (INF,) * len(types), norms)
    return par, op, par.coal_data.plan(types, dtype=dtype, specialize=specialize)


def parcel_adaptive(cloudy, plan, y0, w, t_span, sources=COND, **kw):
    """w: a float, or an array (through w_dev)"""
    return adaptive_call("cloudy_parcel_tsit5_adaptive", cloudy, plan, y0, t_span, sources=sources, forcing=w, **kw)


def parity(got, ref, tight, y0, n, what):
    """the rule of item 1: <= 5 % of the parcels differ from the restatement in (accepted, rejected); the others agree per plane to
    1e-11 x evaluations of |y0| + |want|; every parcel, plane by plane, is within 2 x the restatement's own error + 1e-12 of the
    tight reference"""
    same = same_counts(got, ref)
    rel = A.rel_to(got["u"], ref["u"], y0) / ref["evals"]
    worst = rel[:, same].max()
    where = np.unravel_index(np.argmax(np.where(same[None, :], rel, 0.0)), rel.shape)
    print(f"{what}: the worst agreement is plane {where[0]} of parcel {where[1]} ({ref['accepted'][where[1]]} accepted, "
          f"{ref['rejected'][where[1]]} rejected steps); per plane {rel[:, same].max(axis=1)}")
    ref_each, each = A.rel_to(ref["u"], tight["u"], y0), A.rel_to(got["u"], tight["u"], y0)
    ref_err, err = ref_each.max(axis=1), each.max(axis=1)
    print(f"{what}: {(~same).sum()} of {n} parcels differ in (accepted, rejected); the others agree to {worst:.2e} x evaluations; "
          f"against the reltol = 1e-11 run: restatement {ref_err}, device {err}")
    assert (~same).sum() <= 0.05 * n, (~same).sum()
    assert worst <= A.TOL_EVAL, worst
    assert np.all(each <= 2 * ref_each + 1e-12), (each - 2 * ref_each).max()


# ---- 1. decision parity
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("reltol", H.TOLS)
def test_decision_parity_on_the_decade_batch(gpu_cloudy, oracle, reltol, n):
    """out of place, w through w_dev, ld = n + 15: the parity rule; status 0, t == t_span bit for bit, M0 has the input's bits,
    padding columns and the input untouched.  (The reference's right-hand side is monodisperse_cond_closed: the automatic first
    step reaches states with M1 <= 0, where the device follows update_dist_from_moments' empty distribution.)"""
    cloudy = gpu_cloudy
    _, _, plan = plan_of(cloudy, oracle, (2,))
    y0, w, ref = A.decade_case(n, reltol, plan=True)
    got = parcel_adaptive(cloudy, plan, y0, w, A.T_SPAN, reltol=reltol, ld=n + 15)
    assert np.all(ref["status"] == 0) and np.all(got["status"] == 0) and np.all(got["t"] == A.T_SPAN)
    parity(got, ref, A.decade_tight(n, plan=True), y0, n, f"decade batch reltol={reltol:g} n={n}")
    assert bits_equal(got["u"][4], y0[4])
    assert np.all(is_blank(got["pad"])) and np.array_equal(got["u_in"], got["buf"])


def test_decision_parity_with_coalescence(gpu_cloudy, oracle):
    """COAL | COND on the two-Gamma batch of the host test, n = 257: the same rule (the tight reference at reltol = 1e-11)."""
    cloudy = gpu_cloudy
    n = 257
    _, _, plan = plan_of(cloudy, oracle, (1, 1), tuple(map(tuple, A.GOLOVIN)))
    y0, w, ref = A.two_gamma_case(n)
    _, _, tight = A.two_gamma_case(n, 1e-11)
    got = parcel_adaptive(cloudy, plan, y0, w, A.COAL_T, sources=COAL | COND, ld=n + 15)
    assert np.all(got["status"] == 0) and np.all(got["t"] == A.COAL_T)
    parity(got, ref, tight, y0, n, "COAL | COND n=257")
    assert not bits_equal(got["u"][4], y0[4])
    assert np.all(is_blank(got["pad"])) and np.array_equal(got["u_in"], got["buf"])


# ---- 2. dense output
def test_dense_output(gpu_cloudy, oracle):
    """the twelve save times on the decade batch (n = 257): y_out, dt, t and info have the bits of the call without snapshots; the
    snapshot at 0 has the input's bits, the one at t_span y_out's; the snapshots of the parcels with the restatement's counts agree
    with adaptive_tsit5(t_save) to 1e-11 x evaluations; padding untouched."""
    cloudy = gpu_cloudy
    n = 257
    _, _, plan = plan_of(cloudy, oracle, (2,))
    y0, w, ref = A.decade_case(n, 1e-6, saveat=True, plan=True)
    base = parcel_adaptive(cloudy, plan, y0, w, A.T_SPAN, ld=n + 15)
    got = parcel_adaptive(cloudy, plan, y0, w, A.T_SPAN, times=save_times(A.T_SPAN), ld=n + 15)
    for k in KEYS:
        assert bits_equal(got[k], base[k]), k
    assert np.all(got["status"] == 0) and np.isfinite(got["saved"]).all()
    assert bits_equal(got["saved"][0], y0) and bits_equal(got["saved"][-1], got["u"])
    assert bits_equal(got["saved"][:, 4], np.broadcast_to(y0[4], (12, n)))
    assert np.all(is_blank(got["saved_pad"])) and np.all(is_blank(got["pad"]))
    same = same_counts(got, ref)
    assert (~same).sum() <= 0.05 * n, (~same).sum()
    rel = np.abs(got["saved"] - ref["saved"]) / np.maximum(np.abs(y0)[None] + np.abs(ref["saved"]), 1e-300) / ref["evals"][None, None, :]
    worst = rel[:, :, same].max()
    print(f"dense output: {(~same).sum()} parcels differ in (accepted, rejected); the snapshots of the others agree to {worst:.2e} x evaluations")
    assert worst <= A.TOL_EVAL, worst


def test_rogers_series_from_one_launch(gpu_cloudy, oracle):
    """the monodisperse driver case, 41 save times 0.5 k, one launch: within the Rogers bounds of the host tests"""
    cloudy = gpu_cloudy
    _, _, plan = plan_of(cloudy, oracle, (2,))
    y0, ts = A.rogers_states()
    got = parcel_adaptive(cloudy, plan, y0, 10.0, A.T_SPAN, times=ts)
    assert got["status"][0] == 0
    d_ss, d_r = A.rogers_from_series(ts, got["saved"][:, :, 0])
    print(f"device dense output vs Rogers 1975: supersaturation {d_ss:.4f} percentage points, radius {d_r:.4f} um")
    assert d_ss <= 0.12 and d_r <= 0.05, (d_ss, d_r)


# ---- 3. budget
def test_budget_leaves_nan_beyond_the_time_reached(gpu_cloudy, oracle):
    cloudy = gpu_cloudy
    n = 257
    _, _, plan = plan_of(cloudy, oracle, (2,))
    y0, w = A.decade_batch(n)
    ts = save_times(A.T_SPAN)
    got = parcel_adaptive(cloudy, plan, y0, w, A.T_SPAN, times=ts, max_steps=3, ld=n + 15)
    slow = got["status"] == 1
    assert 0 < slow.sum() < n and np.all(got["status"][~slow] == 0) and np.all(got["t"][slow] < A.T_SPAN)
    beyond = ts[:, None] > got["t"][None, :]
    assert beyond[:, slow].any() and (~beyond[:, slow]).any() and not beyond[:, ~slow].any()
    nan, fin = np.isnan(got["saved"]), np.isfinite(got["saved"])
    assert np.all(nan.all(axis=1) == beyond) and np.all(fin.all(axis=1) == ~beyond)
    assert np.all(is_blank(got["saved_pad"]))


# ---- 4. warm start and in place
def test_warm_start_and_in_place(gpu_cloudy, oracle):
    cloudy = gpu_cloudy
    n = 257
    _, _, plan = plan_of(cloudy, oracle, (2,))
    y0, w, ref = A.decade_case(n, 1e-6, plan=True)
    tight = A.decade_tight(n, plan=True)
    first = parcel_adaptive(cloudy, plan, y0, w, A.T_SPAN / 2, in_place=True)
    assert np.all(first["status"] == 0) and np.all(first["dt"] > 0)
    probe = parcel_adaptive(cloudy, plan, first["u"], w, A.T_SPAN / 2, dt_in=first["dt"], max_steps=1, in_place=True)
    took = probe["accepted"] == 1   # the first proposed step is the dt the first call returned (where it was accepted whole)
    inside = took & (first["dt"] < A.T_SPAN / 2 * (1 - 1e-12))
    assert inside.any() and np.all(probe["t"][inside] == first["dt"][inside])
    second = parcel_adaptive(cloudy, plan, first["u"], w, A.T_SPAN / 2, dt_in=first["dt"], in_place=True)
    assert np.all(second["status"] == 0)
    ref_err, err = A.rel_to(ref["u"], tight["u"], y0).max(axis=1), A.rel_to(second["u"], tight["u"], y0).max(axis=1)
    print(f"two half calls against the reltol = 1e-11 run: {err}; the restatement's single call: {ref_err}")
    assert np.all(err <= 2 * ref_err + 1e-12), (err, ref_err)


# ---- 5. batch independence
def test_batch_independence(gpu_cloudy, oracle):
    cloudy = gpu_cloudy
    n = 257
    _, _, plan = plan_of(cloudy, oracle, (2,))
    y0, w = A.decade_batch(n)
    ts = save_times(A.T_SPAN)
    whole = parcel_adaptive(cloudy, plan, y0, w, A.T_SPAN, times=ts)
    attempts = whole["accepted"] + whole["rejected"]
    for i in (int(np.argmax(attempts)), int(np.argmin(attempts)), 0, 63, 64, 255, 256):
        part = parcel_adaptive(cloudy, plan, np.ascontiguousarray(y0[:, i:i + 1]), w[i:i + 1], A.T_SPAN, times=ts)
        for k in KEYS:
            assert bits_equal(whole[k][..., i:i + 1], part[k]), (k, i)
        assert bits_equal(whole["saved"][:, :, i:i + 1], part["saved"]), i


# ---- 6. served and refused
@pytest.mark.parametrize("name", ["gamma", "mixture"])
def test_driver_plans_with_the_oracle_tendency(gpu_cloudy, oracle, name):
    """a Gamma plan and an Exponential + Gamma plan with COND, n = 65, N and w spread as in the decade batch: the parity rule with
    the moments' tendency from the oracle"""
    cloudy = gpu_cloudy
    n = 65
    types, mom = driver_case(name)
    rows = mass_rows(types)
    _, op, plan = plan_of(cloudy, oracle, tuple(types))
    N, w = A.decade_draws(n)
    moms = np.array(mom)[:, None] * (N / 2e8)[None, :]
    y0 = np.ascontiguousarray(np.vstack([A.thermo_rows(moms[rows].sum(axis=0)), moms]))
    norms = np.concatenate([np.ones(4), plane_norms(tuple(3 if t in (1, 3) else 2 for t in types), A.NORMS)])
    rhs = A.oracle_rhs(oracle, op, w, rows, False)
    run = lambda tol: adaptive_tsit5(rhs, y0, A.T_SPAN, dict(reltol=tol, abstol=1e-9, max_steps=10000, plane_norms=norms))  # noqa: E731
    ref, tight = run(1e-6), run(1e-11)
    got = parcel_adaptive(cloudy, plan, y0, w, A.T_SPAN, ld=n + 15)
    assert np.all(ref["status"] == 0) and np.all(got["status"] == 0) and np.all(got["t"] == A.T_SPAN)
    parity(got, ref, tight, y0, n, name)
    number = [4 + r - 1 for r in rows]
    assert bits_equal(got["u"][number], y0[number]) and np.all(is_blank(got["pad"]))


def test_served_and_refused(gpu_cloudy, oracle):
    """A NumericalCoalStyle plan serves COND.  COAL | COND on cfg3b (a fixed threshold), on a two-Gamma plan with a fixed threshold,
    on a MovingThreshold plan and on a NumericalCoalStyle plan, CLOUDY_F32 planes and a plan without plan-time compilation answer
    CLOUDY_EUNSUPPORTED naming the stage-by-stage alternative; outputs keep their sentinel bits."""
    import bench

    cloudy = gpu_cloudy
    L, E = cloudy.lib(), cloudy._lib
    n = 65
    y0, w = A.two_gamma_batch(n)
    numerical = cloudy.NumericalPlan([1, 1], cloudy.LinearKernelFunction(5e-3), bench.NORMS, 10, quad_mode=cloudy.QUAD_FIXED)
    got = parcel_adaptive(cloudy, numerical, y0, w, A.COAL_T, ld=n + 15)
    assert np.all(got["status"] == 0) and np.all(got["t"] == A.COAL_T) and bits_equal(got["u"][[4, 7]], y0[[4, 7]])
    golovin = tuple(map(tuple, A.GOLOVIN))
    _, _, thresholded = plan_of(cloudy, oracle, (1, 1), golovin, (5e-9, INF), bench.NORMS)
    spec = bench.workload_spec("cfg3b")
    assert spec["n_modes"] == 2 and np.isfinite(spec["thresholds"]).any()
    par_b, _, _ = make_case(cloudy, oracle, [1, 1], bench.kernel_matrix(spec), spec["thresholds"], bench.NORMS)
    cfg3b = par_b.coal_data.plan([1, 1])
    _, _, moving = two_gamma_plan(cloudy, oracle, "moving")
    _, _, f32 = plan_of(cloudy, oracle, (1, 1), golovin, None, A.NORMS, 1)
    _, _, aot = plan_of(cloudy, oracle, (1, 1), golovin, None, A.NORMS, 0, -1)
    ts = save_times(1.0)
    for what, plan, sources in (("cfg3b", cfg3b, COAL | COND), ("thresholds", thresholded, COAL | COND), ("moving", moving, COAL | COND),
                                ("numerical", numerical, COAL | COND), ("F32", f32, COND), ("specialize = -1", aot, COND)):
        got = parcel_adaptive(cloudy, plan, y0, w, 1.0, sources=sources, times=ts, expect=E.EUNSUPPORTED)
        msg = L.cloudy_last_error().decode()
        assert "stage by stage" in msg and "cloudy_cond_evap" in msg, (what, msg)
        assert np.all(is_blank(got["saved_bits"])) and np.all(is_blank(got["u"])), what
        assert not got["accepted"].any() and np.all(got["t"].view(np.uint64) == SENTINEL)


# ---- 7. the Python wrapper
def test_python_wrapper(gpu_cloudy, oracle):
    cloudy = gpu_cloudy
    n = 257
    par, _, plan = plan_of(cloudy, oracle, (2,))
    y0, w = A.decade_batch(n)
    ts = save_times(A.T_SPAN)
    want = parcel_adaptive(cloudy, plan, y0, w, A.T_SPAN, times=ts)
    w_d = dev(cloudy, w[None, :])
    y = dev(cloudy, y0)
    acc, rej, status, t = cloudy.solve_parcel_tsit5_adaptive(par, y, w_d, A.T_SPAN, info=True)
    assert bits_equal(y.to_numpy(), want["u"]) and not status.any() and np.all(t == A.T_SPAN)
    assert np.array_equal(acc, want["accepted"]) and np.array_equal(rej, want["rejected"])
    y = dev(cloudy, y0)
    saved = cloudy.solve_parcel_tsit5_adaptive(par, y, w_d, A.T_SPAN, times=ts)
    assert bits_equal(saved.to_numpy().reshape(len(ts), 6, n), want["saved"]) and bits_equal(y.to_numpy(), want["u"])
    with pytest.raises(RuntimeError, match=r"of 257 parcels did not reach t_span; the first is parcel \d+"):
        cloudy.solve_parcel_tsit5_adaptive(par, dev(cloudy, y0), w_d, A.T_SPAN, max_steps=2, info=True)
