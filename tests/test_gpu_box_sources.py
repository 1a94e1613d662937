"""GPU tests of cloudy_box_ssprk33_steps (csrc/box_sources.hpp): fused SSPRK33 box stepping with the condensation source alone
(the drivers condensation_single_gamma.jl / condensation_exp_gamma.jl) and with coalescence + condensation.  The stepping
reference is OrdinaryDiffEq's SSPRK33 formulas (_ssprk33_host) driven by the unchanged oracle:
oracle.rhs_coal_batch(op, u) + oracle.rhs_condensation_batch(op, xi, s, u).

Run with `-m gpu`.  The setups (seeds, step sizes) are picked on the oracle alone; tools in this file that need no device
(`oracle_reference`, `regular`) are what the picks were made with."""

import numpy as np
import pytest

import bench
from gpu_support import (INF, SENTINEL, TOL_POLY, TOL_QUAD, _ssprk33_host, blank, dev, make_case, many_mode_moments, mixed_moments, oracle_reference,
                         rel_err)

pytestmark = pytest.mark.gpu

XI = 1e-8


def regular(mom, want):
    """the regular parcels of test_fused_ssprk33_batch_vs_oracle_stepping: finite and within a factor 10 of their initial state"""
    with np.errstate(all="ignore"):
        return np.isfinite(want).all(axis=0) & (np.abs(want[:3]) <= 10 * np.abs(mom[:3]) + 1e-300).all(axis=0)


def supersaturation(n):
    return np.random.default_rng(0).uniform(-0.02, 0.05, n)


def box_steps(cloudy, plan, u_in, u_out, n, ld, sources, s, dt, n_steps, xi=XI):
    """the C entry point itself: s a float or a DeviceArray"""
    s_ptr, s_val = (s.ptr, 0.0) if isinstance(s, cloudy.DeviceArray) else (None, float(s))
    return cloudy.lib().cloudy_box_ssprk33_steps(plan.handle, n, ld, u_in.ptr, u_out.ptr, sources, s_ptr, s_val, xi, dt, n_steps, None)


@pytest.mark.parametrize("driver", ["condensation_single_gamma", "condensation_exp_gamma"])
def test_condensation_drivers_in_one_launch(gpu_cloudy, oracle, driver):
    """condensation_single_gamma.jl:17-28 (Gamma(1e8, 1e-10, 1)) and condensation_exp_gamma.jl:14-31 (Exponential + Gamma):
    norms (1e6, 1e-9), s = 0.05, xi = 1e-8, solve(prob, SSPRK33(), dt = 10) over 12 steps, 64 identical columns, sources = COND.
    Against the oracle stepping at 1e-11 (the bound of the condensation right-hand side per evaluation; the state moves by
    20-30 % in total), against the device's own rhs_condensation called stage by stage at 1e-13 (the bound
    test_cfg1_single_box_trajectory_ssprk33 uses for that comparison); number planes unchanged."""
    cloudy = gpu_cloudy
    if driver == "condensation_single_gamma":
        dist_types, u1, number, ratios = [1], [1e8, 1e-2, 2e-12], [0], {1: 1.20269725, 2: 1.28870769}
    else:
        dist_types, u1, number, ratios = [0, 1], [1e8, 1e-2, 1e7, 1e-2, 2e-11], [0, 2], {1: 1.20000348, 3: 1.04218602, 4: 1.0570408}
    par, op, _ = make_case(cloudy, oracle, dist_types, [[1.0]], (INF,) * len(dist_types), bench.NORMS)
    plan = par.coal_data.plan(dist_types)
    u0 = np.tile(np.array(u1)[:, None], (1, 64))
    dt, n_steps, s = 10.0, 12, 0.05
    want = oracle_reference(oracle, op, u0, dt, n_steps, XI, s, False, True)
    for row, r in ratios.items():   # (the oracle's own end state, as recorded when the test was written)
        assert want[row, 0] / u0[row, 0] == pytest.approx(r, rel=1e-8)
    u = dev(cloudy, u0)
    assert cloudy.solve_box_ssprk33(par, u, dt, n_steps, XI, s, coal=False) is u
    got = u.to_numpy()
    assert np.all(got == got[:, :1])
    print(f"{driver}: max rel err vs oracle stepping {np.abs(got / want - 1).max():.2e}")
    assert np.allclose(got, want, rtol=1e-11, atol=0)

    def device_rhs(x):
        dm = cloudy.DeviceArray.zeros(*x.shape)
        cloudy.rhs_condensation(plan, dm, dev(cloudy, x), XI, s)
        return dm.to_numpy()

    staged = _ssprk33_host(device_rhs, u0, dt, n_steps)
    print(f"{driver}: max rel err vs the staged device right-hand side {np.abs(got / staged - 1).max():.2e}")
    assert np.allclose(got, staged, rtol=1e-13, atol=0)
    assert np.allclose(got[number], u0[number], rtol=1e-15, atol=0)


def test_condensation_only_batch_four_closure_families(gpu_cloudy, oracle):
    """Exponential, Gamma, Monodisperse and Lognormal modes, 300 parcels in buffers of leading dimension 320, a supersaturation
    per parcel, 2 steps out of place: padding and input untouched, n_steps = 0 the identity, regular parcels against the oracle."""
    cloudy = gpu_cloudy
    dist_types = [0, 1, 2, 3]
    n, ld, dt, n_steps = 300, 320, 1e-3, 2
    par, op, _ = make_case(cloudy, oracle, dist_types, [[1.0]], (INF,) * 4, bench.NORMS)
    plan = par.coal_data.plan(dist_types)
    mom = mixed_moments(dist_types, n, seed=12)   # (300 of 300 regular on the oracle)
    s = supersaturation(n)
    want = oracle_reference(oracle, op, mom, dt, n_steps, XI, s, False, True)
    ok = regular(mom, want)
    assert ok.sum() >= 0.9 * n, ok.sum()
    nm = mom.shape[0]
    buf = np.full((nm, ld), 7.0)
    buf[:, :n] = mom
    s_dev = dev(cloudy, s[None, :])
    u_in = dev(cloudy, buf)
    u_out = dev(cloudy, blank(nm, ld))
    cloudy._lib.check(box_steps(cloudy, plan, u_in, u_out, n, ld, cloudy.SRC_COND, s_dev, dt, n_steps))
    got = u_out.to_numpy()
    assert np.all(got[:, n:].view(np.uint64) == SENTINEL), "the padding columns were written"
    assert np.array_equal(u_in.to_numpy(), buf), "the input changed"
    err = rel_err(got[:, :n], want, mom, ok)
    print(f"condensation only, four closure families: {ok.sum()} regular parcels of {n}, max rel err {err.max():.2e}")
    assert err.max() < 1e-11, err.max()
    u_zero = dev(cloudy, blank(nm, ld))
    cloudy._lib.check(box_steps(cloudy, plan, u_in, u_zero, n, ld, cloudy.SRC_COND, s_dev, dt, 0))
    z = u_zero.to_numpy()
    assert np.array_equal(z[:, :n], mom) and np.all(z[:, n:].view(np.uint64) == SENTINEL)


@pytest.fixture(scope="module")
def workload_runs(gpu_cloudy, oracle):
    """cfg3a / cfg3b, 400 parcels, 4 steps: the oracle stepping with both sources, the device's coalescence-only and combined
    results -- computed once for the tests below"""
    cloudy = gpu_cloudy
    runs = {}
    for name in ("cfg3a", "cfg3b"):
        n, dt, n_steps = 400, 1e-3, 4
        wl = bench.make_workload(name, n, seed=31)
        op = bench.oracle_params(name)
        s = supersaturation(n)
        plan = wl["coal_data"].plan(wl["dist_types"])
        u_coal = dev(cloudy, wl["mom"])
        cloudy.solve_ssprk33(wl["par"], u_coal, dt, n_steps)
        u_both = dev(cloudy, wl["mom"])
        cloudy.solve_box_ssprk33(wl["par"], u_both, dt, n_steps, XI, dev(cloudy, s[None, :]))
        runs[name] = dict(wl=wl, op=op, s=s, plan=plan, n=n, dt=dt, n_steps=n_steps, coal=u_coal.to_numpy(), both=u_both.to_numpy(),
                          want=oracle_reference(oracle, op, wl["mom"], dt, n_steps, XI, s, True, True))
    return runs


@pytest.mark.parametrize("name,tol", [("cfg3a", TOL_POLY), ("cfg3b", TOL_QUAD)])
def test_combined_sources_vs_oracle_stepping(workload_runs, name, tol):
    """coalescence + condensation on the all-Inf and the thresholded bench workload against the oracle stepping, with the mask,
    the error measure and the bound of test_fused_ssprk33_batch_vs_oracle_stepping; and the condensation term is really there:
    the combined result differs from cloudy_ssprk33_steps' by what the oracle says it should (median 7.1e-8 / 2.0e-7)."""
    r = workload_runs[name]
    mom, want, got = r["wl"]["mom"], r["want"], r["both"]
    ok = regular(mom, want)
    assert ok.sum() >= 0.9 * r["n"], ok.sum()
    err = rel_err(got, want, mom, ok)
    print(f"{name}: fused coalescence + condensation vs oracle stepping, {ok.sum()} regular parcels, max rel err {err.max():.2e}")
    assert err.max() < max(1e3 * tol, 1e-9), err.max()
    shift = np.abs(got - r["coal"])[:, ok] / np.maximum((np.abs(mom) + np.abs(want))[:, ok], 1e-300)
    print(f"{name}: median |combined - coalescence only| / (|u0| + |u|) = {np.median(shift):.2e}")
    assert np.median(shift) > 1e-8, np.median(shift)


@pytest.mark.parametrize("name", ["cfg3a", "cfg3b"])
def test_coalescence_alone_is_cloudy_ssprk33_steps(gpu_cloudy, workload_runs, name):
    """sources = COAL forwards to the cloudy_ssprk33_steps path: the same bits."""
    cloudy = gpu_cloudy
    r = workload_runs[name]
    u = dev(cloudy, r["wl"]["mom"])
    cloudy.solve_box_ssprk33(r["wl"]["par"], u, r["dt"], r["n_steps"], XI, 0.05, cond=False)
    assert np.array_equal(u.to_numpy().view(np.uint64), r["coal"].view(np.uint64))


def test_zero_supersaturation_is_coalescence_alone(gpu_cloudy, workload_runs):
    """COAL | COND with s = 0 on cfg3a against cloudy_ssprk33_steps: <= 1e-13 of |u0| + |u| (not bits: f + 0 may contract
    differently), wherever the coalescence-only state is finite; the same entries are NaN / Inf in both.  The workload's empty
    modes stay exactly zero in both (|u0| + |u| = 0: the denominator's floor makes any other value there fail)."""
    cloudy = gpu_cloudy
    r = workload_runs["cfg3a"]
    mom = r["wl"]["mom"]
    u = dev(cloudy, mom)
    cloudy.solve_box_ssprk33(r["wl"]["par"], u, r["dt"], r["n_steps"], XI, 0.0)
    got, coal = u.to_numpy(), r["coal"]
    fin = np.isfinite(coal)
    assert np.array_equal(np.isfinite(got), fin)
    err = np.abs(got - coal)[fin] / np.maximum((np.abs(mom) + np.abs(coal))[fin], 1e-300)
    print(f"s = 0: max |combined - coalescence only| / (|u0| + |u|) = {err.max():.2e}")
    assert err.max() <= 1e-13, err.max()


@pytest.mark.parametrize("thr,moving", [((INF, INF), False), ((5e-9, INF), False), ((0.9, 1.0), True)])
def test_two_moment_mode_partial_workgroup_and_moving_threshold(gpu_cloudy, oracle, thr, moving):
    """The setup of test_fused_integrators_two_moment_mode_partial_workgroup_and_padding (Exponential + Gamma, 5 planes, 300
    parcels in buffers of leading dimension 320, 2 steps out of place) with COAL | COND, and a MovingThreshold plan besides:
    lanes without a parcel stay for the ranking's barriers and neither read nor write."""
    cloudy = gpu_cloudy
    n, ld, dt, n_steps = 300, 320, 1e-3, 2
    dist_types = [0, 1]
    par, op, _ = make_case(cloudy, oracle, dist_types, bench.kernel_matrix(bench.workload_spec("cfg3a")), thr, bench.NORMS, moving=moving)
    plan = par.coal_data.plan(dist_types)
    assert plan.nmom == 5
    mom = mixed_moments(dist_types, n, seed=7)
    s = supersaturation(n)
    tol = TOL_QUAD if (moving or any(np.isfinite(thr))) else TOL_POLY
    want = oracle_reference(oracle, op, mom, dt, n_steps, XI, s, True, True)
    ok = regular(mom, want)
    print(f"thr={thr} moving={moving}: {ok.sum()} regular parcels of {n}")
    # (of the oracle alone: 300 / 276 / 205 regular parcels -- 300 / 276 with coalescence only; the percentile thresholds of the
    # MovingThreshold plan move mass between the modes faster than a factor 10 in two steps for the rest)
    assert ok.sum() >= (200 if moving else 0.9 * n), ok.sum()
    buf = np.full((5, ld), 7.0)
    buf[:, :n] = mom
    u_in = dev(cloudy, buf)
    u_out = dev(cloudy, blank(5, ld))
    cloudy._lib.check(box_steps(cloudy, plan, u_in, u_out, n, ld, cloudy.SRC_COAL | cloudy.SRC_COND, dev(cloudy, s[None, :]), dt, n_steps))
    got = u_out.to_numpy()
    assert np.all(got[:, n:].view(np.uint64) == SENTINEL), "the padding columns were written"
    assert np.array_equal(u_in.to_numpy(), buf), "the input changed"
    err = rel_err(got[:, :n], want, mom, ok)
    print(f"thr={thr} moving={moving}: fused coalescence + condensation vs oracle stepping, max rel err {err.max():.2e}")
    assert err.max() < max(1e3 * tol, 1e-9), err.max()


def test_float_planes(gpu_cloudy, workload_runs):
    """A CLOUDY_F32 plan of cfg3a, COAL | COND, 400 parcels, 2 steps: the arithmetic is the fp64 plan's, so against the fp64
    plan's result on the float-rounded input the error is the one rounding of the store, 2^-23 = 1.2e-7 of |u0| + |u|."""
    cloudy = gpu_cloudy
    r = workload_runs["cfg3a"]
    wl, s, dt = r["wl"], r["s"], r["dt"]
    mom32 = wl["mom"].astype(np.float32)
    s_dev = dev(cloudy, s[None, :])
    u64 = dev(cloudy, mom32.astype(np.float64))
    cloudy.solve_box_ssprk33(wl["par"], u64, dt, 2, XI, s_dev)
    u32 = dev(cloudy, mom32)
    cloudy.solve_box_ssprk33(wl["par"], u32, dt, 2, XI, s_dev)
    want, got = u64.to_numpy(), u32.to_numpy()
    assert got.dtype == np.float32
    ok = regular(mom32.astype(np.float64), want)
    assert ok.sum() >= 0.9 * r["n"], ok.sum()
    err = rel_err(got.astype(np.float64), want, mom32.astype(np.float64), ok)
    print(f"float planes: {ok.sum()} regular parcels, max err {err.max():.2e} of |u0| + |u|")
    assert err.max() <= 1.2e-7, err.max()


def test_five_gamma_modes_beyond_the_ahead_of_time_families(gpu_cloudy, oracle):
    """A 5-Gamma-mode plan without thresholds, which only the kernels compiled for the plan serve: COAL | COND, 128 parcels,
    2 steps, against the oracle stepping with the bound of test_combined_sources_vs_oracle_stepping.

    The batch is the first 128 parcels of many_mode_moments that have no zero-variance mode.  Such a mode sits ON the closure's
    clamp (k = +Inf -> k_max, or k < 0 -> k_min, by the last bit of M2 M0 - M1^2), where the oracle stepping is no reference at
    1e-9: with M2 of every mode one ulp up, the oracle's own end state of two of the five such parcels of this seed moves by
    1.0 of |u0| + |u| while it calls them regular (test_plans_beyond_the_ahead_of_time_families masks them for the same
    reason).  Of the parcels kept, none moves by more than 1e-9 under that perturbation in either direction: asserted below."""
    cloudy = gpu_cloudy
    dist_types, n, dt, n_steps = [1] * 5, 128, 1e-3, 2
    # (Golovin's kernel, b = 5, between every pair of modes; kernel, seed and step picked on the oracle alone: 128 regular
    # parcels of 128 -- the random order-1 tensors of test_plans_beyond_the_ahead_of_time_families leave none at this step)
    par, op, _ = make_case(cloudy, oracle, dist_types, [[0.0, 5.0], [5.0, 0.0]], (INF,) * 5, bench.NORMS)
    mom, off_clamp = many_mode_moments(dist_types, 160, seed=18)
    mom = np.ascontiguousarray(mom[:, off_clamp][:, :n])
    assert mom.shape == (15, n)
    s = supersaturation(n)
    want = oracle_reference(oracle, op, mom, dt, n_steps, XI, s, True, True)
    ok = regular(mom, want)
    assert ok.sum() >= 0.9 * n, ok.sum()
    for toward in (np.inf, -np.inf):   # the reference's own sensitivity to the last bit of its input
        nudged = mom.copy()
        nudged[2::3] = np.nextafter(mom[2::3], toward)
        moved = rel_err(oracle_reference(oracle, op, nudged, dt, n_steps, XI, s, True, True), want, mom, ok)
        assert moved.max() < 1e-9, moved.max()
    u = dev(cloudy, mom)
    cloudy.solve_box_ssprk33(par, u, dt, n_steps, XI, dev(cloudy, s[None, :]))
    err = rel_err(u.to_numpy(), want, mom, ok)
    print(f"five Gamma modes: {ok.sum()} regular parcels of {n}, max rel err {err.max():.2e}")
    assert err.max() < max(1e3 * TOL_POLY, 1e-9), err.max()


def test_refusals(gpu_cloudy, oracle):
    """Status codes and a message, never an exception or a launch."""
    cloudy = gpu_cloudy
    L, E = cloudy.lib(), cloudy._lib
    COAL, COND = cloudy.SRC_COAL, cloudy.SRC_COND

    def call(plan, u, sources, n_steps=1, dt=1e-3, xi=XI):
        n = u.to_numpy().shape[1]
        rc = L.cloudy_box_ssprk33_steps(plan.handle, n, n, u.ptr, u.ptr, sources, None, 0.01, xi, dt, n_steps, None)
        assert rc == 0 or L.cloudy_last_error() != b"", "a refusal without a message"
        return rc

    # a NumericalCoalStyle plan: condensation alone is served, the combined kernel is not built for it
    numerical = cloudy.NumericalPlan([1, 1], cloudy.LinearKernelFunction(5e-3), bench.NORMS, 10, quad_mode=cloudy.QUAD_FIXED)
    mom = bench.synth_moments(2, 64, 3)
    uq = dev(cloudy, mom)
    assert call(numerical, uq, COAL | COND) == E.EUNSUPPORTED and b"quadrature" in L.cloudy_last_error()
    assert call(numerical, uq, COAL | COND, n_steps=0) == E.EUNSUPPORTED
    assert np.array_equal(uq.to_numpy(), mom)
    assert call(numerical, uq, COND) == 0
    op = oracle.make_params([1, 1], np.zeros((1, 1)), (INF, INF), norms=bench.NORMS)
    want = oracle_reference(oracle, op, mom, 1e-3, 1, XI, 0.01, False, True)   # (64 regular parcels of 64)
    assert np.allclose(uq.to_numpy(), want, rtol=1e-11, atol=0)
    # a tensor plan
    wl = bench.make_workload("cfg3a", 64, seed=3)
    plan = wl["coal_data"].plan(wl["dist_types"])
    u = dev(cloudy, wl["mom"])
    for sources in (0, 4, -1):
        assert call(plan, u, sources) == E.EINVAL
    assert call(plan, u, COAL | COND, n_steps=-1) == E.EINVAL
    assert call(plan, u, COND, dt=float("nan")) == E.EINVAL
    assert call(plan, u, COND, xi=float("nan")) == E.EINVAL
    assert L.cloudy_box_ssprk33_steps(None, 64, 64, u.ptr, u.ptr, COND, None, 0.01, XI, 1e-3, 1, None) == E.EINVAL
    assert L.cloudy_box_ssprk33_steps(plan.handle, 64, 63, u.ptr, u.ptr, COND, None, 0.01, XI, 1e-3, 1, None) == E.EINVAL   # ld < n
    assert np.array_equal(u.to_numpy(), wl["mom"])
    # CLOUDY_F32_FAST: the single-pass operator's mode, as for cloudy_tsit5_steps
    fast = wl["coal_data"].plan(wl["dist_types"], dtype=cloudy.F32_FAST)
    uf = dev(cloudy, wl["mom"].astype(np.float32))
    for sources in (COAL, COND, COAL | COND):
        assert call(fast, uf, sources) == E.EUNSUPPORTED
    # without plan-time compilation the kernels with the condensation source do not exist; coalescence alone is still served
    aot = wl["coal_data"].plan(wl["dist_types"], specialize=-1)
    assert call(aot, u, COAL | COND) == E.EUNSUPPORTED and b"plan-time compilation" in L.cloudy_last_error()
    assert call(aot, u, COND) == E.EUNSUPPORTED and b"plan-time compilation" in L.cloudy_last_error()   # (a documented limit)
    assert np.array_equal(u.to_numpy(), wl["mom"])
    assert call(aot, u, COAL) == 0
    # the per-parcel supersaturation is fp64 whatever the planes are: the Python entry refuses anything else before the launch
    u = dev(cloudy, wl["mom"])
    for bad in (dev(cloudy, np.zeros((1, 64), dtype=np.float32)), dev(cloudy, np.zeros((1, 63))), dev(cloudy, np.zeros((2, 64)))):
        with pytest.raises(ValueError):
            cloudy.solve_box_ssprk33(wl["par"], u, 1e-3, 1, XI, bad)
    assert np.array_equal(u.to_numpy(), wl["mom"])
    # an empty batch is fine
    assert L.cloudy_box_ssprk33_steps(plan.handle, 0, 0, None, None, COAL | COND, None, 0.01, XI, 1e-3, 1, None) == 0
