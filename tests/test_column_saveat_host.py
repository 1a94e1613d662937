"""CPU-only checks of the dense output of the per-column adaptive Tsit5 (cloudy_rainshaft_tsit5_adaptive_saveat,
csrc/adaptive_column.hpp with SAVE = true): the NumPy restatement with snapshots (tsit5_restated.adaptive_tsit5 with nz cells per
group, clamp=True and t_save: the loop of test_column_adaptive_host plus the snapshot rule, one cursor per column, interpolated snapshots
clamped to >= 0) that leaves the integration bit for bit alone, the snapshot paths the batch of the GPU tests walks, the sensitivity of the
snapshots to the last bit of the right-hand side, the accuracy of the interpolant inside a step against the step's end, the ABI,
the argument checks of the C entry point in their order, and the plan-time units compiling for gfx950 without a device.

tests/test_gpu_column_saveat.py runs the same restatement on the oracle's column right-hand side as the device's reference."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest

import bench
from test_column_adaptive_host import (CASES, DT0, FIRST, T_SPAN, column_batch, column_reference, column_reference_cached, column_rhs_host,
                                       oracle_case)
from gpu_support import DZ, GOLOVIN, NCOL, NZ, VEL, XI, supersaturation
from test_host_abi import INF, ROOT, _c_prototypes
from tsit5_restated import (DONE, MAX_STEPS, SAVE_FRACS, adaptive_tsit5, assert_adaptive_opts_refusals, assert_symbol_agrees, default_opts,
                            last_bit_noise, plane_norms, save_times)

NAME = "cloudy_rainshaft_tsit5_adaptive_saveat"
# what the GPU test asks of every snapshot, in units of the maximum of its plane (the bound of the column parity test), and what
# the restatement must resolve for that bound to mean anything: a tenth
SNAPSHOT_BOUND = 1e-9
KEYS = ("u", "t", "dt", "accepted", "rejected", "status", "evals")


def column_saveat_reference(oracle, case, reltol=1e-6, max_steps=10000, dt=None, t_span=None, t_save=None, perturb=None):
    """-> (u0, s, t_save, the restatement's result) of the batch of test_column_adaptive_host (COAL | COND, the profile on) at the
    twelve save times"""
    op, dist_types, _, amp = oracle_case(oracle, case)
    u0 = column_batch(amp)
    s = supersaturation(NZ, DZ, NCOL)
    f = column_rhs_host(oracle, op, NZ, DZ, XI, s)
    rhs = f if perturb is None else (lambda u: f(u) * perturb(u.shape))
    t_span = T_SPAN[case] if t_span is None else t_span
    ts = save_times(t_span) if t_save is None else np.asarray(t_save, dtype=np.float64)
    res = adaptive_tsit5(rhs, u0, t_span, dict(reltol=reltol, abstol=1e-9, max_steps=max_steps, dt=dt,
                                               plane_norms=plane_norms((3,) * len(dist_types)), normalised=False),
                         nz=NZ, clamp=True, t_save=ts)   # (normalised=False: the state of a column is physical, as in column_reference)
    return u0, s, ts, res


@functools.lru_cache(maxsize=None)
def column_saveat_reference_cached(case, first="dt0", reltol=1e-6, max_steps=10000):
    """the unperturbed reference with snapshots, computed once per session and shared (treat the arrays as read-only)"""
    from oracle import cloudy_oracle

    u0, s, ts, res = column_saveat_reference(cloudy_oracle, case, reltol=reltol, max_steps=max_steps, dt=FIRST[first])
    for a in (u0, s, ts) + tuple(v for v in res.values() if isinstance(v, np.ndarray)):
        a.setflags(write=False)
    return u0, s, ts, res


def snapshot_distance(got, want):
    """the largest |got - want| over the cells of a snapshot plane in units of that plane's maximum, over every snapshot and plane
    (NaN where either is NaN)"""
    return float((np.abs(got - want).max(axis=2) / (np.abs(want).max(axis=2) + 1e-300)).max())


def snapshots_reached(saved, nz=NZ):
    """saved (n_save, planes, nz * ncol) -> two (n_save, ncol) masks: every plane of every cell of the column is finite in the
    snapshot; every one is NaN"""
    by_col = saved.reshape(saved.shape[0], saved.shape[1], -1, nz)
    return np.isfinite(by_col).all(axis=(1, 3)), np.isnan(by_col).all(axis=(1, 3))


# ---- 1. the restatement
@pytest.mark.parametrize("first", sorted(FIRST))
@pytest.mark.parametrize("case", CASES)
def test_restatement_integrates_as_the_one_without_snapshots(case, first):
    u0, s, ts, res = column_saveat_reference_cached(case, first)
    _, _, base = column_reference_cached(case, first)
    for key in KEYS:
        assert np.array_equal(np.ascontiguousarray(res[key]).view(np.uint8), np.ascontiguousarray(base[key]).view(np.uint8)), key
    assert res["saved"].shape == (len(SAVE_FRACS), u0.shape[0], NCOL * NZ) and np.isfinite(res["saved"]).all()
    assert np.array_equal(res["saved"][0], u0) and np.array_equal(res["saved"][-1], res["u"])
    assert all(sum(st) == len(SAVE_FRACS) - 1 and len(st) == a for st, a in zip(res["in_step"], res["accepted"]))
    zero = adaptive_tsit5(None, u0, 0.0, dict(reltol=1e-6, abstol=1e-9, max_steps=10, plane_norms=np.ones(u0.shape[0]), normalised=False),
                          nz=NZ, clamp=True, t_save=[0.0])
    assert np.array_equal(zero["saved"][0], u0)


def test_columns_of_one_cell_are_the_per_parcel_restatement_with_snapshots(oracle):
    """nz = 1 on the Golovin batch of test_columns_of_one_cell_are_the_per_parcel_restatement, on which the clamp never acts:
    adaptive_tsit5(clamp=False), both with normalised=False and the save times, bit for bit, the snapshots included."""
    from test_tsit5_adaptive_host import GOLOVIN_KC, GOLOVIN_T, golovin_batch

    op = oracle.make_params([oracle.GAMMA], np.array(GOLOVIN_KC), (INF,), norms=bench.NORMS)
    u0 = golovin_batch("gamma", 33)
    seen = []

    def rhs(u):
        seen.append(float(u.min()))
        return oracle.rhs_coal_batch(op, u)

    ts = save_times(GOLOVIN_T)
    o = dict(reltol=1e-6, abstol=1e-9, max_steps=10000, plane_norms=plane_norms((3,)), dt=GOLOVIN_T / 6, normalised=False)
    want = adaptive_tsit5(rhs, u0, GOLOVIN_T, o, t_save=ts)
    got = adaptive_tsit5(rhs, u0, GOLOVIN_T, o, nz=1, clamp=True, t_save=ts)
    assert min(seen) > 0.0 and want["saved"].min() > 0.0    # the clamp never acted, on a stage argument or on a snapshot
    assert want["rejected"].sum() > 0
    for key in KEYS + ("saved",):
        assert np.array_equal(np.ascontiguousarray(got[key]).view(np.uint8), np.ascontiguousarray(want[key]).view(np.uint8)), key
    assert got["in_step"] == want["in_step"]


# ---- 2. the batch exercises the snapshot paths
@pytest.mark.parametrize("case", CASES)
def test_the_batch_walks_every_snapshot_path(case):
    """From DT0, with the twelve save fractions of test_tsit5_saveat_host as they stand: a column with an accepted step that holds
    two or more save times, an accepted step that holds none, a column that rejected a step before its first snapshot inside a
    step, no negative snapshot; with max_steps = 3 a column that stops with status 1 between two save times and a column that
    reaches t_span.
    (No negative snapshot: of the eleven save times > 0, the ones the integrator forms.  The batch holds one cell with -1e-30 on
    purpose, the clamp's test, and the snapshot at 0 is by its own rule the bits of the input, that cell included: it is held to
    that rule instead, and is negative nowhere else.)"""
    u0, _, ts, res = column_saveat_reference_cached(case, "dt0")
    steps = res["in_step"]
    print(f"{case}: save times per accepted step, column by column: {steps}; rejected before the first snapshot {res['rejected_before'].tolist()}")
    assert any(max(st) >= 2 for st in steps)
    assert any(min(st) == 0 for st in steps)
    assert (res["rejected_before"] > 0).any()
    assert ts[0] == 0.0 and ts[1] > 0.0 and res["saved"][1:].min() >= 0.0
    assert np.array_equal(res["saved"][0].view(np.uint64), u0.view(np.uint64)) and (u0 < 0).sum() == u0.shape[0]
    _, _, _, cut = column_saveat_reference_cached(case, "dt0", 1e-6, 3)
    reached, none = snapshots_reached(cut["saved"])
    assert np.all(reached | none)                       # a snapshot of a column is there in every cell and plane, or in none
    n_reached = reached.sum(axis=0)
    partly = (cut["status"] == MAX_STEPS) & (n_reached > 1) & (n_reached < len(ts))
    print(f"{case}, max_steps = 3: status {cut['status'].tolist()}, snapshots reached {n_reached.tolist()}")
    assert partly.any() and ((cut["status"] == DONE) & (n_reached == len(ts))).any()
    for c in range(NCOL):                               # what a column reached is what it passed: t_save <= t
        assert np.array_equal(reached[:, c], ts <= cut["t"][c]), c


# ---- 3. sensitivity
@pytest.mark.parametrize("case", CASES)
def test_snapshots_are_insensitive_to_the_last_bit_of_the_rhs(oracle, case):
    """Every entry of the right-hand side times 1 +- 1e-15: no column changes its counts and no snapshot moves by more than a
    tenth of the 1e-9 of its plane's maximum that the GPU test asks of the device (the device's right-hand side differs from the
    oracle's in the last bits).  Measured: 1.1e-14 on the thresholded plan, 4.8e-15 on the one-mode plan."""
    _, _, _, base = column_saveat_reference_cached(case, "dt0")
    _, _, _, pert = column_saveat_reference(oracle, case, perturb=last_bit_noise(1), dt=DT0)
    changed = (base["accepted"] != pert["accepted"]) | (base["rejected"] != pert["rejected"])
    moved = snapshot_distance(pert["saved"], base["saved"])
    print(f"{case}: {int(changed.sum())} of {NCOL} columns change their counts under last-bit noise of the right-hand side; the "
          f"snapshots move by {moved:.1e} of the plane maxima")
    assert not changed.any(), np.flatnonzero(changed)
    assert moved <= SNAPSHOT_BOUND / 10


# ---- 4. accuracy of the interpolant
# The worst error of a snapshot inside a step over the worst error at t_span of the same reltol = 1e-6 run (from DT0), both
# against restatement runs at reltol = 1e-10 (which end at the time compared) and in units of the plane maxima; measured on this
# restatement on the CPU, per case (the docstring below has the errors themselves); the assertion allows twice that.
INTERIOR_FRACS = (0.2, 0.5, 0.8)
INTERIOR_OVER_END_MEASURED = {"gamma_mixture": 3.79, "single_gamma": 39.2}


@pytest.mark.parametrize("case", CASES)
def test_interpolant_is_as_accurate_as_the_step(oracle, case):
    """A 4th-order interpolant inside a 5th-order step may be worse than the step's end.  Three save times inside the run
    (t_span times 0.2, 0.5, 0.8), each against a restatement run at reltol = 1e-10 that ends there, and the end of the run against
    the one that ends at t_span; measured, in units of the plane maxima:
      gamma_mixture  worst snapshot 5.78e-08, end of run 1.52e-08, ratio 3.79
      single_gamma   worst snapshot 7.49e-08, end of run 1.91e-09, ratio 39.2
    The snapshots of the two plans are equally good, 6e-8 .. 7e-8 at reltol = 1e-6; the ratios differ because the end point of the
    single-mode run happens to be eight times better than the other's.  Asserted: at most twice the measured ratio of the case."""
    _, _, ts, res = column_saveat_reference_cached(case, "dt0")
    _, _, fine = column_reference_cached(case, "auto", 1e-10)
    scale = lambda want: np.abs(want).max(axis=1) + 1e-300   # noqa: E731
    end = float((np.abs(res["u"] - fine["u"]).max(axis=1) / scale(fine["u"])).max())
    interior = 0.0
    for frac in INTERIOR_FRACS:
        j = SAVE_FRACS.index(frac)
        _, _, want = column_reference(oracle, case, reltol=1e-10, t_span=float(ts[j]))
        assert np.all(want["status"] == DONE)
        interior = max(interior, float((np.abs(res["saved"][j] - want["u"]).max(axis=1) / scale(want["u"])).max()))
    print(f"{case}: worst interior snapshot error {interior:.3e}, end-of-run error {end:.3e}, ratio {interior / end:.3f}")
    assert interior <= 2 * INTERIOR_OVER_END_MEASURED[case] * end


# ---- 5. ABI
ARGS = ["ptr", "size_t", "size_t", "size_t", "ptr", "ptr", "int", "ptr", "double", "double", "double", "double", "ptr", "ptr", "ptr", "ptr",
        "ptr", "size_t", "ptr", "ptr"]


def test_symbol_in_header_ctypes_table_julia_shim_and_python(cloudy):
    protos = _c_prototypes()
    assert len(ARGS) == 20
    assert_symbol_agrees(cloudy, NAME, ARGS)
    assert protos[NAME][1] == protos["cloudy_rainshaft_tsit5_adaptive"][1] + protos["cloudy_tsit5_adaptive_saveat"][1][-3:]
    ctype_of = {"ptr": (C.c_void_p, C.POINTER(cloudy._lib.AdaptiveOptsC), C.POINTER(C.c_double)), "size_t": (C.c_size_t,), "int": (C.c_int,),
                "double": (C.c_double,)}
    for a, c in zip(cloudy._lib.SYMBOLS[NAME][1], ARGS):
        assert a in ctype_of[c], (a, c)
    src = open(os.path.join(ROOT, "julia", "CloudyHIP.jl")).read()
    assert "function solve_rainshaft_tsit5_adaptive_saveat!(u, usave, plan::Plan, nz, dz, t_span, t_save;" in src
    assert "solve_rainshaft_tsit5_adaptive_saveat" in cloudy.__all__
    sig = inspect.signature(cloudy.solve_rainshaft_tsit5_adaptive_saveat).parameters
    assert list(sig) == ["par", "u", "t_span", "t_save", "xi", "s", "reltol", "abstol", "dt", "max_steps", "out", "save_out", "dt_dev", "info",
                         "stream"]
    assert sig["t_save"].default is inspect.Parameter.empty
    assert (sig["xi"].default, sig["s"].default, sig["reltol"].default, sig["abstol"].default) == (0.0, None, 1e-6, 1e-9)
    assert (sig["dt"].default, sig["max_steps"].default, sig["out"].default, sig["save_out"].default) == (None, 10000, None, None)
    assert sig["dt_dev"].default is None and sig["info"].default is False and sig["stream"].default is None
    header = open(os.path.join(ROOT, "include", "cloudy_hip.h")).read()
    assert "cloudy_rainshaft_cond_ssprk33_steps as the alternative" in header and "[3][n_columns]" in header
    assert "Dense output at save times and" not in header


def test_argument_checks_answer_einval_with_a_message(cloudy):
    """The save times first, then the checks of cloudy_rainshaft_tsit5_adaptive in its order, the plan last."""
    L, E = cloudy.lib(), cloudy._lib
    nan, inf = float("nan"), float("inf")
    dummy = C.c_void_p(64)   # never dereferenced: every check below precedes any device work
    cap = int(re.search(r"#define CLOUDY_MAX_SAVE_TIMES (\d+)", open(os.path.join(ROOT, "include", "cloudy_hip.h")).read()).group(1))

    def call(times=(0.0, 0.25, 1.0), n_save=None, t_save="times", u_save=dummy, nz=20, ncol=2, ld=40, t_span=1.0, u_in=dummy, u_out=dummy,
             sources=3, xi=1e-8, dz=150.0, opts="default", **kw):
        o = default_opts(cloudy, **kw) if opts == "default" else opts
        arr = (C.c_double * max(len(times), 1))(*times)
        return getattr(L, NAME)(None, nz, ncol, ld, u_in, u_out, sources, None, 0.01, xi, dz, t_span, None if o is None else C.byref(o), None,
                                None, None, None, len(times) if n_save is None else n_save, arr if t_save == "times" else t_save, u_save)

    def msg():
        return L.cloudy_last_error().decode()

    assert call() == E.EINVAL and msg() == "plan is NULL"          # everything else is in order
    assert call(times=(), t_save=None, u_save=None) == E.EINVAL and msg() == "plan is NULL"   # n_save = 0 with NULL pointers
    assert call(times=(0.0,), t_span=0.0) == E.EINVAL and msg() == "plan is NULL"
    # the save times come first: each of these calls has a later argument out of order as well
    later = dict(sources=0, nz=0, dz=-1.0, xi=nan, ld=1)
    big = tuple(np.linspace(0.0, 1.0, cap + 1))
    assert call(times=big, **later) == E.EINVAL and "n_save" in msg() and str(cap) in msg()
    assert call(times=big[:cap]) == E.EINVAL and msg() == "plan is NULL"
    assert call(t_save=None, **later) == E.EINVAL and "t_save" in msg() and "NULL" in msg()
    assert call(u_save=None, **later) == E.EINVAL and "u_save_dev" in msg() and "NULL" in msg()
    for bad in (nan, inf, -inf, -1e-3, 1.0 + 1e-12):                # not finite, negative, beyond t_span
        assert call(times=(0.0, bad), **later) == E.EINVAL and "t_save[1]" in msg(), bad
    assert call(times=(-1e-300,), **later) == E.EINVAL and "t_save[0]" in msg()
    for bad in ((0.5, 0.5), (0.5, 0.25), (0.0, 0.2, 0.2, 1.0)):
        assert call(times=bad, **later) == E.EINVAL and "t_save" in msg() and "strictly increasing" in msg(), bad
    # then the column's checks, in the order of cloudy_rainshaft_tsit5_adaptive
    assert call(reltol=0.0, ld=1, sources=0) == E.EINVAL and "reltol" in msg()
    assert_adaptive_opts_refusals(cloudy, call, msg, n_parcels=40, no_times=dict(times=(), t_save=None, u_save=None),
                                  later=(dict(sources=0), dict(sources=0, dz=-1.0)))
    for bad in (0, 2, 4, -1):
        assert call(sources=bad, nz=0, dz=-1.0) == E.EINVAL and "sources" in msg(), bad
    assert call(nz=0, ncol=2, ld=40, xi=nan) == E.EINVAL and "nz" in msg()
    for bad in (0.0, -150.0, nan):
        assert call(dz=bad, xi=nan) == E.EINVAL and "dz" in msg(), bad
    assert call(xi=nan) == E.EINVAL and "xi" in msg()
    assert call(xi=0.0, sources=1) == E.EINVAL and msg() == "plan is NULL"


# ---- 6. the plan-time units
def _units(tmp_path, word=" cloudy_jit_column_dense_"):
    return [f for f in sorted(os.listdir(tmp_path)) if f.endswith(".hip") and word in open(tmp_path / f).read()]


@pytest.mark.parametrize("case", CASES)
def test_saving_column_units_compile_without_a_gpu(cloudy, case, tmp_path, monkeypatch):
    """cloudy_jit_selfcheck of the reference's two column plans: one unit with the saving kernels per workgroup size, each with
    the kernel without and the kernel with the condensation source as SAVE instances of column_tsit5_adaptive_body; they name
    adaptive_column.hpp, define no kernel of cloudy_rainshaft_tsit5_adaptive (whose three units are still there beside them), and
    their code objects exist."""
    monkeypatch.setenv("CLOUDY_HIP_JIT_DUMP", str(tmp_path))
    L = cloudy.lib()
    nm = 1 if case == "single_gamma" else 2
    d, keep = cloudy.Plan.make_desc([1] * nm, np.array(GOLOVIN), (2e-10, INF)[2 - nm:], bench.NORMS, 0, vel=VEL)
    assert L.cloudy_jit_selfcheck(C.byref(d), b"gfx950") == 0, L.cloudy_last_error().decode()
    units = _units(tmp_path)
    assert len(units) == 3, units
    assert len(_units(tmp_path, " cloudy_jit_column_adaptive_")) == 3
    mode = "MODE_ALLINF" if nm == 1 else "MODE_FIXED"
    tails = set()
    for u in units:
        text = open(tmp_path / u).read()
        m = re.search(r" cloudy_jit_column_dense_coal_n%dp2_f64(_b512|_b1024|)\(" % nm, text)
        assert m, u
        tails.add(m.group(1))
        assert " cloudy_jit_column_dense_coalcond_n%dp2_f64%s(" % (nm, m.group(1)) in text
        bs = m.group(1)[2:] or "256"
        assert text.count(f"__launch_bounds__({bs})") == 2 and text.count("__global__") == 2
        assert re.search(r"column_tsit5_adaptive_body<%d, 2, cloudy::%s, double, true, %s, false, true>" % (nm, mode, bs), text)
        assert re.search(r"column_tsit5_adaptive_body<%d, 2, cloudy::%s, double, true, %s, true, true>" % (nm, mode, bs), text)
        assert text.count("n_save, t_save, u_save)") == 2
        assert '#include "adaptive_column.hpp"' in text and "SediArgs kS" in text
        assert " cloudy_jit_column_adaptive_" not in text and "cloudy_jit_rainshaft" not in text and "cloudy_jit_dense_tsit5" not in text
        assert os.path.getsize(tmp_path / u.replace(".hip", ".co")) > 1000
    assert tails == {"", "_b512", "_b1024"}


@pytest.mark.parametrize("case", ["moving", "numerical"])
def test_plans_that_are_not_served_have_no_such_unit(cloudy, case, tmp_path, monkeypatch):
    monkeypatch.setenv("CLOUDY_HIP_JIT_DUMP", str(tmp_path))
    L = cloudy.lib()
    if case == "numerical":
        d = cloudy.NumericalPlan.make_desc([1, 1], cloudy.LinearKernelFunction(5e-3), bench.NORMS, 10, quad_mode=cloudy.QUAD_FIXED)
    else:
        d, keep = cloudy.Plan.make_desc([1, 1], np.array(GOLOVIN), (0.9, 1.0), bench.NORMS, 1, vel=VEL)
    assert L.cloudy_jit_selfcheck(C.byref(d), b"gfx950") == 0, L.cloudy_last_error().decode()
    assert any(f.endswith(".hip") for f in os.listdir(tmp_path))
    assert _units(tmp_path, "cloudy_jit_column_dense_") == []
