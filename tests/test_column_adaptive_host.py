"""CPU-only checks of the per-column adaptive Tsit5 for rainshaft columns (cloudy_rainshaft_tsit5_adaptive, csrc/adaptive_column.hpp):
the NumPy restatement of its rules (tsit5_restated.adaptive_tsit5 with nz cells per group and clamp=True: one controller per
column, the clamp of u and u_new, the column norm), the restatement against the per-parcel one
for columns of one cell, the batch the GPU tests use -- picked on the oracle alone -- with the range of its attempts and the
sensitivity of its accept / reject decisions to the last bit of the right-hand side, the symbol in the header, the ctypes table,
the Julia shim and the Python wrapper, every argument check of the C entry point, and the plan-time units compiling for gfx950
without a device.

tests/test_gpu_column_adaptive.py runs the same restatement on the oracle's column right-hand side as the device's reference."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest

import bench
from gpu_support import DZ, GOLOVIN, NCOL, NZ, VEL, XI, column_set, supersaturation
from test_host_abi import INF, ROOT
from tsit5_restated import (DONE, adaptive_tsit5, assert_adaptive_opts_refusals, assert_symbol_agrees, default_opts, last_bit_noise,
                            plane_norms)

NAME = "cloudy_rainshaft_tsit5_adaptive"


def column_rhs_host(oracle, op, nz, dz, xi=0.0, s=None):
    """-> f(x): the column right-hand side on a clamped COPY of x -- oracle.rainshaft_cell_batch, the upwind divergence, and (s not
    None) oracle.rhs_condensation_batch: the f of test_gpu_column_sources.oracle_stepping without the in-place mutation"""
    def f(x):
        x = np.where(x < 0, 0.0, x)
        nmom, n = x.shape
        cs, sf = oracle.rainshaft_cell_batch(op, x)
        fl = np.concatenate([sf.reshape(nmom, n // nz, nz), np.zeros((nmom, n // nz, 1))], axis=2)
        out = cs + (-(fl[:, :, 1:] - fl[:, :, :-1]) / dz).reshape(nmom, n)
        return out if s is None else out + oracle.rhs_condensation_batch(op, xi, s, x)

    return f


# ---- the batch (shared with the GPU tests): picked on the oracle alone
# the 20-cell, dz = 150 columns of gpu_support.column_set, column c scaled by 10^(c / 26 - 1 / 2): amplitudes over a
# decade (times the factors the set has already), supersaturation() on.  T_SPAN: at reltol = 1e-6 the columns take 7 .. 22
# (gamma_mixture) and 8 .. 15 (single_gamma) attempts from the automatic first step.  Under this controller these columns reject
# nothing from there (scanned on the oracle: t_span 5 .. 400, reltol 1e-3 .. 1e-6, amplitudes down to a thirtieth: no rejection),
# so the batch is run a second time from a caller's first step DT0 = t_span / 2, which the denser columns reject up to three
# times: 3 .. 16 and 3 .. 8 attempts (test_the_batch_of_the_gpu_tests asserts the ranges and the rejections and prints the counts).
T_SPAN = {"gamma_mixture": 12.0, "single_gamma": 12.0}
DT0 = 6.0
FIRST = {"auto": None, "dt0": DT0}
CASES = ("gamma_mixture", "single_gamma")


def oracle_case(oracle, case):
    """-> (oracle params, dist_types, thresholds, amplitudes) of the reference's two column plans (gpu_support.reference_case)"""
    if case == "gamma_mixture":
        dist_types, thr, amp = [1, 1], (2e-10, INF), np.array([1e7, 1e-3, 2e-13, 0.0, 0.0, 0.0])
    else:
        dist_types, thr, amp = [1], (INF,), np.array([1e7, 1e-3, 2e-13])
    N = len(dist_types)
    kc = np.broadcast_to(np.asarray(GOLOVIN, dtype=np.float64), (N, N, 2, 2)).copy()
    return oracle.make_params(dist_types, kc, thr, norms=bench.NORMS, vel=VEL), dist_types, thr, amp


def column_batch(amp, ncol=NCOL):
    u0 = column_set(amp)
    scale = 10.0 ** (np.arange(NCOL) / (NCOL - 1) - 0.5)
    return np.ascontiguousarray((u0 * np.repeat(scale, NZ))[:, : ncol * NZ])


def column_reference(oracle, case, reltol=1e-6, max_steps=10000, dt=None, t_span=None, cond=True, ncol=NCOL, perturb=None, xi=XI, u0=None):
    """-> (u0, s, the restatement's result) of the batch"""
    op, dist_types, _, amp = oracle_case(oracle, case)
    u0 = column_batch(amp, ncol) if u0 is None else u0
    s = supersaturation(NZ, DZ, NCOL)[: u0.shape[1]]
    f = column_rhs_host(oracle, op, NZ, DZ, xi, s if cond else None)
    rhs = f if perturb is None else (lambda u: f(u) * perturb(u.shape))
    # normalised=False: the column kernels keep the state physical (abstol_i = abstol norm_i), whatever the plan's thresholds
    res = adaptive_tsit5(rhs, u0, T_SPAN[case] if t_span is None else t_span,
                         dict(reltol=reltol, abstol=1e-9, max_steps=max_steps, dt=dt, plane_norms=plane_norms((3,) * len(dist_types)),
                              normalised=False), nz=NZ, clamp=True)
    return u0, s, res


@functools.lru_cache(maxsize=None)
def column_reference_cached(case, first="auto", reltol=1e-6, max_steps=10000, cond=True):
    """the unperturbed reference of the batch, computed once per session and shared (treat the arrays as read-only)"""
    from oracle import cloudy_oracle

    u0, s, res = column_reference(cloudy_oracle, case, reltol=reltol, max_steps=max_steps, cond=cond, dt=FIRST[first])
    for a in (u0, s) + tuple(res.values()):
        a.setflags(write=False)
    return u0, s, res


# ---- 1. the restatement against the per-parcel one
def test_columns_of_one_cell_are_the_per_parcel_restatement(oracle):
    """nz = 1: the column norm is the parcel's, nothing couples the cells, and -- on an input on which the clamp never acts (a
    Golovin box: M0 falls towards a positive limit, M1 stays, M2 grows) -- the restatement reproduces
    adaptive_tsit5(clamp=False), both with normalised=False, bit for bit: state, t, dt and counts."""
    from test_tsit5_adaptive_host import GOLOVIN_KC, GOLOVIN_T, golovin_batch

    op = oracle.make_params([oracle.GAMMA], np.array(GOLOVIN_KC), (INF,), norms=bench.NORMS)
    u0 = golovin_batch("gamma", 33)
    seen = []

    def rhs(u):
        seen.append(float(u.min()))
        return oracle.rhs_coal_batch(op, u)

    # (dt: a first step the dense parcels reject)
    o = dict(reltol=1e-6, abstol=1e-9, max_steps=10000, plane_norms=plane_norms((3,)), dt=GOLOVIN_T / 6, normalised=False)
    want = adaptive_tsit5(rhs, u0, GOLOVIN_T, o)
    got = adaptive_tsit5(rhs, u0, GOLOVIN_T, o, nz=1, clamp=True)
    assert min(seen) > 0.0                              # the clamp never acted, in either run
    assert want["rejected"].sum() > 0 and want["accepted"].max() > 4 * want["accepted"].min()
    for key in ("u", "t", "dt", "accepted", "rejected", "status", "evals"):
        assert np.array_equal(got[key], want[key]), key


# ---- 2. the batch of the GPU tests
@pytest.mark.parametrize("first", sorted(FIRST))
@pytest.mark.parametrize("case", CASES)
def test_the_batch_of_the_gpu_tests(oracle, case, first):
    """On the restatement alone: every column reaches t_span in between 3 and 40 attempts, from the caller's first step there are
    rejections, and the counts differ between columns; with every entry of the right-hand side multiplied by 1 +- 1e-15 NO column changes its
    (accepted, rejected) -- the GPU tests compare them column by column, and the device's right-hand side differs from the
    oracle's in the last bits -- and the end state of the batch moves by no more than 1e-10 of the plane maxima: a reference
    resolves the 1e-9 the GPU tests ask the device for only if its own response to the last bit of its right-hand side is well
    below, a tenth (measured: 3.7e-11 on the thresholded plan, whose nearly empty rain mode amplifies it)."""
    u0, s, base = column_reference_cached(case, first)
    att = base["accepted"] + base["rejected"]
    print(f"{case}, first step {first}: t_span = {T_SPAN[case]}, attempts {att.min()} .. {att.max()}, rejected {base['rejected'].sum()} in "
          f"{(base['rejected'] > 0).sum()} columns; accepted {base['accepted'].tolist()}")
    assert np.all(base["status"] == DONE) and np.all(base["t"] == T_SPAN[case])
    assert att.min() >= 3 and att.max() <= 40
    assert base["rejected"].sum() >= (1 if first == "dt0" else 0)
    assert len(set(att[:25].tolist())) > 1              # (the 25 columns of the first 512-thread workgroup)
    assert base["u"].min() >= 0.0
    _, _, pert = column_reference(oracle, case, perturb=last_bit_noise(1), dt=FIRST[first])
    changed = (base["accepted"] != pert["accepted"]) | (base["rejected"] != pert["rejected"])
    moved = (np.abs(pert["u"] - base["u"]).max(axis=1) / (np.abs(base["u"]).max(axis=1) + 1e-300)).max()
    print(f"{case}: {int(changed.sum())} of {NCOL} columns change (accepted, rejected) under last-bit noise of the right-hand side; "
          f"the end state moves by {moved:.1e} of the plane maxima")
    assert not changed.any(), np.flatnonzero(changed)
    assert moved <= 1e-10
    # the proposed next step: from the caller's first step the reference resolves the 1e-6 the GPU tests ask for (a tenth: 1e-7;
    # measured 1e-9).  From the automatic first step it does not: the first steps are so short that their error estimates are
    # rounding noise, and q = EEst^(7/50) of such a step moves dt by up to 7e-3 -- which is why the GPU tests compare dt_dev on the
    # runs from DT0 and hold the automatic runs to counts and state.
    dt_moved = (np.abs(pert["dt"] - base["dt"]) / base["dt"]).max()
    print(f"{case}, first step {first}: dt moves by {dt_moved:.1e} relative")
    assert dt_moved <= (1e-7 if first == "dt0" else 5e-2)


# ---- 3. ABI
ARGS = ["ptr", "size_t", "size_t", "size_t", "ptr", "ptr", "int", "ptr", "double", "double", "double", "double", "ptr", "ptr", "ptr", "ptr",
        "ptr"]


def test_symbol_in_header_ctypes_table_julia_shim_and_python(cloudy):
    assert_symbol_agrees(cloudy, NAME, ARGS)
    ctype_of = {"ptr": (C.c_void_p, C.POINTER(cloudy._lib.AdaptiveOptsC)), "size_t": (C.c_size_t,), "int": (C.c_int,), "double": (C.c_double,)}
    for a, c in zip(cloudy._lib.SYMBOLS[NAME][1], ARGS):
        assert a in ctype_of[c], (a, c)
    assert "function solve_rainshaft_tsit5_adaptive!(u, plan::Plan, nz, dz, t_span;" in open(os.path.join(ROOT, "julia", "CloudyHIP.jl")).read()
    assert "solve_rainshaft_tsit5_adaptive" in cloudy.__all__
    sig = inspect.signature(cloudy.solve_rainshaft_tsit5_adaptive).parameters
    assert list(sig) == ["par", "u", "t_span", "xi", "s", "reltol", "abstol", "dt", "max_steps", "out", "dt_dev", "info", "stream"]
    assert (sig["xi"].default, sig["s"].default, sig["reltol"].default, sig["abstol"].default) == (0.0, None, 1e-6, 1e-9)
    assert (sig["dt"].default, sig["max_steps"].default, sig["out"].default, sig["dt_dev"].default) == (None, 10000, None, None)
    assert sig["info"].default is False
    header = open(os.path.join(ROOT, "include", "cloudy_hip.h")).read()
    assert "cloudy_rainshaft_cond_ssprk33_steps as the alternative" in header and "[3][n_columns]" in header


def test_argument_checks_answer_einval_with_a_message(cloudy):
    L, E = cloudy.lib(), cloudy._lib
    nan = float("nan")
    dummy = C.c_void_p(64)   # never dereferenced: every check below precedes any device work

    def call(opts="default", nz=20, ncol=2, ld=40, t_span=1.0, u_in=dummy, u_out=dummy, sources=3, xi=1e-8, dz=150.0, **kw):
        o = default_opts(cloudy, **kw) if opts == "default" else opts
        return L.cloudy_rainshaft_tsit5_adaptive(None, nz, ncol, ld, u_in, u_out, sources, None, 0.01, xi, dz, t_span,
                                                 None if o is None else C.byref(o), None, None, None, None)

    def msg():
        return L.cloudy_last_error().decode()

    assert call() == E.EINVAL and msg() == "plan is NULL"          # everything else is in order
    assert call(sources=1) == E.EINVAL and msg() == "plan is NULL"
    assert call(ncol=0, ld=0, u_in=None, u_out=None) == E.EINVAL and msg() == "plan is NULL"
    assert_adaptive_opts_refusals(cloudy, call, msg, n_parcels=40)
    for bad in (0, 2, 4, -1):                           # CLOUDY_SRC_COND alone is not a column right-hand side
        assert call(sources=bad) == E.EINVAL and "sources" in msg(), bad
    assert call(nz=0, ncol=2, ld=40) == E.EINVAL and "nz" in msg()
    for bad in (0.0, -150.0, nan):
        assert call(dz=bad) == E.EINVAL and "dz" in msg(), bad
    assert call(xi=nan) == E.EINVAL and "xi" in msg()
    assert call(xi=0.0) == E.EINVAL and msg() == "plan is NULL"


# ---- 4. the plan-time units
def _units(tmp_path):
    return [f for f in sorted(os.listdir(tmp_path)) if f.endswith(".hip") and " cloudy_jit_column_adaptive_" in open(tmp_path / f).read()]


@pytest.mark.parametrize("case", CASES)
def test_adaptive_column_units_compile_without_a_gpu(cloudy, case, tmp_path, monkeypatch):
    """cloudy_jit_selfcheck compiles every unit the runtime could request for a plan: for the reference's two column plans that
    includes one adaptive column unit per workgroup size, each with the kernel without and the kernel with the condensation
    source as instances of column_tsit5_adaptive_body; kept through CLOUDY_HIP_JIT_DUMP, they name adaptive_column.hpp, define no
    kernel of another unit, and their code objects exist."""
    monkeypatch.setenv("CLOUDY_HIP_JIT_DUMP", str(tmp_path))
    L = cloudy.lib()
    nm = 1 if case == "single_gamma" else 2
    d, keep = cloudy.Plan.make_desc([1] * nm, np.array(GOLOVIN), (2e-10, INF)[2 - nm:], bench.NORMS, 0, vel=VEL)
    assert L.cloudy_jit_selfcheck(C.byref(d), b"gfx950") == 0, L.cloudy_last_error().decode()
    units = _units(tmp_path)
    assert len(units) == 3, units
    mode = "MODE_ALLINF" if nm == 1 else "MODE_FIXED"
    tails = set()
    for u in units:
        text = open(tmp_path / u).read()
        m = re.search(r" cloudy_jit_column_adaptive_coal_n%dp2_f64(_b512|_b1024|)\(" % nm, text)
        assert m, u
        tails.add(m.group(1))
        assert " cloudy_jit_column_adaptive_coalcond_n%dp2_f64%s(" % (nm, m.group(1)) in text
        bs = m.group(1)[2:] or "256"
        assert text.count(f"__launch_bounds__({bs})") == 2
        assert re.search(r"column_tsit5_adaptive_body<%d, 2, cloudy::%s, double, true, %s, false>" % (nm, mode, bs), text)
        assert re.search(r"column_tsit5_adaptive_body<%d, 2, cloudy::%s, double, true, %s, true>" % (nm, mode, bs), text)
        assert '#include "adaptive_column.hpp"' in text and "SediArgs kS" in text
        assert "cloudy_jit_rainshaft" not in text and "cloudy_jit_adaptive_tsit5" not in text and "cloudy_jit_box" not in text
        assert os.path.getsize(tmp_path / u.replace(".hip", ".co")) > 1000
    assert tails == {"", "_b512", "_b1024"}


@pytest.mark.parametrize("case", CASES + ("moving", "numerical"))
def test_every_declared_kernel_is_defined_with_its_argument_tags(cloudy, case):
    """cloudy_jit_selfcheck(desc, "source-only") compiles nothing: for every unit of the four plans of this file it checks that each
    kernel the loader would ask for is defined in the unit's text with as many parameters as the launch has argument tags -- the
    generators write both from one list, and the adaptive ones append shared lists to it."""
    L = cloudy.lib()
    if case == "numerical":
        d = cloudy.NumericalPlan.make_desc([1, 1], cloudy.LinearKernelFunction(5e-3), bench.NORMS, 10, quad_mode=cloudy.QUAD_FIXED)
    elif case == "moving":
        d, keep = cloudy.Plan.make_desc([1, 1], np.array(GOLOVIN), (0.9, 1.0), bench.NORMS, 1, vel=VEL)
    else:
        nm = 1 if case == "single_gamma" else 2
        d, keep = cloudy.Plan.make_desc([1] * nm, np.array(GOLOVIN), (2e-10, INF)[2 - nm:], bench.NORMS, 0, vel=VEL)
    assert L.cloudy_jit_selfcheck(C.byref(d), b"source-only") == 0, L.cloudy_last_error().decode()


@pytest.mark.parametrize("case", ["moving", "numerical"])
def test_plans_that_are_not_served_have_no_such_unit(cloudy, case, tmp_path, monkeypatch):
    """A MovingThreshold plan (with a velocity term) and a NumericalCoalStyle plan: none of their units defines an adaptive column
    kernel (the entry point refuses them)."""
    monkeypatch.setenv("CLOUDY_HIP_JIT_DUMP", str(tmp_path))
    L = cloudy.lib()
    if case == "numerical":
        d = cloudy.NumericalPlan.make_desc([1, 1], cloudy.LinearKernelFunction(5e-3), bench.NORMS, 10, quad_mode=cloudy.QUAD_FIXED)
    else:
        d, keep = cloudy.Plan.make_desc([1, 1], np.array(GOLOVIN), (0.9, 1.0), bench.NORMS, 1, vel=VEL)
    assert L.cloudy_jit_selfcheck(C.byref(d), b"gfx950") == 0, L.cloudy_last_error().decode()
    assert any(f.endswith(".hip") for f in os.listdir(tmp_path))
    assert _units(tmp_path) == []
