"""CPU-only checks of cloudy_parcel_tsit5_adaptive (csrc/adaptive_thermo.hpp): per-parcel adaptive Tsit5 of the adiabatic parcel
Y = (S, p, T, q_v, mom...).  The error norm treats the four thermodynamic components as planes of norm 1, so the NumPy
restatement of the controller (tsit5_restated.adaptive_tsit5, with snapshots: its t_save) describes the device loop with
plane_norms = (1, 1, 1, 1, norms...), normalised = True, on
the restated right-hand side of test_parcel_host (parcel_rhs_numpy); no second restatement of the controller is written.  Here: the
ABI, every argument check of the C entry point, the plan-time unit compiling for gfx950 without a device, the restatement on the
batches the GPU tests use (attempt ranges, sensitivity of its decisions to the last bit of the right-hand side, error against a
tight-tolerance run) and the Rogers 1975 points through dense output.

tests/test_gpu_parcel_adaptive.py runs the same restatement as the device's reference."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest

import bench
import test_parcel_host as P
from test_host_abi import INF, ROOT, _c_prototypes
from tsit5_restated import (DONE, adaptive_tsit5, assert_adaptive_opts_refusals, assert_symbol_agrees, default_opts, last_bit_noise, plane_norms,
                            save_times)

NAME = "cloudy_parcel_tsit5_adaptive"
NORMS = (1e8, 1e-12)
T_SPAN = 20.0
COAL_T = 5.0        # the COAL | COND batch: picked on the restatement (test 5)
TOL_EVAL = 1e-11    # the per-evaluation bound the project asserts for the condensation right-hand side (tests/test_gpu_box_sources.py)
GOLOVIN = [[0.0, 50.0], [50.0, 0.0]]   # tests/test_gpu_parcel.py


# ---- the batches (shared with the GPU tests): picked on the restatement alone
def decade_draws(n, seed=5):
    """default_rng(seed), two draws in this order: N = 2e8 10^U(-1, 1), w = U(0.5, 10)"""
    rng = np.random.default_rng(seed)
    return 2e8 * 10.0 ** rng.uniform(-1.0, 1.0, n), rng.uniform(0.5, 10.0, n)


def thermo_rows(mass):
    """(S, p, T, q_v) = driver_initial_state(DEFAULTS, M1) per parcel -> (4, n)"""
    return np.array([P.driver_initial_state(P.DEFAULTS, m) for m in mass]).T


def decade_batch(n):
    """the "decade batch": one Monodisperse mode, droplet number and updraft speed spread over a decade each -> (y0 (6, n), w)"""
    N, w = decade_draws(n)
    M1 = N * P.M0_DROP
    return np.ascontiguousarray(np.vstack([thermo_rows(M1), N, M1])), w


def decade_norms(plan=False):
    """plan = False: plane_norms = (1, 1, 1, 1, 1e8, 1e-12), the recipe the figures of test 4 were stated for.  plan = True: the
    norms the plan itself holds for the two planes of the mode, mom_norms = n0 m0^order = (1e8, 1e-4) -- what the device divides by,
    and so what the GPU tests' reference uses (abstol = 1e-9 of M1 / 1e-4 ~ 0.4 .. 40 then matters at reltol = 1e-9: the two
    restatements take different steps there, 10 .. 53 attempts against 18 .. 54 at n = 65)."""
    return np.array([1.0, 1.0, 1.0, 1.0, NORMS[0], NORMS[0] * NORMS[1] if plan else NORMS[1]])


def monodisperse_cond_closed(c, mom_norms=(NORMS[0], NORMS[0] * NORMS[1])):
    """test_parcel_host.monodisperse_cond on the whole state space: get_cond_evap(update_dist_from_moments(mom)) hands an EMPTY
    distribution -- a zero tendency -- to moments that are not positive in the plan's normalised units (ParticleDistributions.jl
    :530-541: m0 > eps and m1 > eps, else n = 0), where the plain restatement takes the cube root of a negative mass.  On states
    with positive moments the two are the same expression.  An adaptive loop does reach the others: S0 = 1 gives no condensation
    tendency, so the automatic first step is far too long, its stage states have M1 <= 0 (109 evaluations of the 65-parcel batch),
    the step is rejected -- and the step size proposed after it depends on what the right-hand side answered there (with the
    plain restatement 1 of 65 and 7 of 257 parcels take another path at reltol 1e-6 than the device does)."""
    plain, eps = P.monodisperse_cond(c), np.finfo(np.float64).eps

    def f(mom, xi, s):
        ok = (mom[0] / mom_norms[0] > eps) & (mom[1] / mom_norms[1] > eps)
        return np.where(ok[None, :], plain(mom, xi, s), 0.0)
    return f


def decade_rhs(w, perturb=None):
    c = P.DEFAULTS
    f = lambda Y: P.parcel_rhs_numpy(c, Y, w, [1], monodisperse_cond_closed(c))  # noqa: E731
    return f if perturb is None else (lambda Y: f(Y) * perturb(Y.shape))


def decade_run(n, reltol, max_steps=10000, perturb=None, times=None, dt=None, t_span=T_SPAN, y0=None, plan=False):
    base, w = decade_batch(n)
    y0 = base if y0 is None else y0
    opts = dict(reltol=reltol, abstol=1e-9, max_steps=max_steps, plane_norms=decade_norms(plan), dt=dt)
    rhs = decade_rhs(w, perturb)
    return y0, w, adaptive_tsit5(rhs, y0, t_span, opts, t_save=times)


@functools.lru_cache(maxsize=None)
def decade_case(n, reltol, max_steps=10000, saveat=False, plan=False):
    """the unperturbed restatement on the decade batch, once per session and shared (treat the arrays as read-only)"""
    return decade_run(n, reltol, max_steps, times=save_times(T_SPAN) if saveat else None, plan=plan)


@functools.lru_cache(maxsize=None)
def decade_tight(n, plan=False):
    """the reltol = 1e-11 run of the same restatement: the reference of the error figures"""
    return decade_run(n, 1e-11, plan=plan)[2]


def two_gamma_batch(n):
    """the two-Gamma state of tests/test_gpu_parcel.py scaled per parcel by N / 2e8, N and w as in the decade batch"""
    N, w = decade_draws(n)
    m0 = P.M0_DROP
    mom = np.array([0.9, 0.9 * m0, 0.9 * (m0 / 2) ** 2 * 6, 0.1, 0.1 * 4 * m0, 0.1 * (2 * m0) ** 2 * 6])[:, None] * N[None, :]
    return np.ascontiguousarray(np.vstack([thermo_rows(mom[1] + mom[4]), mom])), w


def oracle_rhs(oracle, op, w, rows, coal, perturb=None):
    """parcel_rhs_numpy with the moments' tendency from the oracle, as tests/test_gpu_parcel.py's reference() forms it"""
    c = P.DEFAULTS
    scale = (1000.0 / c["rho_l"]) ** (1 / 3)
    cond = lambda mom, xi, s: oracle.rhs_condensation_batch(op, 1.0, xi * s * scale, np.ascontiguousarray(mom))   # noqa: E731
    coal_f = (lambda mom: oracle.rhs_coal_batch(op, np.ascontiguousarray(mom))) if coal else None
    f = lambda Y: P.parcel_rhs_numpy(c, Y, w, rows, cond, coal_f)   # noqa: E731
    return f if perturb is None else (lambda Y: f(Y) * perturb(Y.shape))


def two_gamma_params(oracle):
    return oracle.make_params([oracle.GAMMA] * 2, np.array(GOLOVIN), (INF, INF), norms=NORMS)


def two_gamma_norms():
    return np.concatenate([np.ones(4), plane_norms((3, 3), NORMS)])


def two_gamma_run(oracle, n, coal=True, reltol=1e-6, perturb=None):
    y0, w = two_gamma_batch(n)
    rhs = oracle_rhs(oracle, two_gamma_params(oracle), w, [1, 4], coal, perturb)
    return y0, w, adaptive_tsit5(rhs, y0, COAL_T, dict(reltol=reltol, abstol=1e-9, max_steps=10000, plane_norms=two_gamma_norms()))


@functools.lru_cache(maxsize=None)
def two_gamma_case(n, reltol=1e-6):
    from oracle import cloudy_oracle

    return two_gamma_run(cloudy_oracle, n, reltol=reltol)


def rel_to(got, ref, y0):
    """per plane and parcel: |got - ref| / (|y0| + |ref|)"""
    return np.abs(got - ref) / np.maximum(np.abs(y0) + np.abs(ref), 1e-300)


def rogers_states():
    """the monodisperse driver case (N = 2e8, w = 10) and its 41 save times 0.5 k"""
    y0 = np.array(P.driver_initial_state(P.DEFAULTS, P.N0 * P.M0_DROP) + [P.N0, P.N0 * P.M0_DROP])[:, None]
    return y0, 0.5 * np.arange(41)


def rogers_from_series(t, ys):
    """ys (n_save, 6): -> (supersaturation deviation in percentage points, radius deviation in um)"""
    return P.rogers_deviation(t, (ys[:, 0] - 1) * 100, P.mean_radius_um(P.DEFAULTS, ys[:, 4], ys[:, 5]))


# ---- 1. ABI
def test_symbol_in_header_ctypes_table_julia_shim_and_python(cloudy):
    protos = _c_prototypes()
    plain, steps = protos["cloudy_tsit5_adaptive_saveat"][1], protos["cloudy_parcel_ssprk33_steps"][1]
    # (plan, n, ld, in, out) + (sources, w_dev, w, params) + (t_span, opts, dt_dev, t_dev, info_dev, stream, n_save, t_save, save)
    assert len(protos[NAME][1]) == 18
    assert_symbol_agrees(cloudy, NAME, plain[:5] + steps[5:9] + plain[5:])
    src = open(os.path.join(ROOT, "julia", "CloudyHIP.jl")).read()
    assert re.search(r"function solve_parcel_tsit5_adaptive!\(y, plan::Plan, w, t_span; params::ParcelParams = ParcelParams\(\), "
                     r"coal::Bool = false", src)
    assert "solve_parcel_tsit5_adaptive" in cloudy.__all__
    sig = inspect.signature(cloudy.solve_parcel_tsit5_adaptive).parameters
    assert list(sig) == ["par", "y", "w", "t_span", "params", "coal", "reltol", "abstol", "dt", "max_steps", "times", "out", "dt_dev",
                         "info", "stream"]
    assert sig["params"].default is None and sig["coal"].default is False and sig["times"].default == () and sig["out"].default is None
    assert (sig["reltol"].default, sig["abstol"].default, sig["dt"].default, sig["max_steps"].default) == (1e-6, 1e-9, None, 10000)
    header = open(os.path.join(ROOT, "include", "cloudy_hip.h")).read()
    doc = header[header.index("Per-parcel ADAPTIVE Tsit5 of the adiabatic parcel"):header.index("int " + NAME)]
    for word in ("cloudy_tsit5_adaptive", "abstol in their own units", "max(reltol, abstol / q_v)", "(j * (4 + nmom) + p) * ld + i"):
        assert word in doc, word


# ---- 2. argument checks (no device: the plan is the last thing looked at)
def test_argument_checks_answer_einval_with_a_message(cloudy):
    L, E = cloudy.lib(), cloudy._lib
    nan, inf = float("nan"), float("inf")
    dummy = C.c_void_p(64)   # never dereferenced: every check below precedes any device work
    ok = cloudy.ParcelParams().to_c()
    COAL, COND = cloudy.SRC_COAL, cloudy.SRC_COND

    def call(times=(0.0, 0.25, 1.0), t_save="times", y_save=dummy, n=4, ld=4, t_span=1.0, y_in=dummy, y_out=dummy, sources=COND, w=10.0,
             params=ok, opts="default", **kw):
        o = default_opts(cloudy, **kw) if opts == "default" else opts
        arr = (C.c_double * max(len(times), 1))(*times)
        return L.cloudy_parcel_tsit5_adaptive(None, n, ld, y_in, y_out, sources, None, w, None if params is None else C.byref(params),
                                              t_span, None if o is None else C.byref(o), None, None, None, None, len(times),
                                              arr if t_save == "times" else t_save, y_save)

    def msg():
        return L.cloudy_last_error().decode()

    assert call() == E.EINVAL and msg() == "plan is NULL"          # everything else is in order
    assert call(times=(), t_save=None, y_save=None) == E.EINVAL and msg() == "plan is NULL"   # n_save = 0 with NULL pointers
    assert call(sources=COAL | COND) == E.EINVAL and msg() == "plan is NULL"
    assert call(n=0, ld=0, y_in=None, y_out=None) == E.EINVAL and msg() == "plan is NULL"
    # the save times first (a wrong `sources` / NULL params would answer later)
    assert call(t_save=None, params=None) == E.EINVAL and "t_save" in msg() and "NULL" in msg()
    assert call(y_save=None, params=None) == E.EINVAL and "y_save_dev" in msg() and "NULL" in msg()
    for bad in (nan, inf, -1e-3, 1.0 + 1e-12):
        assert call(times=(0.0, bad), sources=0) == E.EINVAL and "t_save[1]" in msg(), bad
    assert call(times=(0.5, 0.5), params=None) == E.EINVAL and "strictly increasing" in msg()
    cap = int(re.search(r"#define CLOUDY_MAX_SAVE_TIMES (\d+)", open(os.path.join(ROOT, "include", "cloudy_hip.h")).read()).group(1))
    assert call(times=tuple(np.linspace(0.0, 1.0, cap + 1))) == E.EINVAL and "n_save" in msg()
    # then those of cloudy_tsit5_adaptive
    assert_adaptive_opts_refusals(cloudy, call, msg, buffers=("y_in", "y_out"), no_times=dict(times=(), t_save=None, y_save=None),
                                  later=(dict(params=None), dict(sources=0), dict(sources=COAL)))
    # then the parcel's: params, a constant, sources
    assert call(params=None, sources=COAL) == E.EINVAL and msg() == "params is NULL"
    short_p = cloudy.ParcelParams().to_c()
    short_p.struct_size -= 8
    assert call(params=short_p, sources=COAL) == E.EINVAL and "params.struct_size" in msg()
    for field in P.FIELDS:
        for bad in (0.0, -1.0, nan):
            p = cloudy.ParcelParams(**{field: bad}).to_c()
            assert call(params=p, sources=COAL) == E.EINVAL and f"params.{field}" in msg() and "positive" in msg(), (field, bad)
    for bad in (COAL, 0, 4, -1):
        assert call(sources=bad) == E.EINVAL and "sources" in msg() and "CLOUDY_SRC_COND" in msg(), bad
    assert call(w=nan) == E.EINVAL and msg() == "plan is NULL"     # (the updraft speed is the caller's, as in the fixed-step call)


# ---- 3. the plan-time unit
@pytest.mark.parametrize("case", ["gamma", "exp_gamma", "cfg3b", "numerical"])
def test_parcel_adaptive_unit_compiles_without_a_gpu(cloudy, case, tmp_path, monkeypatch):
    """cloudy_jit_selfcheck compiles every unit the runtime could request for a plan (the plans of
    test_parcel_unit_compiles_without_a_gpu): exactly one dumped unit includes adaptive_thermo.hpp; it defines, once each, the
    condensation kernel with and without snapshots and -- tensor plans whose thresholds are all Inf -- the coalescence +
    condensation kernel with and without; it defines no kernel of another unit and names none of the headers the other units'
    tests look for; its code object holds the kernels."""
    monkeypatch.setenv("CLOUDY_HIP_JIT_DUMP", str(tmp_path))
    L = cloudy.lib()
    if case == "numerical":
        d = cloudy.NumericalPlan.make_desc([1, 1], cloudy.LinearKernelFunction(5e-3), bench.NORMS, 10, quad_mode=cloudy.QUAD_FIXED)
        keep = None
    elif case == "cfg3b":
        spec = bench.workload_spec("cfg3b")
        d, keep = cloudy.Plan.make_desc([1] * spec["n_modes"], bench.kernel_matrix(spec), spec["thresholds"], bench.NORMS, 0)
    else:
        types = [1] if case == "gamma" else [0, 1]
        d, keep = cloudy.Plan.make_desc(types, np.array([[1.0]]), (INF,) * len(types), NORMS, 0)
    assert L.cloudy_jit_selfcheck(C.byref(d), b"gfx950") == 0, L.cloudy_last_error().decode()
    texts = {f: open(tmp_path / f).read() for f in sorted(os.listdir(tmp_path)) if f.endswith(".hip")}
    units = [f for f, text in texts.items() if "adaptive_thermo.hpp" in text]
    assert len(units) == 1, units
    text = texts[units[0]]
    kernels = re.findall(r"__global__ void [^\n]*? (cloudy_jit_\w+)\(", text)
    want = ["cloudy_jit_parcel_adaptive_cond_", "cloudy_jit_parcel_adaptive_cond_dense_"]
    if case in ("gamma", "exp_gamma"):
        want += ["cloudy_jit_parcel_adaptive_coalcond_", "cloudy_jit_parcel_adaptive_coalcond_dense_"]
    assert len(kernels) == len(want) and all(k.startswith(w) for k, w in zip(kernels, want)), kernels
    assert len(set(kernels)) == len(kernels)
    assert not any("cloudy_jit_parcel_adaptive" in t for f, t in texts.items() if f != units[0])
    for other in ("parcel.hpp", "adaptive.hpp", "adaptive_box.hpp", "box_sources.hpp", "cloudy_jit_box", "cloudy_jit_rainshaft",
                  " cloudy_jit_parcel_cond_", " cloudy_jit_parcel_rhs_", " cloudy_jit_parcel_coalcond_", "cloudy_jit_adaptive_tsit5",
                  "cloudy_jit_dense_tsit5"):
        assert other not in text, other
    assert text.count("n_save, t_save, y_save)") == len(want) // 2 and "cloudy::SRC_COND>" in text
    code = open(tmp_path / units[0].replace(".hip", ".co"), "rb").read()
    assert len(code) > 1000 and all(k.encode() in code for k in kernels)


# ---- 4. the restatement on the decade batch
@pytest.mark.parametrize("n,reltol,lo,hi", [(257, 1e-6, 2, 36), (257, 1e-9, 15, 55), (65, 1e-6, 4, 36), (65, 1e-9, 18, 54)])
def test_restatement_on_the_decade_batch(n, reltol, lo, hi):
    """Measured on the restatement (every status 0): attempts 2 .. 36 (n = 257, reltol 1e-6; at most 5 rejected), 15 .. 55 (257,
    1e-9), 4 .. 36 (65, 1e-6), 18 .. 54 (65, 1e-9).  Under last-bit noise of the right-hand side 0 parcels change (accepted,
    rejected) and the end state moves per evaluation by at most 1.3e-13 (1e-6) / 8.9e-15 (1e-9) of |y0| + |y|.  Against the
    reltol = 1e-11 run (n = 65), per plane (S, p, T, q_v, M0, M1): (4.7e-7, 1.2e-10, 1.4e-8, 2.1e-7, 0, 1.6e-5) at 1e-6 and
    (2.2e-10, 1.6e-15, 6.5e-12, 9.6e-11, 0, 3.3e-10) at 1e-9.  Asserted: the ranges, status 0, flips <= 5 % of n, the movement of the
    others < 1e-11 (TOL_EVAL), the error <= 1e-4 at 1e-6 and <= 1e-8 at 1e-9 -- but for (n = 257, reltol 1e-6): that batch holds parcels
    the 65 do not, and there the restatement itself is 5.3e-4 off in M1 (1.1e-5 in S) -- a parcel that reaches t_span in two attempts
    -- so no implementation of this controller meets 1e-4 there; the figure is printed, and the GPU tests bound the device per parcel
    by the restatement's own error.  (n = 257 at 1e-9: 7.8e-10 in M1, asserted.)"""
    y0, _, base = decade_case(n, reltol)
    _, _, pert = decade_run(n, reltol, perturb=last_bit_noise(1))
    attempts = base["accepted"] + base["rejected"]
    diff = (base["accepted"] != pert["accepted"]) | (base["rejected"] != pert["rejected"])
    moved = float((rel_to(pert["u"], base["u"], y0) / base["evals"])[:, ~diff].max())
    err = rel_to(base["u"], decade_tight(n)["u"], y0).max(axis=1)
    print(f"n={n} reltol={reltol:g}: attempts {attempts.min()} .. {attempts.max()}, rejected at most {base['rejected'].max()}; "
          f"{int(diff.sum())} parcels change (accepted, rejected) under last-bit noise, the others move by {moved:.1e} x evaluations; "
          f"error against reltol = 1e-11 per plane {err}")
    assert np.all(base["status"] == DONE) and np.all(pert["status"] == DONE) and np.all(base["t"] == T_SPAN)
    assert (attempts.min(), attempts.max()) == (lo, hi)
    if (n, reltol) == (257, 1e-6):
        assert base["rejected"].max() == 5
    assert diff.sum() <= 0.05 * n, diff.sum()
    assert moved < TOL_EVAL, moved
    if (n, reltol) != (257, 1e-6):   # (n = 257 holds a parcel whose M1 is 5.3e-4 off at reltol 1e-6, whatever steps it: the docstring)
        assert np.all(err <= (1e-4 if reltol == 1e-6 else 1e-8)), err
    assert np.array_equal(decade_tight(n)["status"], np.zeros(n, np.int64))


# ---- 5. the same sensitivity for COAL | COND
def test_decisions_are_insensitive_to_the_last_bit_of_the_coalcond_rhs(oracle):
    """Two Gamma modes, thresholds Inf, GOLOVIN (b = 50) and the two-Gamma state of tests/test_gpu_parcel.py scaled per parcel by
    N / 2e8 with N and w as in the decade batch (default_rng(5)), the tendencies from the oracle, n = 257, reltol 1e-6.  Picked on
    the restatement: seed 5, t_span = 5 s.  Measured: every status 0, attempts 2 .. 19, 0 parcels change (accepted, rejected) under
    last-bit noise, the others move by 3.4e-16 x evaluations, and coalescence moves all six moment planes by 0.19 .. 0.92 of
    |y0| + |y| (S by 7e-4, q_v by 3e-4)."""
    n = 257
    y0, _, base = two_gamma_case(n)
    _, _, pert = two_gamma_run(oracle, n, perturb=last_bit_noise(1))
    _, _, cond_only = two_gamma_run(oracle, n, coal=False)
    attempts = base["accepted"] + base["rejected"]
    diff = (base["accepted"] != pert["accepted"]) | (base["rejected"] != pert["rejected"])
    moved = float((rel_to(pert["u"], base["u"], y0) / base["evals"])[:, ~diff].max())
    coal_moves = rel_to(cond_only["u"], base["u"], y0).max(axis=1)
    print(f"COAL | COND n={n}: attempts {attempts.min()} .. {attempts.max()}; {int(diff.sum())} parcels change (accepted, rejected); the "
          f"others move by {moved:.1e} x evaluations; coalescence moves the planes by {coal_moves}")
    assert np.all(base["status"] == DONE) and np.all(pert["status"] == DONE)
    assert attempts.max() >= 5
    assert diff.sum() <= 0.05 * n, diff.sum()
    assert moved < TOL_EVAL, moved
    assert (coal_moves[4:] > 1e-4).sum() >= 2, coal_moves


# ---- 6. Rogers 1975 through dense output
def test_rogers_1975_through_dense_output():
    """the monodisperse driver case, 41 save times 0.5 k, reltol 1e-6, on the restatement: supersaturation within 0.12 percentage
    points and mean radius within 0.05 um of Rogers's points, the bounds of test_restatement_against_rogers_1975."""
    y0, ts = rogers_states()
    rhs = lambda Y: P.parcel_rhs_numpy(P.DEFAULTS, Y, 10.0, [1], monodisperse_cond_closed(P.DEFAULTS))  # noqa: E731
    res = adaptive_tsit5(rhs, y0, T_SPAN, dict(reltol=1e-6, abstol=1e-9, max_steps=10000, plane_norms=decade_norms()), t_save=ts)
    assert res["status"][0] == DONE and np.isfinite(res["saved"]).all()
    d_ss, d_r = rogers_from_series(ts, res["saved"][:, :, 0])
    print(f"dense output vs Rogers 1975: supersaturation {d_ss:.4f} percentage points, radius {d_r:.4f} um; "
          f"{res['accepted'][0]} accepted, {res['rejected'][0]} rejected steps")
    assert d_ss <= 0.12 and d_r <= 0.05, (d_ss, d_r)
