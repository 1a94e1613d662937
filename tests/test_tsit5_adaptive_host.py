"""CPU-only checks of the per-parcel adaptive Tsit5 (cloudy_tsit5_adaptive, csrc/adaptive.hpp): the NumPy restatement of the
algorithm (tsit5_restated.adaptive_tsit5, its own copy of every constant, vectorised over parcels with per-parcel masks), the order
conditions of the error weights, the restatement against the closed form of the single-mode Golovin box, the sensitivity of its
accept / reject decisions to the last bit of the right-hand side on the batches the GPU tests use, every argument check of the C
entry point, and the plan-time unit compiling for gfx950 without a device.

tests/test_gpu_tsit5_adaptive.py runs the same restatement on the oracle's right-hand side as the device's reference."""
import ctypes as C
import functools
import inspect
import os

import numpy as np
import pytest

import bench
from test_host_abi import INF, ROOT, _c_prototypes, _julia_ccalls
from tsit5_restated import (A_ROWS, BTILDE, C_NODES, DONE, EPS, adaptive_tsit5, assert_adaptive_opts_refusals, default_opts, last_bit_noise,
                            plane_norms)

# ---- the batches (shared with the GPU tests): picked on the oracle alone
GOLOVIN_B = 5.0
GOLOVIN_KC = [[0.0, GOLOVIN_B], [GOLOVIN_B, 0.0]]
GOLOVIN_T = 0.6     # b M1 t_span between 3e-3 and 3 over the batch
TOLS = (1e-6, 1e-9)


def golovin_batch(dist, n, seed=3):
    """One mode, Gamma (3 planes) or Exponential (2), number concentrations log-uniform over three decades (1e6 .. 1e9), shuffled;
    n = 1: the densest parcel"""
    rng = np.random.default_rng(seed)
    nn = 1e9 * 10.0 ** (-3.0 * (np.arange(n) / max(n - 1, 1)))
    rng.shuffle(nn)
    th = 0.5e-9 * (1 + 0.3 * rng.uniform(size=n))
    if dist == "gamma":
        k = 2.0
        return np.stack([nn, nn * k * th, nn * k * (k + 1) * th * th])
    return np.stack([nn, nn * 2 * th])


def golovin_exact(u0, t):
    """K = b (x + y), thresholds Inf: dM0 = -b M0 M1, dM1 = 0, dM2 = 2 b M1 M2"""
    out = u0.copy()
    out[0] = u0[0] * np.exp(-GOLOVIN_B * u0[1] * t)
    if u0.shape[0] == 3:
        out[2] = u0[2] * np.exp(2 * GOLOVIN_B * u0[1] * t)
    return out


def plane_errors(got, exact, u0):
    """per plane: max over parcels of |got - exact| / (|u0| + |exact|)"""
    return (np.abs(got - exact) / np.maximum(np.abs(u0) + np.abs(exact), 1e-300)).max(axis=1)


def golovin_case(oracle, dist, n, reltol, seed=3):
    """-> (u0, exact, the restatement's result, its per-plane errors against the closed form)"""
    types, nprog = ([oracle.GAMMA], (3,)) if dist == "gamma" else ([oracle.EXPONENTIAL], (2,))
    op = oracle.make_params(types, np.array(GOLOVIN_KC), (INF,), norms=bench.NORMS)
    u0 = golovin_batch(dist, n, seed)
    res = adaptive_tsit5(lambda u: oracle.rhs_coal_batch(op, u), u0, GOLOVIN_T,
                         dict(reltol=reltol, abstol=1e-9, max_steps=10000, plane_norms=plane_norms(nprog)))
    exact = golovin_exact(u0, GOLOVIN_T)
    return u0, exact, res, plane_errors(res["u"], exact, u0)


# t_span of the two-Gamma batches: the densest parcels take 5 .. 10 attempts at reltol = 1e-6, more than half of the batch one step
# (the oracle alone: all-Inf 1 .. 10 attempts over 2e-2; fixed thresholds 1 .. 6 over 4e-3, moving thresholds 1 .. 5 over 1e-3)
TWO_GAMMA_T = {"allinf": 2e-2, "fixed": 4e-3, "moving": 1e-3}


def two_gamma_batch(n, seed=21, kind="allinf"):
    """Two Gamma modes, the cloud mode's number concentration log-uniform over three decades (1e6 .. 1e9).  All-Inf plans:
    bench.synth_moments without degenerate parcels.  Thresholded plans: the same cloud mode beside a POPULATED rain mode (mean
    mass 2e-9 .. 2e-8; n 1e6 .. 1e8 under the fixed threshold, 1e5 .. 1e7 under the moving one).  With synth_moments' rain mode (n 1 .. 1e5) the transfer across the threshold refills a nearly
    empty mode by factors up to 1e6 and drives its shape onto the closure's clamp (k = 10), where one ulp of a stage state decides
    the closure (test_gpu_parity.py masks such parcels for that reason): there the restatement, driven by the oracle alone with
    its right-hand side multiplied by 1 +- 1e-15 per entry, moves its own end state by 7e-12 (fixed) and 9e-9 (moving) x
    evaluations on a handful of parcels -- no reference at 1e-13.  On the populated batches no parcel ends on a clamp and the same
    measure is below 1e-15 (with noise of 2e-14, the size of the device's difference from the oracle per evaluation of these
    plans: fixed 8e-16, moving 2e-15) (test_decisions_are_insensitive_to_the_last_bit_of_the_rhs asserts 1e-14)."""
    if kind == "allinf":
        return bench.synth_moments(2, n, seed, degenerate_frac=0.0)
    rng = np.random.Generator(np.random.Philox(key=seed))
    cloud = bench._gamma_mode(rng, n, 1e6, 1e9, 0.5, 8.0, 1e-11, 1e-9)
    n_lo = 1e6 if kind == "fixed" else 1e5
    rain = bench._gamma_mode(rng, n, n_lo, 100 * n_lo, 1.0, 6.0, 2e-9, 2e-8)
    return np.ascontiguousarray(np.concatenate([cloud, rain]))


def two_gamma_case(oracle, kind):
    """-> (oracle params, thresholds, moving) of the decision-parity plans: the bench's cfg3a matrix with thresholds Inf or
    (5e-9, Inf), and the MovingThreshold example plan's percentiles (0.9, 1.0) on the same matrix"""
    kc = bench.kernel_matrix(bench.workload_spec("cfg3a"))
    thr, moving = {"allinf": ((INF, INF), False), "fixed": ((5e-9, INF), False), "moving": ((0.9, 1.0), True)}[kind]
    op = oracle.make_params([oracle.GAMMA] * 2, kc, thr, norms=bench.NORMS, threshold_style=1 if moving else 0)
    return op, kc, thr, moving


def two_gamma_reference(oracle, kind, n, reltol=1e-6, max_steps=10000, dt=None, t_span=None, seed=21, perturb=None):
    op, _, _, _ = two_gamma_case(oracle, kind)
    u0 = two_gamma_batch(n, seed, kind)
    t_span = TWO_GAMMA_T[kind] if t_span is None else t_span
    rhs = (lambda u: oracle.rhs_coal_batch(op, u)) if perturb is None else (lambda u: oracle.rhs_coal_batch(op, u) * perturb(u.shape))
    res = adaptive_tsit5(rhs, u0, t_span, dict(reltol=reltol, abstol=1e-9, max_steps=max_steps, dt=dt,
                                               plane_norms=plane_norms((3, 3)), normalised=kind == "allinf"))
    return u0, res


@functools.lru_cache(maxsize=None)
def two_gamma_reference_cached(kind, n, max_steps=10000):
    """the unperturbed reference of a batch, computed once per session and shared (treat the arrays as read-only)"""
    from oracle import cloudy_oracle

    return two_gamma_reference(cloudy_oracle, kind, n, max_steps=max_steps)


# ---- 1. order conditions
def test_error_weights_and_tableau_order_conditions():
    c = np.array(C_NODES)
    for p in range(4):
        s = sum(b * cj**p for b, cj in zip(BTILDE, c))
        print(f"sum bt_j c_j^{p} = {s:.3e}")
        assert abs(s) <= 1e-15, (p, s)
    # row sums of a equal c: every coefficient is a decimal rounded to a double (half an ulp each, entries up to 13 in size), so the
    # exactly summed row may miss c_i by eps/2 sum_j |a_ij|; math.fsum adds no rounding of its own beyond the last
    import math

    for row, cj in zip(A_ROWS, c[1:]):
        assert abs(math.fsum(row) - cj) <= EPS * sum(abs(a) for a in row), (row, cj)
    # the device's copy of the error weights is this one, digit for digit
    text = open(os.path.join(ROOT, "cloudy.jl_amd", "csrc", "adaptive.hpp")).read()
    import re

    for j, b in enumerate(BTILDE, 1):
        assert float(re.search(rf"\bbt{j} = (-?[0-9.e-]+)", text).group(1)) == b, j


# ---- 2. the restatement against the closed form
@pytest.mark.parametrize("dist", ["gamma", "exponential"])
@pytest.mark.parametrize("reltol", TOLS)
def test_restatement_against_the_golovin_closed_form(oracle, dist, reltol):
    """64 parcels, n over three decades, b M1 t_span from 3e-3 to 3: the densest parcels take tens of steps, the sparsest one.
    A controller that keeps the local error per step below reltol x scale leaves a global error of (steps) x reltol at the most;
    asserted: every plane within 100 reltol of |u0| + |exact| (measured: see the printed values), all statuses 0, t == t_span."""
    u0, exact, res, err = golovin_case(oracle, dist, 64, reltol)
    print(f"{dist} reltol={reltol:g}: max error per plane {err}, attempts {(res['accepted'] + res['rejected']).min()}.."
          f"{(res['accepted'] + res['rejected']).max()}, rejected {res['rejected'].sum()}")
    assert np.all(res["status"] == DONE) and np.all(res["t"] == GOLOVIN_T)
    assert np.all(err <= 100 * reltol), err
    assert res["accepted"].min() >= 1 and res["accepted"].max() > 4 * res["accepted"].min()
    assert np.array_equal(res["u"][1], u0[1]) or np.allclose(res["u"][1], u0[1], rtol=1e-13, atol=0)   # M1 is conserved


# ---- 3. sensitivity of the decisions to the last bit of the right-hand side
@pytest.mark.parametrize("case,n,reltol,max_steps", [
    ("golovin_gamma", 257, 1e-6, 10000), ("golovin_gamma", 257, 1e-9, 10000), ("golovin_exponential", 257, 1e-6, 10000),
    ("golovin_exponential", 257, 1e-9, 10000), ("allinf", 257, 1e-6, 10000), ("allinf", 257, 1e-6, 3), ("fixed", 65, 1e-6, 10000),
    ("fixed", 257, 1e-6, 10000), ("moving", 65, 1e-6, 10000), ("moving", 257, 1e-6, 10000)])
def test_decisions_are_insensitive_to_the_last_bit_of_the_rhs(oracle, case, n, reltol, max_steps):
    """The GPU tests compare (accepted, rejected) per parcel with this restatement, whose right-hand side differs from the
    device's in the last bits.  With every entry of the right-hand side multiplied by 1 +- 1e-15, fewer than 1 % of the parcels
    of every batch whose counts those tests compare (sizes, tolerances and the max_steps = 3 run included) may change theirs."""
    moved = 0.0
    if case.startswith("golovin"):
        dist = case.split("_")[1]
        types, nprog = ([oracle.GAMMA], (3,)) if dist == "gamma" else ([oracle.EXPONENTIAL], (2,))
        op = oracle.make_params(types, np.array(GOLOVIN_KC), (INF,), norms=bench.NORMS)
        u0 = golovin_batch(dist, n)
        o = dict(reltol=reltol, abstol=1e-9, max_steps=max_steps, plane_norms=plane_norms(nprog))
        base = adaptive_tsit5(lambda u: oracle.rhs_coal_batch(op, u), u0, GOLOVIN_T, o)
        noise = last_bit_noise(1)
        pert = adaptive_tsit5(lambda u: oracle.rhs_coal_batch(op, u) * noise(u.shape), u0, GOLOVIN_T, o)
    else:
        _, base = two_gamma_reference_cached(case, n, max_steps)
        _, pert = two_gamma_reference(oracle, case, n, max_steps=max_steps, perturb=last_bit_noise(1))
    diff = (base["accepted"] != pert["accepted"]) | (base["rejected"] != pert["rejected"])
    changed = int(diff.sum())
    if not case.startswith("golovin") and max_steps > 3:   # (a budget-stopped parcel is compared where it stopped: test_max_steps_budget)
        u0 = two_gamma_batch(n, kind=case)
        rel = np.abs(pert["u"] - base["u"]) / np.maximum(np.abs(u0) + np.abs(base["u"]), 1e-300) / base["evals"]
        moved = float(rel[:, ~diff].max())
    print(f"{case}: {changed} of {n} parcels change (accepted, rejected) under last-bit noise of the right-hand side; the end state "
          f"of the others moves by {moved:.1e} x evaluations")
    assert changed < 0.01 * n, changed
    # the GPU tests ask the device to agree with this restatement to 1e-13 x evaluations
    # of |u0| + |want| on the parcels with equal counts.  A reference resolves that only if its own response to the last bit of its
    # right-hand side is well below: a tenth, on the same batches.
    assert moved <= 1e-14, moved


# ---- 4. ABI, defaults, argument checks (no device: the plan is the last thing looked at)
def test_symbols_in_header_ctypes_table_julia_shim_and_python(cloudy):
    protos = _c_prototypes()
    assert protos["cloudy_adaptive_opts_init"] == ("void", ["ptr"])
    assert protos["cloudy_tsit5_adaptive"] == ("int", ["ptr", "size_t", "size_t", "ptr", "ptr", "double", "ptr", "ptr", "ptr", "ptr", "ptr"])
    src = open(os.path.join(ROOT, "julia", "CloudyHIP.jl")).read()
    calls = _julia_ccalls(src)
    for name in ("cloudy_adaptive_opts_init", "cloudy_tsit5_adaptive"):
        assert len(cloudy._lib.SYMBOLS[name][1]) == len(protos[name][1]) and hasattr(cloudy.lib(), name)
        mine = [c for c in calls if c[0] == name]
        assert len(mine) == 1 and len(mine[0][2]) == len(protos[name][1]), name
    assert "function solve_tsit5_adaptive!(" in src
    assert "solve_tsit5_adaptive" in cloudy.__all__
    sig = inspect.signature(cloudy.solve_tsit5_adaptive).parameters
    assert list(sig) == ["par", "u", "t_span", "reltol", "abstol", "dt", "max_steps", "out", "dt_dev", "info", "stream", "coal_type"]
    assert (sig["reltol"].default, sig["abstol"].default, sig["dt"].default, sig["max_steps"].default) == (1e-6, 1e-9, None, 10000)
    assert sig["info"].default is False and sig["out"].default is None and sig["dt_dev"].default is None


def test_opts_defaults(cloudy):
    o = default_opts(cloudy)
    assert o.struct_size == C.sizeof(cloudy._lib.AdaptiveOptsC) == 40
    assert (o.reltol, o.abstol, o.dt_init, o.max_steps) == (1e-6, 1e-9, 0.0, 10000)
    cloudy.lib().cloudy_adaptive_opts_init(None)   # (tolerated)


def test_argument_checks_answer_einval_with_a_message(cloudy):
    L, E = cloudy.lib(), cloudy._lib
    dummy = C.c_void_p(64)   # never dereferenced: every check below precedes any device work

    def call(opts="default", n=4, ld=4, t_span=1.0, u_in=dummy, u_out=dummy, **kw):
        o = default_opts(cloudy, **kw) if opts == "default" else opts
        return L.cloudy_tsit5_adaptive(None, n, ld, u_in, u_out, t_span, None if o is None else C.byref(o), None, None, None, None)

    def msg():
        return L.cloudy_last_error().decode()

    assert call() == E.EINVAL and msg() == "plan is NULL"          # everything else is in order
    assert call(n=0, ld=0, u_in=None, u_out=None) == E.EINVAL and msg() == "plan is NULL"
    assert_adaptive_opts_refusals(cloudy, call, msg)


# ---- 5. the plan-time unit
@pytest.mark.parametrize("case", ["gamma", "cfg3a", "cfg3b", "moving", "numerical"])
def test_adaptive_unit_compiles_without_a_gpu(cloudy, case, tmp_path, monkeypatch):
    """cloudy_jit_selfcheck compiles every unit the runtime could request for a plan: for a tensor plan exactly one dumped unit
    names adaptive.hpp, defines the kernel and has a code object; it includes neither parcel.hpp nor box_sources.hpp and defines
    no kernel of another unit; a NumericalCoalStyle description has none."""
    monkeypatch.setenv("CLOUDY_HIP_JIT_DUMP", str(tmp_path))
    L = cloudy.lib()
    if case == "numerical":
        d = cloudy.NumericalPlan.make_desc([1, 1], cloudy.LinearKernelFunction(5e-3), bench.NORMS, 10, quad_mode=cloudy.QUAD_FIXED)
        keep = None
    elif case in ("cfg3a", "cfg3b"):
        spec = bench.workload_spec(case)
        d, keep = cloudy.Plan.make_desc([1] * spec["n_modes"], bench.kernel_matrix(spec), spec["thresholds"], bench.NORMS, 0)
    elif case == "moving":
        d, keep = cloudy.Plan.make_desc([1, 1], bench.kernel_matrix(bench.workload_spec("cfg3a")), (0.9, 1.0), bench.NORMS, 1)
    else:
        d, keep = cloudy.Plan.make_desc([1], np.array(GOLOVIN_KC), (INF,), bench.NORMS, 0)
    assert L.cloudy_jit_selfcheck(C.byref(d), b"gfx950") == 0, L.cloudy_last_error().decode()
    units = [f for f in sorted(os.listdir(tmp_path)) if f.endswith(".hip") and "adaptive.hpp" in open(tmp_path / f).read()]
    if case == "numerical":
        assert units == []
        return
    assert len(units) == 1, units
    text = open(tmp_path / units[0]).read()
    assert "parcel.hpp" not in text and "box_sources.hpp" not in text
    assert "cloudy_jit_parcel" not in text and "cloudy_jit_box" not in text and "cloudy_jit_rainshaft" not in text
    assert text.count(" cloudy_jit_adaptive_tsit5_") == 1
    assert os.path.getsize(tmp_path / units[0].replace(".hip", ".co")) > 1000
