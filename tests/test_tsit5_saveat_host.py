"""CPU-only checks of the dense output of the per-parcel adaptive Tsit5 (cloudy_tsit5_adaptive_saveat, csrc/adaptive.hpp): the
interpolant's coefficients as the kernel holds them against the tableau, the NumPy restatement with snapshots
(tsit5_restated.adaptive_tsit5 with t_save: the same loop plus the snapshot rule) that leaves the integration bit for bit alone, the
restatement against the closed form of the single-mode Golovin box AT THE SAVE TIMES, the ABI, every argument check of the C
entry point, and the plan-time unit with both kernels compiling for gfx950 without a device.

tests/test_gpu_tsit5_saveat.py runs the same restatement on the oracle's right-hand side as the device's reference."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest

import bench
import test_tsit5_adaptive_host as H
from test_host_abi import INF, ROOT, _c_prototypes, _julia_ccalls
from tsit5_restated import (A_ROWS, C_NODES, INTERP, SAVE_FRACS, adaptive_tsit5, assert_adaptive_opts_refusals, default_opts, interp_weights,
                            plane_norms, save_times)


def golovin_saveat_case(oracle, dist, n, reltol, max_steps=10000):
    """-> (u0, t_save, the restatement's result) of the Golovin batch of test_tsit5_adaptive_host at the twelve save times"""
    types, nprog = ([oracle.GAMMA], (3,)) if dist == "gamma" else ([oracle.EXPONENTIAL], (2,))
    op = oracle.make_params(types, np.array(H.GOLOVIN_KC), (INF,), norms=bench.NORMS)
    u0 = H.golovin_batch(dist, n)
    ts = save_times(H.GOLOVIN_T)
    res = adaptive_tsit5(lambda u: oracle.rhs_coal_batch(op, u), u0, H.GOLOVIN_T,
                         dict(reltol=reltol, abstol=1e-9, max_steps=max_steps, plane_norms=plane_norms(nprog)), t_save=ts)
    return u0, ts, res


def golovin_snapshot_errors(saved, u0, ts):
    """per plane: the maximum over the save times of H.plane_errors against the closed form at that time"""
    return np.max([H.plane_errors(saved[j], H.golovin_exact(u0, t), u0) for j, t in enumerate(ts)], axis=0)


@functools.lru_cache(maxsize=None)
def two_gamma_saveat_cached(kind, n, max_steps=10000):
    """the restatement with snapshots on a two-Gamma batch of test_tsit5_adaptive_host, computed once per session and shared
    (treat the arrays as read-only) -> (u0, t_save, result)"""
    from oracle import cloudy_oracle as oracle

    op, _, _, _ = H.two_gamma_case(oracle, kind)
    u0 = H.two_gamma_batch(n, kind=kind)
    ts = save_times(H.TWO_GAMMA_T[kind])
    res = adaptive_tsit5(lambda u: oracle.rhs_coal_batch(op, u), u0, H.TWO_GAMMA_T[kind],
                         dict(reltol=1e-6, abstol=1e-9, max_steps=max_steps, plane_norms=plane_norms((3, 3)),
                              normalised=kind == "allinf"), t_save=ts)
    return u0, ts, res


# ---- 1. the interpolant against the tableau, on the kernel's own digits
def device_interp_coefficients():
    text = open(os.path.join(ROOT, "cloudy.jl_amd", "csrc", "adaptive.hpp")).read()
    lines = [ln for ln in text.splitlines() if ln.lstrip().startswith("constexpr double") or re.match(r"\s+bi\d_", ln)]
    coef = {}
    for i, name, val in re.findall(r"\bbi(\d)_(s|r1|r2|p|q) = (-?[0-9.e-]+)", "\n".join(lines)):
        coef.setdefault(int(i), {})[name] = float(val)
    return coef


def test_interpolant_against_the_tableau():
    """The coefficients are read out of csrc/adaptive.hpp: b_i(1) = a_7i (the interpolant ends on the 5th-order solution) and
    b_7(1) = 0, b_i(0) = 0, sum_i b_i(th) c_i^p = th^(p+1) / (p+1) for p = 0 .. 3 (4th order) to 1e-14 at nine th; the p = 4
    residual is not zero (it is a 4th-order interpolant, ~1e-3)."""
    coef = device_interp_coefficients()
    assert sorted(coef) == [1, 2, 3, 4, 5, 6, 7], sorted(coef)
    assert {i: set(c) for i, c in coef.items()} == {i: set(c) for i, c in INTERP.items()}
    assert coef == INTERP      # the restatement's copy is the kernel's, digit for digit
    c = np.array(C_NODES)
    b1 = interp_weights(1.0, coef)
    for i in range(6):
        assert abs(b1[i] - A_ROWS[-1][i]) <= 1e-14, (i, b1[i])
    assert b1[6] == 0.0
    assert all(b == 0.0 for b in interp_weights(0.0, coef))
    worst4 = 0.0
    for th in (0.05, 0.1, 0.25, 0.37, 0.5, 0.62, 0.83, 0.95, 1.0):
        b = np.array(interp_weights(th, coef))
        for p in range(4):
            res = float(np.sum(b * c**p) - th ** (p + 1) / (p + 1))
            assert abs(res) <= 1e-14, (th, p, res)
        worst4 = max(worst4, abs(float(np.sum(b * c**4) - th**5 / 5)))
    print(f"largest p = 4 residual over the nine th: {worst4:.2e}")
    assert worst4 > 1e-5


# ---- 2. the restatement leaves the integration alone
@pytest.mark.parametrize("case", ["golovin_gamma", "golovin_exponential", "allinf"])
def test_restatement_integrates_as_the_one_without_snapshots(oracle, case):
    keys = ("u", "t", "dt", "accepted", "rejected", "status", "evals")
    if case == "allinf":
        u0, ts, res = two_gamma_saveat_cached("allinf", 257)
        _, base = H.two_gamma_reference_cached("allinf", 257)
    else:
        dist = case.split("_")[1]
        u0, ts, res = golovin_saveat_case(oracle, dist, 257, 1e-6)
        _, _, base, _ = H.golovin_case(oracle, dist, 257, 1e-6)
    for k in keys:
        assert np.array_equal(np.ascontiguousarray(res[k]).view(np.uint8), np.ascontiguousarray(base[k]).view(np.uint8)), k
    assert res["saved"].shape == (len(SAVE_FRACS), u0.shape[0], 257) and np.isfinite(res["saved"]).all()
    assert np.array_equal(res["saved"][0], u0) and np.array_equal(res["saved"][-1], res["u"])
    assert all(sum(s) == len(SAVE_FRACS) - 1 and len(s) == a for s, a in zip(res["in_step"], res["accepted"]))
    # t_span = 0 and a budget that stops parcels
    zero = adaptive_tsit5(None, u0, 0.0, dict(reltol=1e-6, abstol=1e-9, max_steps=10, plane_norms=np.ones(u0.shape[0])), t_save=[0.0])
    assert np.array_equal(zero["saved"][0], u0)


# ---- 3. the restatement against the closed form at the save times
# Interior (interpolated) error against end-point error of the Golovin batches, per plane: the largest ratio measured on this
# restatement against the closed form on the CPU over both distributions, both tolerances and all planes (the docstring below
# has every value); the assertion allows twice that.
INTERIOR_OVER_END_MEASURED = 3.94


@pytest.mark.parametrize("dist", ["gamma", "exponential"])
@pytest.mark.parametrize("reltol", H.TOLS)
def test_restatement_against_the_golovin_closed_form_at_the_save_times(oracle, dist, reltol):
    """257 parcels, n over three decades, the twelve save times: some parcel has two save times inside one accepted step, some an
    accepted step without one, some a save time in its first and some in its last step.  A 4th-order interpolant inside a
    5th-order step may be worse than the step's end: per plane, the largest error over the save times (the one at t_span among
    them, so the ratio is at least 1) over the error at t_span, measured on this restatement against the closed form --
      Gamma        reltol 1e-6: 2.59 (M0), 1 (M1, conserved), 3.56 (M2);   reltol 1e-9: 3.94, 1, 1.46
      Exponential  reltol 1e-6: 2.18 (M0), 1 (M1);                         reltol 1e-9: 3.34, 1
    -- asserted: at most 2 x 3.94 in every plane, and every snapshot within 100 reltol as the end point is."""
    u0, ts, res = golovin_saveat_case(oracle, dist, 257, reltol)
    assert np.all(res["status"] == 0)
    steps = res["in_step"]
    assert any(max(s) >= 2 for s in steps)                      # two save times inside one accepted step
    assert any(min(s) == 0 for s in steps)                      # an accepted step without a save time
    assert any(s[0] >= 1 for s in steps)                        # a save time in a first step (t_save = 0 belongs to none)
    assert any(s[-1] >= 1 and len(s) > 1 for s in steps)        # ... and in a last step that is not the only one
    exact = H.golovin_exact(u0, H.GOLOVIN_T)
    end = H.plane_errors(res["u"], exact, u0)
    interior = golovin_snapshot_errors(res["saved"], u0, ts)
    print(f"{dist} reltol={reltol:g}: end-point error per plane {end}, largest over the save times {interior}, ratio {interior / end}")
    assert np.all(interior <= 100 * reltol), interior
    assert np.all(interior <= 2 * INTERIOR_OVER_END_MEASURED * end), interior / end


# ---- 4. ABI
def test_symbols_in_header_ctypes_table_julia_shim_and_python(cloudy):
    protos = _c_prototypes()
    name = "cloudy_tsit5_adaptive_saveat"
    assert protos[name] == ("int", protos["cloudy_tsit5_adaptive"][1] + ["size_t", "ptr", "ptr"])
    assert len(cloudy._lib.SYMBOLS[name][1]) == len(protos[name][1]) == 14 and hasattr(cloudy.lib(), name)
    src = open(os.path.join(ROOT, "julia", "CloudyHIP.jl")).read()
    mine = [c for c in _julia_ccalls(src) if c[0] == name]
    assert len(mine) == 1 and len(mine[0][2]) == 14
    assert "function solve_tsit5_adaptive_saveat!(" in src
    assert "solve_tsit5_adaptive_saveat" in cloudy.__all__
    sig = inspect.signature(cloudy.solve_tsit5_adaptive_saveat).parameters
    plain = list(inspect.signature(cloudy.solve_tsit5_adaptive).parameters)
    assert list(sig) == plain[:3] + ["saveat"] + plain[3:]
    assert (sig["reltol"].default, sig["abstol"].default, sig["dt"].default, sig["max_steps"].default) == (1e-6, 1e-9, None, 10000)
    assert sig["info"].default is False and sig["out"].default is None and sig["dt_dev"].default is None
    assert sig["saveat"].default is inspect.Parameter.empty
    assert C.sizeof(cloudy._lib.AdaptiveOptsC) == 40


# ---- 5. argument checks (no device: the plan is the last thing looked at)
def test_argument_checks_answer_einval_with_a_message(cloudy):
    L, E = cloudy.lib(), cloudy._lib
    nan, inf = float("nan"), float("inf")
    dummy = C.c_void_p(64)   # never dereferenced: every check below precedes any device work
    cap = int(re.search(r"#define CLOUDY_MAX_SAVE_TIMES (\d+)", open(os.path.join(ROOT, "include", "cloudy_hip.h")).read()).group(1))

    def call(times=(0.0, 0.25, 1.0), n_save=None, t_save="times", u_save=dummy, t_span=1.0, opts="default", ld=4, u_in=dummy, u_out=dummy,
             **kw):
        o = default_opts(cloudy, **kw) if opts == "default" else opts
        arr = (C.c_double * max(len(times), 1))(*times)
        return L.cloudy_tsit5_adaptive_saveat(None, 4, ld, u_in, u_out, t_span, None if o is None else C.byref(o), None, None, None, None,
                                              len(times) if n_save is None else n_save, arr if t_save == "times" else t_save, u_save)

    def msg():
        return L.cloudy_last_error().decode()

    assert call() == E.EINVAL and msg() == "plan is NULL"          # everything else is in order
    assert call(times=(), t_save=None, u_save=None) == E.EINVAL and msg() == "plan is NULL"   # n_save = 0 with NULL pointers
    assert call(times=(0.0,), t_span=0.0) == E.EINVAL and msg() == "plan is NULL"
    assert call(t_save=None) == E.EINVAL and "t_save" in msg() and "NULL" in msg()
    assert call(u_save=None) == E.EINVAL and "u_save_dev" in msg() and "NULL" in msg()
    for bad in (nan, inf, -inf, -1e-3, 1.0 + 1e-12):
        assert call(times=(0.0, bad)) == E.EINVAL and "t_save[1]" in msg(), bad
    assert call(times=(-1e-300,)) == E.EINVAL and "t_save[0]" in msg()
    for bad in ((0.5, 0.5), (0.5, 0.25), (0.0, 0.2, 0.2, 1.0)):
        assert call(times=bad) == E.EINVAL and "t_save" in msg() and "strictly increasing" in msg(), bad
    big = tuple(np.linspace(0.0, 1.0, cap + 1))
    assert call(times=big) == E.EINVAL and "n_save" in msg() and str(cap) in msg()
    assert call(times=big[:cap]) == E.EINVAL and msg() == "plan is NULL"
    # the checks of cloudy_tsit5_adaptive follow
    assert call(times=(0.0,), t_span=nan) == E.EINVAL    # (a save time compared with a t_span that is no number)
    assert_adaptive_opts_refusals(cloudy, call, msg, no_times=dict(times=(), t_save=None, u_save=None))


# ---- 6. the plan-time unit
@pytest.mark.parametrize("case", ["gamma", "cfg3a", "cfg3b", "moving", "numerical"])
def test_adaptive_unit_holds_both_kernels_and_compiles_without_a_gpu(cloudy, case, tmp_path, monkeypatch):
    """cloudy_jit_selfcheck compiles every unit the runtime could request for a plan: the single unit that names adaptive.hpp
    defines the kernel of cloudy_tsit5_adaptive and the one of cloudy_tsit5_adaptive_saveat, once each, and has a code object
    that holds both; a NumericalCoalStyle description has neither."""
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
        d, keep = cloudy.Plan.make_desc([1], np.array(H.GOLOVIN_KC), (INF,), bench.NORMS, 0)
    assert L.cloudy_jit_selfcheck(C.byref(d), b"gfx950") == 0, L.cloudy_last_error().decode()
    texts = {f: open(tmp_path / f).read() for f in sorted(os.listdir(tmp_path)) if f.endswith(".hip")}
    units = [f for f, text in texts.items() if "adaptive.hpp" in text]
    if case == "numerical":
        assert units == []
        assert not any("cloudy_jit_adaptive_tsit5" in text or "cloudy_jit_dense_tsit5" in text for text in texts.values())
        return
    assert len(units) == 1, units
    text = texts[units[0]]
    plain = re.findall(r"__global__ void [^\n]*? (cloudy_jit_adaptive_tsit5_\w+)\(", text)
    dense = re.findall(r"__global__ void [^\n]*? (cloudy_jit_dense_tsit5_\w+)\(", text)
    assert len(plain) == 1 and len(dense) == 1, (plain, dense)
    assert not any("cloudy_jit_dense_tsit5" in t for f, t in texts.items() if f != units[0])
    assert "n_save, t_save, u_save)" in text and ", true, 256, true>" in text
    code = open(tmp_path / units[0].replace(".hip", ".co"), "rb").read()
    assert len(code) > 1000 and plain[0].encode() in code and dense[0].encode() in code
