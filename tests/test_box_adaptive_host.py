"""CPU-only checks of cloudy_box_tsit5_adaptive (csrc/adaptive_box.hpp): per-parcel adaptive Tsit5 of du/dt = [coal](u) + [cond](u; s, xi).
The reference is the NumPy restatement of the controller (tsit5_restated.adaptive_tsit5, with snapshots: its t_save) on the
unchanged oracle's rhs_coal_batch + rhs_condensation_batch: the restatement against
the closed form of a Monodisperse mode under condensation, the sensitivity of its decisions to the last bit of the combined
right-hand side on the batches the GPU tests use, the ABI, every argument check of the C entry point, and the plan-time unit
compiling for gfx950 without a device.

tests/test_gpu_box_adaptive.py runs the same restatement as the device's reference."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest

import bench
import test_tsit5_adaptive_host as H
from test_host_abi import INF, ROOT, _c_prototypes
from tsit5_restated import (DONE, adaptive_tsit5, assert_adaptive_opts_refusals, assert_symbol_agrees, default_opts, last_bit_noise, plane_norms,
                            save_times)

NAME = "cloudy_box_tsit5_adaptive"
XI_COND = 1e-8      # the closed-form batch
XI_BOX = 1e-5       # the two-Gamma batches: condensation moves five of six planes by 5e-4 .. 7e-2 of |u0| + |u|
COND_T = 200.0
RHO_L = 1000.0
# the per-evaluation bound the project asserts for the condensation right-hand side (tests/test_gpu_box_sources.py)
TOL_EVAL = 1e-11


# ---- the batches (shared with the GPU tests): picked on the oracle alone
def cond_batch(n):
    """One Monodisperse mode (planes M0 = n, M1 = n x0) and a supersaturation per parcel: default_rng(5), three draws in this
    order -- n = 1e9 10^(-3 U), x0 = 1e-10 10^U(-1, 1), s = U(-0.02, 0.05)"""
    rng = np.random.default_rng(5)
    nn = 1e9 * 10.0 ** (-3.0 * rng.uniform(size=n))
    x0 = 1e-10 * 10.0 ** rng.uniform(-1.0, 1.0, size=n)
    s = rng.uniform(-0.02, 0.05, size=n)
    return np.stack([nn, nn * x0]), s


def cond_exact(u0, s, t, xi=XI_COND):
    """M0 constant, M1(t) = n (x0^(2/3) + 2 c xi s t)^(3/2), c = (4 pi / 3)^(2/3) / rho_l^(1/3)"""
    c = (4.0 * np.pi / 3.0) ** (2.0 / 3.0) / RHO_L ** (1.0 / 3.0)
    out = u0.copy()
    out[1] = u0[0] * ((u0[1] / u0[0]) ** (2.0 / 3.0) + 2.0 * c * xi * s * t) ** 1.5
    return out


def cond_params(oracle):
    return oracle.make_params([oracle.MONODISPERSE], np.array([[1.0]]), (INF,), norms=bench.NORMS)


@functools.lru_cache(maxsize=None)
def cond_case(n, reltol, saveat=False, max_steps=10000):
    """-> (u0, s, exact at t_span, the restatement's result (with snapshots: at save_times(COND_T)), its per-plane errors);
    computed once per session and shared (treat the arrays as read-only)"""
    from oracle import cloudy_oracle as oracle

    op = cond_params(oracle)
    u0, s = cond_batch(n)
    rhs = lambda u: oracle.rhs_condensation_batch(op, XI_COND, s, u)  # noqa: E731
    opts = dict(reltol=reltol, abstol=1e-9, max_steps=max_steps, plane_norms=plane_norms((2,)))
    res = adaptive_tsit5(rhs, u0, COND_T, opts, t_save=save_times(COND_T) if saveat else None)
    exact = cond_exact(u0, s, COND_T)
    return u0, s, exact, res, H.plane_errors(res["u"], exact, u0)


def box_supersaturation(n):
    return np.random.default_rng(0).uniform(-0.02, 0.05, n)


def box_rhs(oracle, kind, n, perturb=None):
    """the combined oracle right-hand side of a two-Gamma batch of test_tsit5_adaptive_host: coalescence + condensation"""
    op, _, _, _ = H.two_gamma_case(oracle, kind)
    s = box_supersaturation(n)
    f = lambda u: oracle.rhs_coal_batch(op, u) + oracle.rhs_condensation_batch(op, XI_BOX, s, u)  # noqa: E731
    return f if perturb is None else (lambda u: f(u) * perturb(u.shape))


def box_reference(oracle, kind, n, max_steps=10000, perturb=None, saveat=False):
    u0 = H.two_gamma_batch(n, kind=kind)
    opts = dict(reltol=1e-6, abstol=1e-9, max_steps=max_steps, plane_norms=plane_norms((3, 3)), normalised=kind == "allinf")
    t_span = H.TWO_GAMMA_T[kind]
    rhs = box_rhs(oracle, kind, n, perturb)
    return u0, adaptive_tsit5(rhs, u0, t_span, opts, t_save=save_times(t_span) if saveat else None)


@functools.lru_cache(maxsize=None)
def box_reference_cached(kind, n, max_steps=10000, saveat=False):
    """the unperturbed reference of a batch, once per session and shared (treat the arrays as read-only)"""
    from oracle import cloudy_oracle

    return box_reference(cloudy_oracle, kind, n, max_steps=max_steps, saveat=saveat)


# ---- 1. ABI
def test_symbol_in_header_ctypes_table_julia_shim_and_python(cloudy):
    protos = _c_prototypes()
    plain, box = protos["cloudy_tsit5_adaptive_saveat"][1], protos["cloudy_box_ssprk33_steps"][1]
    assert len(protos[NAME][1]) == 18
    assert_symbol_agrees(cloudy, NAME, plain[:5] + box[5:9] + plain[5:])
    src = open(os.path.join(ROOT, "julia", "CloudyHIP.jl")).read()
    assert re.search(r"function solve_box_tsit5_adaptive!\(u, plan::Plan, t_span, xi, s; coal::Bool = true, cond::Bool = true", src)
    assert "solve_box_tsit5_adaptive" in cloudy.__all__
    sig = inspect.signature(cloudy.solve_box_tsit5_adaptive).parameters
    assert list(sig) == ["par", "u", "t_span", "xi", "s", "coal", "cond", "saveat", "reltol", "abstol", "dt", "max_steps", "out", "dt_dev",
                         "info", "stream", "coal_type"]
    assert (sig["coal"].default, sig["cond"].default, sig["saveat"].default) == (True, True, None)
    assert (sig["reltol"].default, sig["abstol"].default, sig["dt"].default, sig["max_steps"].default) == (1e-6, 1e-9, None, 10000)
    assert sig["info"].default is False and sig["out"].default is None and sig["dt_dev"].default is None
    with pytest.raises(ValueError, match="Invalid coal style"):
        cloudy.solve_box_tsit5_adaptive(None, None, 1.0, 1e-8, 0.05, coal_type="analytical")
    header = open(os.path.join(ROOT, "include", "cloudy_hip.h")).read()
    assert "box_model_helpers.jl:55-67" in header[header.index("Per-parcel ADAPTIVE Tsit5 of the box"):header.index("int " + NAME)]
    assert "Condensation.jl:22-37" in header[header.index("Per-parcel ADAPTIVE Tsit5 of the box"):header.index("int " + NAME)]


# ---- 2. argument checks (no device: the plan is the last thing looked at)
def test_argument_checks_answer_einval_with_a_message(cloudy):
    L, E = cloudy.lib(), cloudy._lib
    nan, inf = float("nan"), float("inf")
    dummy = C.c_void_p(64)   # never dereferenced: every check below precedes any device work

    def call(times=(0.0, 0.25, 1.0), t_save="times", u_save=dummy, n=4, ld=4, t_span=1.0, u_in=dummy, u_out=dummy, sources=3, s=0.05,
             xi=1e-8, opts="default", **kw):
        o = default_opts(cloudy, **kw) if opts == "default" else opts
        arr = (C.c_double * max(len(times), 1))(*times)
        return L.cloudy_box_tsit5_adaptive(None, n, ld, u_in, u_out, sources, None, s, xi, t_span, None if o is None else C.byref(o), None,
                                           None, None, None, len(times), arr if t_save == "times" else t_save, u_save)

    def msg():
        return L.cloudy_last_error().decode()

    assert call() == E.EINVAL and msg() == "plan is NULL"          # everything else is in order
    assert call(times=(), t_save=None, u_save=None) == E.EINVAL and msg() == "plan is NULL"   # n_save = 0 with NULL pointers
    for good in (1, 2, 3):
        assert call(sources=good) == E.EINVAL and msg() == "plan is NULL"
    assert call(s=nan) == E.EINVAL and msg() == "plan is NULL"     # (the supersaturation is the caller's, as in the fixed-step call)
    # the save times first
    assert call(t_save=None) == E.EINVAL and "t_save" in msg() and "NULL" in msg()
    assert call(u_save=None) == E.EINVAL and "u_save_dev" in msg() and "NULL" in msg()
    for bad in (nan, inf, -1e-3, 1.0 + 1e-12):
        assert call(times=(0.0, bad), sources=0) == E.EINVAL and "t_save[1]" in msg(), bad
    assert call(times=(0.5, 0.5)) == E.EINVAL and "strictly increasing" in msg()
    cap = int(re.search(r"#define CLOUDY_MAX_SAVE_TIMES (\d+)", open(os.path.join(ROOT, "include", "cloudy_hip.h")).read()).group(1))
    assert call(times=tuple(np.linspace(0.0, 1.0, cap + 1))) == E.EINVAL and "n_save" in msg()
    # then those of cloudy_tsit5_adaptive
    assert_adaptive_opts_refusals(cloudy, call, msg, no_times=dict(times=(), t_save=None, u_save=None),
                                  later=(dict(sources=0), dict(sources=7), dict(xi=nan)))
    # then the box's: sources, xi
    for bad in (0, -1, 4, 7):
        assert call(sources=bad, xi=nan) == E.EINVAL and "sources" in msg() and str(bad) in msg(), bad
    assert call(xi=nan) == E.EINVAL and "xi" in msg()
    assert call(sources=1, xi=nan) == E.EINVAL and "xi" in msg()


# ---- 3. the plan-time unit
@pytest.mark.parametrize("case", ["gamma", "cfg3a", "cfg3b", "moving", "numerical", "cfg3a_f32"])
def test_box_adaptive_unit_holds_both_kernels_per_instance_and_compiles_without_a_gpu(cloudy, case, tmp_path, monkeypatch):
    """cloudy_jit_selfcheck compiles every unit the runtime could request for a plan: exactly one dumped unit includes
    adaptive_box.hpp; it defines, once each, the condensation kernel with and without snapshots and -- tensor plans -- the
    coalescence + condensation kernel with and without, has a code object that holds them, and defines no kernel of another unit.
    The units of cloudy_tsit5_adaptive and cloudy_box_ssprk33_steps keep their kernels."""
    monkeypatch.setenv("CLOUDY_HIP_JIT_DUMP", str(tmp_path))
    L = cloudy.lib()
    if case == "numerical":
        d = cloudy.NumericalPlan.make_desc([1, 1], cloudy.LinearKernelFunction(5e-3), bench.NORMS, 10, quad_mode=cloudy.QUAD_FIXED)
        keep = None
    elif case in ("cfg3a", "cfg3b", "cfg3a_f32"):
        spec = bench.workload_spec(case[:5])
        d, keep = cloudy.Plan.make_desc([1] * spec["n_modes"], bench.kernel_matrix(spec), spec["thresholds"], bench.NORMS, 0,
                                        dtype=1 if case.endswith("f32") else 0)
    elif case == "moving":
        d, keep = cloudy.Plan.make_desc([1, 1], bench.kernel_matrix(bench.workload_spec("cfg3a")), (0.9, 1.0), bench.NORMS, 1)
    else:
        d, keep = cloudy.Plan.make_desc([1], np.array(H.GOLOVIN_KC), (INF,), bench.NORMS, 0)
    assert L.cloudy_jit_selfcheck(C.byref(d), b"gfx950") == 0, L.cloudy_last_error().decode()
    texts = {f: open(tmp_path / f).read() for f in sorted(os.listdir(tmp_path)) if f.endswith(".hip")}
    units = [f for f, text in texts.items() if "adaptive_box.hpp" in text]
    assert len(units) == 1, units
    text = texts[units[0]]
    kernels = re.findall(r"__global__ void [^\n]*? (cloudy_jit_\w+)\(", text)
    want = ["cloudy_jit_box_adaptive_cond_", "cloudy_jit_box_adaptive_cond_dense_"]
    if case != "numerical":
        want += ["cloudy_jit_box_adaptive_coalcond_", "cloudy_jit_box_adaptive_coalcond_dense_"]
    assert len(kernels) == len(want) and all(k.startswith(w) for k, w in zip(kernels, want)), kernels
    assert len(set(kernels)) == len(kernels)
    assert not any("cloudy_jit_box_adaptive" in t for f, t in texts.items() if f != units[0])
    assert text.count("n_save, t_save, u_save)") == len(want) // 2 and "cloudy::SRC_COND>" in text
    if case == "cfg3a_f32":
        assert "const float *u_in" in text and "float *__restrict__ u_save" in text
    code = open(tmp_path / units[0].replace(".hip", ".co"), "rb").read()
    assert len(code) > 1000 and all(k.encode() in code for k in kernels)
    if case != "numerical":
        assert sum(" cloudy_jit_adaptive_tsit5_" in t for t in texts.values()) == 1
    assert sum(" cloudy_jit_box_cond_" in t for t in texts.values()) == 1


# ---- 4. the restatement against the closed form
@pytest.mark.parametrize("reltol", H.TOLS)
def test_restatement_against_the_condensation_closed_form(oracle, reltol):
    """One Monodisperse mode, condensation only, 257 parcels, xi = 1e-8, t_span = 200 (the earliest complete evaporation of the batch
    is at t = 675): M0 is constant and M1 moves by factors 0.59 .. 2.8.  Measured on the oracle: every status 0; attempts 1 .. 8 at
    reltol 1e-6 and 1 .. 16 at 1e-9; the error of plane 1 against the closed form 4.9e-10 and 5.6e-9 -- not monotone in reltol (the
    oracle's right-hand side limits it), which is why the device's bounds are stated against this error and not against reltol.
    Asserted: those ranges and the error <= 1e-7."""
    u0, s, exact, res, err = cond_case(257, reltol)
    attempts = res["accepted"] + res["rejected"]
    print(f"reltol={reltol:g}: attempts {attempts.min()} .. {attempts.max()}, error per plane {err}, "
          f"M1 moves by {(exact[1] / u0[1]).min():.3g} .. {(exact[1] / u0[1]).max():.3g}")
    assert np.all(res["status"] == DONE) and np.all(res["t"] == COND_T)
    assert attempts.min() == 1 and attempts.max() == (8 if reltol == 1e-6 else 16)
    assert (exact[1] / u0[1]).min() < 0.6 and (exact[1] / u0[1]).max() > 2.7 and np.all(exact[1] > 0)
    assert np.all(err <= 1e-7), err
    assert np.allclose(res["u"][0], u0[0], rtol=4e-16, atol=0)


# ---- 5. sensitivity of the decisions to the last bit of the combined right-hand side
@pytest.mark.parametrize("kind,n", [("allinf", 257), ("fixed", 65), ("fixed", 257), ("moving", 65), ("moving", 257)])
def test_decisions_are_insensitive_to_the_last_bit_of_the_combined_rhs(oracle, kind, n):
    """The GPU tests compare (accepted, rejected) per parcel with this restatement, whose right-hand side differs from the
    device's in the last bits.  The batches are two_gamma_batch(n, kind) with rhs_coal_batch + rhs_condensation_batch, xi = 1e-5,
    s = default_rng(0).uniform(-0.02, 0.05, n), t_span = TWO_GAMMA_T[kind] (seed and t_span as test_tsit5_adaptive_host has them:
    no batch, `moving` included, needed another).  With every entry of the right-hand side multiplied by 1 +- 1e-15: at most 5 % of
    the parcels change (accepted, rejected), and the end state of the others moves by less than the tolerance the GPU test asks of
    the device, 1e-11 x evaluations of |u0| + |u|.  Every status is 0; condensation moves the state far above reltol, so a kernel
    that drops the term cannot pass."""
    u0, base = box_reference_cached(kind, n)
    _, pert = box_reference(oracle, kind, n, perturb=last_bit_noise(1))
    _, coal_only = H.two_gamma_reference_cached(kind, n)
    attempts = base["accepted"] + base["rejected"]
    diff = (base["accepted"] != pert["accepted"]) | (base["rejected"] != pert["rejected"])
    scale = np.maximum(np.abs(u0) + np.abs(base["u"]), 1e-300)
    moved = float((np.abs(pert["u"] - base["u"]) / scale / base["evals"])[:, ~diff].max())
    cond_moves = (np.abs(base["u"] - coal_only["u"]) / scale).max(axis=1)
    print(f"{kind} n={n}: attempts {attempts.min()} .. {attempts.max()}; {int(diff.sum())} of {n} parcels change (accepted, rejected) "
          f"under last-bit noise; the others move by {moved:.1e} x evaluations; condensation moves the planes by {cond_moves}")
    assert np.all(base["status"] == DONE) and np.all(pert["status"] == DONE)
    assert attempts.min() == 1 and attempts.max() >= 5
    assert diff.sum() <= 0.05 * n, diff.sum()
    assert moved < TOL_EVAL, moved
    assert (cond_moves > 1e-4).sum() >= 5, cond_moves
