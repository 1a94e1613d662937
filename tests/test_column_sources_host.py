"""CPU-only checks of the column entry points with the condensation source (cloudy_rainshaft_cond_ssprk33_steps,
cloudy_rainshaft_cond_rhs): the symbols in the header, the ctypes table and the Julia shim with one arity, the Python wrappers
exported, and the plan-time units that hold their kernels compiling for gfx950 without a device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import bench
from test_host_abi import INF, ROOT, _c_prototypes, _julia_ccalls

EPS = np.finfo(np.float64).eps
GOLOVIN = np.array([[EPS / 1e6, 5.0], [5.0, 0.0]])   # the kernel of the rainshaft drivers (rainshaft_gamma_mixture.jl)
VEL = ((50.0, 1.0 / 6),)
ARGS = {
    "cloudy_rainshaft_cond_ssprk33_steps": ["ptr", "size_t", "size_t", "size_t", "ptr", "ptr", "ptr", "double", "double", "double",
                                            "double", "int", "ptr"],
    "cloudy_rainshaft_cond_rhs": ["ptr", "size_t", "size_t", "size_t", "ptr", "ptr", "double", "double", "double", "ptr", "ptr", "ptr"],
}


@pytest.mark.parametrize("name", sorted(ARGS))
def test_symbol_in_header_ctypes_table_and_julia_shim(cloudy, name):
    protos = _c_prototypes()
    assert name in protos
    ret, args = protos[name]
    assert ret == "int" and args == ARGS[name]
    res, argtypes = cloudy._lib.SYMBOLS[name]
    assert res is C.c_int and len(argtypes) == len(args)
    ctype_of = {"ptr": (C.c_void_p,), "size_t": (C.c_size_t,), "int": (C.c_int,), "double": (C.c_double,)}
    for a, c in zip(argtypes, args):
        assert a in ctype_of[c], (a, c)
    assert hasattr(cloudy.lib(), name)
    src = open(os.path.join(ROOT, "julia", "CloudyHIP.jl")).read()
    calls = [c for c in _julia_ccalls(src) if c[0] == name]
    assert len(calls) == 1 and calls[0][1] == "Cint" and len(calls[0][2]) == len(args)


def test_julia_wrappers_are_defined():
    src = open(os.path.join(ROOT, "julia", "CloudyHIP.jl")).read()
    assert re.search(r"function solve_rainshaft_cond_ssprk33!\(u, plan::Plan, nz, dz, dt, n_steps, xi, s; stream = nothing", src)
    assert re.search(r"function rainshaft_cond_rhs!\(dm, flux, m, plan::Plan, nz, dz, xi, s; stream = nothing", src)


def test_python_wrapper_signatures(cloudy):
    assert "solve_rainshaft_cond_ssprk33" in cloudy.__all__ and "make_rainshaft_cond_rhs" in cloudy.__all__
    params = list(inspect.signature(cloudy.solve_rainshaft_cond_ssprk33).parameters)
    assert params == ["par", "u", "n_steps", "xi", "s", "out", "stream"]
    rhs = cloudy.make_rainshaft_cond_rhs()
    assert list(inspect.signature(rhs).parameters) == ["m", "p", "t", "xi", "s", "out", "work"]


def test_entry_points_check_their_plan_before_any_device(cloudy):
    L, E = cloudy.lib(), cloudy._lib
    assert L.cloudy_rainshaft_cond_ssprk33_steps(None, 20, 2, 40, None, None, None, 0.05, 1e-8, 150.0, 1.0, 1, None) == E.EINVAL
    assert L.cloudy_last_error() == b"plan is NULL"
    assert L.cloudy_rainshaft_cond_rhs(None, 20, 2, 40, None, None, 0.05, 1e-8, 150.0, None, None, None) == E.EINVAL
    assert L.cloudy_last_error() == b"plan is NULL"


def _cond_units(tmp_path):
    return [f for f in sorted(os.listdir(tmp_path))
            if f.endswith(".hip") and " cloudy_jit_rainshaft_cond_" in open(tmp_path / f).read()]


@pytest.mark.parametrize("case", ["gamma_mixture", "single_gamma", "gamma_mixture_f32"])
def test_column_condensation_units_compile_without_a_gpu(cloudy, case, tmp_path, monkeypatch):
    """cloudy_jit_selfcheck compiles every unit the runtime could request for a plan: for the reference's two column plans (the
    thresholded two-mode plan, the all-Inf one-mode plan; one velocity term) that includes one unit per workgroup size with the
    column integrator and the column RHS with the condensation source.  Kept through CLOUDY_HIP_JIT_DUMP, their text defines
    both kernels as the COND instances of the column body, and their code objects exist."""
    monkeypatch.setenv("CLOUDY_HIP_JIT_DUMP", str(tmp_path))
    L = cloudy.lib()
    nm = 1 if case == "single_gamma" else 2
    d, keep = cloudy.Plan.make_desc([1] * nm, GOLOVIN, (2e-10, INF)[2 - nm:], bench.NORMS, 0, vel=VEL,
                                    dtype=1 if case.endswith("f32") else 0)
    assert L.cloudy_jit_selfcheck(C.byref(d), b"gfx950") == 0, L.cloudy_last_error().decode()
    units = _cond_units(tmp_path)
    assert len(units) == 3, units
    mode = "MODE_ALLINF" if nm == 1 else "MODE_FIXED"
    tails = set()
    for u in units:
        text = open(tmp_path / u).read()
        m = re.search(r" cloudy_jit_rainshaft_cond_ssprk33_n%dp2_(f64|f32)(_b512|_b1024|)\(" % nm, text)
        assert m, u
        tails.add(m.group(2))
        assert " cloudy_jit_rainshaft_cond_rhs_n%dp2_%s%s(" % (nm, m.group(1), m.group(2)) in text
        bs = m.group(2)[2:] or "256"
        assert f"__launch_bounds__({bs})" in text
        assert re.search(r"rainshaft_ssprk33_body<%d, 2, cloudy::%s, \w+, true, %s, false, true>" % (nm, mode, bs), text)
        assert re.search(r"rainshaft_ssprk33_body<%d, 2, cloudy::%s, \w+, true, %s, true, true>" % (nm, mode, bs), text)
        assert "const double *__restrict__ s_dev" in text and " cloudy_jit_rainshaft_ssprk33_" not in text
        if case.endswith("f32"):
            assert "const float *u_in" in text
        assert os.path.getsize(tmp_path / u.replace(".hip", ".co")) > 1000
    assert tails == {"", "_b512", "_b1024"}


def test_a_numerical_coal_style_plan_has_no_such_unit(cloudy, tmp_path, monkeypatch):
    """A NumericalCoalStyle description has no column body: none of its units defines a column kernel with the condensation
    source (the entry points refuse such plans)."""
    monkeypatch.setenv("CLOUDY_HIP_JIT_DUMP", str(tmp_path))
    L = cloudy.lib()
    d = cloudy.NumericalPlan.make_desc([1, 1], cloudy.LinearKernelFunction(5e-3), bench.NORMS, 10, quad_mode=cloudy.QUAD_FIXED)
    assert L.cloudy_jit_selfcheck(C.byref(d), b"gfx950") == 0, L.cloudy_last_error().decode()
    assert any(f.endswith(".hip") for f in os.listdir(tmp_path))
    assert _cond_units(tmp_path) == []
