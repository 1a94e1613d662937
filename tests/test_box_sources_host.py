"""CPU-only checks of cloudy_box_ssprk33_steps (fused SSPRK33 stepping with the condensation source): the symbol in the header,
the ctypes table and the Julia shim with one arity, the CLOUDY_SRC_* constants mirrored, the Python wrapper exported, and the
plan-time unit that holds its kernels compiling for gfx950 without a device."""
import ctypes as C
import inspect
import os
import re

import pytest

import bench
from test_host_abi import INF, ROOT, _c_prototypes, _julia_ccalls

NAME = "cloudy_box_ssprk33_steps"


def test_symbol_in_header_ctypes_table_and_julia_shim(cloudy):
    protos = _c_prototypes()
    assert NAME in protos
    ret, args = protos[NAME]
    assert ret == "int"
    assert args == ["ptr", "size_t", "size_t", "ptr", "ptr", "int", "ptr", "double", "double", "double", "int", "ptr"]
    res, argtypes = cloudy._lib.SYMBOLS[NAME]
    assert res is C.c_int and len(argtypes) == len(args)
    ctype_of = {"ptr": (C.c_void_p,), "size_t": (C.c_size_t,), "int": (C.c_int,), "double": (C.c_double,)}
    for a, c in zip(argtypes, args):
        assert a in ctype_of[c], (a, c)
    assert hasattr(cloudy.lib(), NAME)
    src = open(os.path.join(ROOT, "julia", "CloudyHIP.jl")).read()
    calls = [c for c in _julia_ccalls(src) if c[0] == NAME]
    assert len(calls) == 1 and calls[0][1] == "Cint" and len(calls[0][2]) == len(args)
    assert re.search(r"function solve_box_ssprk33!\(u, plan::Plan, dt, n_steps, xi, s; coal::Bool = true, cond::Bool = true", src)


def test_source_constants_are_mirrored(cloudy):
    text = open(os.path.join(ROOT, "include", "cloudy_hip.h")).read()
    c = {k: int(v) for k, v in re.findall(r"#define (CLOUDY_SRC_\w+) (\d+)", text)}
    assert c == {"CLOUDY_SRC_COAL": 1, "CLOUDY_SRC_COND": 2}
    assert (cloudy.SRC_COAL, cloudy.SRC_COND) == (c["CLOUDY_SRC_COAL"], c["CLOUDY_SRC_COND"])
    assert (cloudy._lib.SRC_COAL, cloudy._lib.SRC_COND) == (1, 2)
    src = open(os.path.join(ROOT, "julia", "CloudyHIP.jl")).read()
    assert re.search(r"const SRC_COAL, SRC_COND = 1, 2\b", src)


def test_python_wrapper_signature(cloudy):
    assert "solve_box_ssprk33" in cloudy.__all__
    params = list(inspect.signature(cloudy.solve_box_ssprk33).parameters)
    assert params == ["par", "u", "dt", "n_steps", "xi", "s", "coal", "cond", "out", "stream", "coal_type"]
    with pytest.raises(ValueError, match="Invalid coal style"):
        cloudy.solve_box_ssprk33(None, None, 1.0, 1, 1e-8, 0.05, coal_type="analytical")


def test_entry_point_checks_its_plan_before_any_device(cloudy):
    L, E = cloudy.lib(), cloudy._lib
    assert L.cloudy_box_ssprk33_steps(None, 4, 4, None, None, 3, None, 0.05, 1e-8, 1.0, 1, None) == E.EINVAL
    assert L.cloudy_last_error() == b"plan is NULL"


@pytest.mark.parametrize("case", ["cfg3a", "cfg3b", "cfg3a_f32", "cfg3_moving", "n5_beyond_aot", "numerical"])
def test_box_unit_compiles_without_a_gpu(cloudy, case, tmp_path, monkeypatch):
    """cloudy_jit_selfcheck compiles every unit the runtime could request for a plan, the box-sources unit among them: kept
    through CLOUDY_HIP_JIT_DUMP, its text defines both kernels (a NumericalCoalStyle plan: condensation alone) and its code
    object exists."""
    import numpy as np

    monkeypatch.setenv("CLOUDY_HIP_JIT_DUMP", str(tmp_path))
    L = cloudy.lib()
    if case == "numerical":
        d = cloudy.NumericalPlan.make_desc([1, 1], cloudy.LinearKernelFunction(5e-3), bench.NORMS, 10, quad_mode=cloudy.QUAD_FIXED)
        keep = None
    elif case == "n5_beyond_aot":
        d, keep = cloudy.Plan.make_desc([1] * 5, np.array([[0.0, 5.0], [5.0, 0.0]]), (INF,) * 5, bench.NORMS, 0)
    else:
        spec = bench.workload_spec("cfg3b" if case == "cfg3_moving" else case[:5])
        moving, thr = (1, (0.9, 1.0)) if case == "cfg3_moving" else (0, spec["thresholds"])
        d, keep = cloudy.Plan.make_desc([1] * spec["n_modes"], bench.kernel_matrix(spec), thr, bench.NORMS, moving,
                                        dtype=1 if case.endswith("f32") else 0)
    assert L.cloudy_jit_selfcheck(C.byref(d), b"gfx950") == 0, L.cloudy_last_error().decode()
    units = [f for f in sorted(os.listdir(tmp_path)) if f.endswith(".hip") and "box_sources.hpp" in open(tmp_path / f).read()]
    assert len(units) == 1, units
    text = open(tmp_path / units[0]).read()
    assert " cloudy_jit_box_cond_" in text and "cloudy::SRC_COND>" in text
    assert (" cloudy_jit_box_coalcond_" in text) == (case != "numerical")
    if case == "cfg3a_f32":
        assert "const float *u_in" in text
    assert os.path.getsize(tmp_path / units[0].replace(".hip", ".co")) > 1000
