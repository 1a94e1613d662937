"""CPU-only checks of the adiabatic parcel (cloudy_parcel_rhs, cloudy_parcel_ssprk33_steps, cloudy_parcel_thermo_host;
csrc/parcel.hpp): the ABI in the header, the ctypes table and the Julia shim; the argument checks; the closure helper against a
NumPy restatement of the equations (written here: `thermo`, `parcel_rhs_numpy`); the plan-time unit compiling for gfx950
without a device; and the restatement alone against Rogers's 1975 points that the reference driver plots
(test/examples/Analytical/parcel_example.jl:189-192, tests/golden/rogers_1975.json).

tests/test_gpu_parcel.py steps the same restatement with the oracle's condensation tendency as the device's reference."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest

import bench
from test_host_abi import INF, ROOT, _c_prototypes, _julia_ccalls

NAMES = ("cloudy_parcel_rhs", "cloudy_parcel_ssprk33_steps", "cloudy_parcel_thermo_host")
FIELDS = ("R_d", "R_v", "cp_d", "cp_v", "cp_l", "LH_v0", "T_0", "press_triple", "T_triple", "grav", "K_therm", "D_vapor", "rho_l")
_R = 8.3144598
DEFAULTS = dict(R_d=_R / 0.02897, R_v=_R / 0.018015, cp_d=_R / 0.02897 * 7 / 2, cp_v=1859.0, cp_l=4181.0, LH_v0=2.5008e6, T_0=273.16,
                press_triple=611.657, T_triple=273.16, grav=9.81, K_therm=2.4e-2, D_vapor=2.26e-5, rho_l=1000.0)


# ---- the NumPy restatement of the issue's equations (vectorised over parcels)
def p_vs(c, T):
    dcp = c["cp_v"] - c["cp_l"]
    return c["press_triple"] * (T / c["T_triple"]) ** (dcp / c["R_v"]) * np.exp(
        (c["LH_v0"] - dcp * c["T_0"]) / c["R_v"] * (1 / c["T_triple"] - 1 / T))


def thermo(c, S, p, T, q_v, m_liq):
    """(rho, R, cp, L, p_vs, xi, a1, a3)"""
    R_m = lambda q_t, q_l: c["R_d"] * (1 + (c["R_v"] / c["R_d"] - 1) * q_t - (c["R_v"] / c["R_d"]) * q_l)  # noqa: E731
    cp_m = lambda q_t, q_l: c["cp_d"] + (c["cp_v"] - c["cp_d"]) * q_t + (c["cp_l"] - c["cp_v"]) * q_l      # noqa: E731
    rho0 = p / (R_m(q_v, 0.0) * T)
    q_l = m_liq / rho0
    R, cp = R_m(q_v + q_l, q_l), cp_m(q_v + q_l, q_l)
    rho = p / (R * T)
    L = c["LH_v0"] + (c["cp_v"] - c["cp_l"]) * (T - c["T_0"])
    pv = p_vs(c, T)
    xi = 1 / (L / (c["K_therm"] * T) * (L / (c["R_v"] * T) - 1) + c["R_v"] * T / (c["D_vapor"] * pv))
    g = c["grav"]
    a1 = L * g / (cp * T**2 * c["R_v"]) - g / (R * T)
    a3 = L**2 / (c["R_v"] * T**2 * cp)
    return rho, R, cp, L, pv, xi, a1, a3


def parcel_rhs_numpy(c, Y, w, mass_rows, cond_tendency, coal_tendency=None):
    """dY of Y = (S, p, T, q_v, mom...) with shape (4 + nmom, n).  cond_tendency(mom, xi, s) -> dmom of get_cond_evap (physical
    units, xi and s per parcel); mass_rows: the rows of `mom` that hold the modes' mass moments."""
    S, p, T, q_v, mom = Y[0], Y[1], Y[2], Y[3], Y[4:]
    rho, R, cp, L, _, xi, a1, a3 = thermo(c, S, p, T, q_v, mom[mass_rows].sum(axis=0))
    dmom = cond_tendency(mom, xi, S - 1)
    dq_l = dmom[mass_rows].sum(axis=0) / rho
    dY = np.empty_like(Y)
    dY[0] = a1 * w * S - (1 / q_v + a3) * S * dq_l
    dY[1] = -p * c["grav"] * w / (R * T)
    dY[2] = -c["grav"] * w / cp + L * dq_l / cp
    dY[3] = -dq_l
    dY[4:] = dmom if coal_tendency is None else dmom + coal_tendency(mom)
    return dY


def ssprk33(rhs, u0, dt, n_steps, keep=False):
    """OrdinaryDiffEq's SSPRK33 update formulas; keep: the whole series"""
    u, series = u0.copy(), [u0.copy()]
    for _ in range(n_steps):
        up = u
        u = up + dt * rhs(up)
        u = (3 * up + u + dt * rhs(u)) / 4
        u = (up + 2 * u + 2 * dt * rhs(u)) / 3
        series.append(u)
    return np.array(series) if keep else u


def monodisperse_cond(c):
    """get_cond_evap of one Monodisperse mode (n, theta) = (M0, M1 / M0): d M1/dt = 3 xi s (4 pi/3)^(2/3) / rho_l^(1/3) M_{1/3}"""
    def f(mom, xi, s):
        with np.errstate(all="ignore"):
            m13 = mom[0] * np.cbrt(mom[1] / mom[0])
        return np.stack([np.zeros_like(m13), 3 * xi * s * (4 * np.pi / 3) ** (2 / 3) / np.cbrt(c["rho_l"]) * m13])
    return f


def driver_initial_state(c, M1_total, T0=280.15, p0=8e4, S0=1.0):
    """parcel_example.jl:174-179, 218: (S, p, T, q_v)"""
    e = p_vs(c, T0)
    m_d, m_v = (p0 - e) / c["R_d"] / T0, e / c["R_v"] / T0
    return [S0, p0, T0, m_v / (m_d + m_v + M1_total)]


N0, R0 = 2e8, 8e-6
M0_DROP = 4 / 3 * np.pi * R0**3 * 1000.0


def mean_radius_um(c, M0, M1):
    return np.cbrt(M1 / M0 / c["rho_l"] / 4 / np.pi * 3) * 1e6


def rogers():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "rogers_1975.json")))


def rogers_deviation(t, supersat_percent, radius_um):
    """max |series - Rogers's points|, the series interpolated on its step grid (np.interp)"""
    r = rogers()
    return (np.abs(np.interp(r["time_supersat"], t, supersat_percent) - r["supersat"]).max(),
            np.abs(np.interp(r["time_radius"], t, radius_um) - r["radius"]).max())


def monodisperse_series(dt, n_steps):
    c = DEFAULTS
    y0 = np.array(driver_initial_state(c, N0 * M0_DROP) + [N0, N0 * M0_DROP])[:, None]
    return ssprk33(lambda Y: parcel_rhs_numpy(c, Y, 10.0, [1], monodisperse_cond(c)), y0, dt, n_steps, keep=True)[:, :, 0]


# ---- 1. ABI
def test_symbols_in_header_ctypes_table_and_julia_shim(cloudy):
    protos = _c_prototypes()
    want = {
        "cloudy_parcel_params_init": ("void", ["ptr"]),
        "cloudy_parcel_rhs": ("int", ["ptr", "size_t", "size_t", "ptr", "ptr", "double", "ptr", "int", "ptr", "ptr"]),
        "cloudy_parcel_ssprk33_steps": ("int", ["ptr", "size_t", "size_t", "ptr", "ptr", "int", "ptr", "double", "ptr", "double", "int",
                                                "ptr"]),
    }
    for name, (ret, args) in want.items():
        assert protos[name] == (ret, args), name
    assert protos["cloudy_parcel_thermo_host"][0] == "int" and len(protos["cloudy_parcel_thermo_host"][1]) == 7
    src = open(os.path.join(ROOT, "julia", "CloudyHIP.jl")).read()
    calls = _julia_ccalls(src)
    for name in NAMES + ("cloudy_parcel_params_init",):
        res, argtypes = cloudy._lib.SYMBOLS[name]
        assert len(argtypes) == len(protos[name][1]), name
        assert hasattr(cloudy.lib(), name)
    for name in ("cloudy_parcel_params_init", "cloudy_parcel_rhs", "cloudy_parcel_ssprk33_steps"):
        mine = [c for c in calls if c[0] == name]
        assert len(mine) == 1 and len(mine[0][2]) == len(protos[name][1]), name
    assert re.search(r"function parcel_rhs!\(dy, y, plan::Plan, w; params::ParcelParams = ParcelParams\(\), coal::Bool = false", src)
    assert re.search(r"function solve_parcel_ssprk33!\(y, plan::Plan, w, dt, n_steps; params::ParcelParams = ParcelParams\(\), "
                     r"coal::Bool = false", src)
    body = re.search(r"mutable struct ParcelParams\n(.*?)\n    function", src, re.S).group(1)
    assert [l.strip() for l in body.splitlines()] == ["struct_size::UInt32"] + [f"{f}::Float64" for f in FIELDS]


def test_params_defaults_bit_equal_in_every_binding(cloudy):
    c = cloudy._lib.ParcelParamsC()
    cloudy.lib().cloudy_parcel_params_init(C.byref(c))
    assert c.struct_size == C.sizeof(cloudy._lib.ParcelParamsC) == 8 + 13 * 8
    mine = cloudy.ParcelParams().to_c()
    assert mine.struct_size == c.struct_size
    assert [f[0] for f in cloudy._lib.ParcelParamsC._fields_] == ["struct_size"] + list(FIELDS)
    for f in FIELDS:
        assert np.float64(getattr(mine, f)).view(np.uint64) == np.float64(getattr(c, f)).view(np.uint64), f
        assert getattr(c, f) == DEFAULTS[f], f
    assert cloudy.ParcelParams(rho_l=997.0).to_c().rho_l == 997.0


def test_python_wrappers_are_exported_with_their_signatures(cloudy):
    for n in ("ParcelParams", "parcel_rhs", "solve_parcel_ssprk33"):
        assert n in cloudy.__all__
    assert list(inspect.signature(cloudy.parcel_rhs).parameters) == ["par", "dy", "y", "w", "params", "coal", "stream"]
    assert list(inspect.signature(cloudy.solve_parcel_ssprk33).parameters) == ["par", "y", "w", "dt", "n_steps", "params", "coal", "out",
                                                                               "stream"]
    sig = inspect.signature(cloudy.solve_parcel_ssprk33).parameters
    assert sig["params"].default is None and sig["coal"].default is False and sig["out"].default is None


# ---- 2. argument checks, all before any device work (no plan exists here: it is the last thing looked at)
def test_argument_checks_answer_einval_with_a_message(cloudy):
    L, E = cloudy.lib(), cloudy._lib
    COAL, COND = cloudy.SRC_COAL, cloudy.SRC_COND
    ok = cloudy.ParcelParams().to_c()

    def steps(params=ok, sources=COND, n=4, ld=4, dt=0.5, n_steps=1):
        ref = None if params is None else C.byref(params)
        return L.cloudy_parcel_ssprk33_steps(None, n, ld, None, None, sources, None, 10.0, ref, dt, n_steps, None)

    def rhs(params=ok, sources=COND, n=4, ld=4):
        ref = None if params is None else C.byref(params)
        return L.cloudy_parcel_rhs(None, n, ld, None, None, 10.0, ref, sources, None, None)

    def msg():
        return L.cloudy_last_error().decode()

    for call in (steps, rhs):
        assert call() == E.EINVAL and msg() == "plan is NULL"
        assert call(params=None) == E.EINVAL and msg() == "params is NULL"
        short = cloudy.ParcelParams().to_c()
        short.struct_size -= 8
        assert call(params=short) == E.EINVAL and "struct_size" in msg()
        for field in FIELDS:
            for bad in (0.0, -1.0, float("nan")):
                p = cloudy.ParcelParams(**{field: bad}).to_c()
                assert call(params=p) == E.EINVAL and f"params.{field}" in msg() and "positive" in msg(), (field, bad)
        for sources in (COAL, 0, 4, -1):
            assert call(sources=sources) == E.EINVAL and "CLOUDY_SRC_COND" in msg(), sources
        assert call(n=4, ld=3) == E.EINVAL and "ld (3) must be >= n_parcels (4)" in msg()
        assert call(sources=COAL | COND) == E.EINVAL and msg() == "plan is NULL"
    assert steps(n_steps=-1) == E.EINVAL and "n_steps must be >= 0" in msg()
    assert steps(dt=float("nan")) == E.EINVAL and "dt not NaN" in msg()
    out = (C.c_double * 8)()
    assert L.cloudy_parcel_thermo_host(None, 1.0, 8e4, 280.0, 8e-3, 0.0, out) == E.EINVAL and msg() == "params is NULL"
    assert L.cloudy_parcel_thermo_host(C.byref(cloudy.ParcelParams(K_therm=0.0).to_c()), 1.0, 8e4, 280.0, 8e-3, 0.0, out) == E.EINVAL
    assert L.cloudy_parcel_thermo_host(C.byref(ok), 1.0, 8e4, 280.0, 8e-3, 0.0, None) == E.EINVAL and msg() == "out is NULL"


# ---- 3. / 4. the closure helper
def thermo_host(cloudy, params, S, p, T, q_v, m_liq):
    out = (C.c_double * 8)()
    c = params.to_c()
    assert cloudy.lib().cloudy_parcel_thermo_host(C.byref(c), S, p, T, q_v, m_liq, out) == 0
    return np.array(out[:])


def test_closure_helper_against_the_numpy_restatement(cloudy):
    """200 random states; every output to 1e-13 relative: the roundings of one log / exp pair and a dozen operations (the host
    path of the closure calls the library's log and exp; measured worst 6.7e-16)."""
    rng = np.random.default_rng(2024)
    c = DEFAULTS
    worst = 0.0
    for _ in range(200):
        T, p, S, m_liq = rng.uniform(250, 310), rng.uniform(3e4, 1.05e5), rng.uniform(0.9, 1.1), rng.uniform(0, 5e-3)
        q_v = 0.622 * S * p_vs(c, T) / p
        got = thermo_host(cloudy, cloudy.ParcelParams(), S, p, T, q_v, m_liq)
        want = np.array(thermo(c, S, p, T, q_v, m_liq))
        worst = max(worst, np.abs(got / want - 1).max())
    print(f"closure helper: worst relative difference {worst:.2e}")
    assert worst <= 1e-13, worst
    # other constants reach the helper too
    other = dict(DEFAULTS, rho_l=997.0, K_therm=2.5e-2, grav=9.80665, T_0=273.15)
    got = thermo_host(cloudy, cloudy.ParcelParams(**other), 1.01, 9e4, 285.0, 9e-3, 1e-3)
    assert np.allclose(got, thermo(other, 1.01, 9e4, 285.0, 9e-3, 1e-3), rtol=1e-13, atol=0)


def test_recorded_xi_and_saturation_pressure(cloudy):
    got = thermo_host(cloudy, cloudy.ParcelParams(), 1.0, 8e4, 280.15, 7.8e-3, 0.0)
    want = thermo(DEFAULTS, 1.0, 8e4, 280.15, 7.8e-3, 0.0)
    assert got[4] == pytest.approx(want[4], rel=1e-13) and got[5] == pytest.approx(want[5], rel=1e-13)
    # (the NumPy values, recorded)
    assert want[4] == pytest.approx(RECORDED_P_VS, rel=1e-12) and want[5] == pytest.approx(RECORDED_XI, rel=1e-12)


RECORDED_P_VS, RECORDED_XI = 1001.7608735363531, 8.037041635520475e-08   # p_vs(280.15) [Pa], xi(280.15) [m^2/s] of the default constants


# ---- 5. the plan-time unit
@pytest.mark.parametrize("case", ["gamma", "exp_gamma", "cfg3b", "numerical"])
def test_parcel_unit_compiles_without_a_gpu(cloudy, case, tmp_path, monkeypatch):
    """cloudy_jit_selfcheck compiles every unit the runtime could request for a plan, the parcel unit among them: exactly one
    dumped unit names parcel.hpp; it defines the integrator and the one-evaluation kernel, those with coalescence only for
    tensor plans whose thresholds are all Inf; its code object exists."""
    monkeypatch.setenv("CLOUDY_HIP_JIT_DUMP", str(tmp_path))
    L = cloudy.lib()
    norms = (1e8, 1e-12)
    if case == "numerical":
        d = cloudy.NumericalPlan.make_desc([1, 1], cloudy.LinearKernelFunction(5e-3), bench.NORMS, 10, quad_mode=cloudy.QUAD_FIXED)
        keep = None
    elif case == "cfg3b":
        spec = bench.workload_spec("cfg3b")
        d, keep = cloudy.Plan.make_desc([1] * spec["n_modes"], bench.kernel_matrix(spec), spec["thresholds"], bench.NORMS, 0)
    else:
        types = [1] if case == "gamma" else [0, 1]
        d, keep = cloudy.Plan.make_desc(types, np.array([[1.0]]), (INF,) * len(types), norms, 0)
    assert L.cloudy_jit_selfcheck(C.byref(d), b"gfx950") == 0, L.cloudy_last_error().decode()
    units = [f for f in sorted(os.listdir(tmp_path)) if f.endswith(".hip") and "parcel.hpp" in open(tmp_path / f).read()]
    assert len(units) == 1, units
    text = open(tmp_path / units[0]).read()
    assert "box_sources.hpp" not in text
    assert "cloudy_jit_rainshaft" not in text and "cloudy_jit_box" not in text
    assert " cloudy_jit_parcel_cond_" in text and " cloudy_jit_parcel_rhs_" in text
    assert (" cloudy_jit_parcel_coalcond_" in text) == (case in ("gamma", "exp_gamma"))
    assert os.path.getsize(tmp_path / units[0].replace(".hip", ".co")) > 1000


# ---- 6. the restatement alone
def test_restatement_against_rogers_1975():
    """The monodisperse case of the driver (N = 2e8, r0 = 8 um, T0 = 280.15, p0 = 8e4, S0 = 1, w = 10, dt = 0.5, 40 steps) with the
    distributions updated from the current moments: supersaturation within 0.12 percentage points of Rogers's points (measured
    0.078), mean radius within 0.05 um (measured 0.029); recorded values; dt/2 moves the end state by <= 1e-6."""
    c = DEFAULTS
    ys = monodisperse_series(0.5, 40)
    t = 0.5 * np.arange(41)
    ss, rad = (ys[:, 0] - 1) * 100, mean_radius_um(c, ys[:, 4], ys[:, 5])
    d_ss, d_r = rogers_deviation(t, ss, rad)
    print(f"restatement vs Rogers 1975: supersaturation {d_ss:.4f} percentage points, radius {d_r:.4f} um")
    assert d_ss <= 0.12 and d_r <= 0.05, (d_ss, d_r)
    k = int(np.argmax(ss))
    assert t[k] == 8.0 and ss[k] == pytest.approx(1.04973806, rel=1e-8)
    assert ys[40, 2] == pytest.approx(279.028977741, rel=1e-8)
    assert rad[40] == pytest.approx(9.65839662, rel=1e-8)
    fine = monodisperse_series(0.25, 80)
    moved = np.abs(fine[80] / ys[40] - 1)
    moved[0] = abs(fine[80, 0] - ys[40, 0]) / abs(ys[40, 0])
    print(f"dt / 2 moves the end state by {moved.max():.2e}")
    assert moved.max() <= 1e-6, moved
