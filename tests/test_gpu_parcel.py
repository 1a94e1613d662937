"""GPU tests of the adiabatic parcel (cloudy_parcel_ssprk33_steps, cloudy_parcel_rhs; csrc/parcel.hpp).

The stepping reference is OrdinaryDiffEq's SSPRK33 formulas (gpu_support._ssprk33_host) over the NumPy right-hand side
of test_parcel_host (parcel_rhs_numpy) with the moments' tendency from the unchanged oracle,
    dmom = oracle.rhs_condensation_batch(op, 1.0, xi(T) (S - 1) (1000 / rho_l)^(1/3), mom)
(the tendency is linear in xi s), plus oracle.rhs_coal_batch(op, mom) for coal = True.

Run with `-m gpu`.  Seeds, steps and the coalescence rate were picked on this reference alone, which needs no device
(`reference`, `random_batch`): seed 5 keeps 300 of 300 parcels finite over the two steps, none is excluded; with the Golovin
rate of test 5 the reference's end state with coalescence differs from the one without by 1.3e-2 of |y0| + |y| in the number
planes."""
import ctypes as C

import numpy as np
import pytest

import bench
from gpu_support import INF, SENTINEL, _ssprk33_host, blank, dev, driver_case, make_case, mass_rows
from test_parcel_host import DEFAULTS, M0_DROP, N0, driver_initial_state, mean_radius_um, p_vs, parcel_rhs_numpy, rogers_deviation

pytestmark = pytest.mark.gpu

NORMS = (1e8, 1e-12)
TOL = 1e-10   # per plane, of |y0| + |want| (S: of the trajectory's max |S - 1|): the condensation right-hand side is asserted at
#               1e-11 per evaluation elsewhere in this suite, the system relaxes rather than amplifies, and 120 evaluations at the
#               measured ~1e-14 stay below 1e-11 -- 1e-10 leaves one order


def reference(oracle, op, c, y0, w, dt, n_steps, rows, coal=False):
    """-> (end state, max |S - 1| along the trajectory per parcel, the series of states after each step)"""
    scale = (1000.0 / c["rho_l"]) ** (1 / 3)
    cond = lambda mom, xi, s: oracle.rhs_condensation_batch(op, 1.0, xi * s * scale, np.ascontiguousarray(mom))   # noqa: E731
    coal_f = (lambda mom: oracle.rhs_coal_batch(op, np.ascontiguousarray(mom))) if coal else None
    rhs = lambda Y: parcel_rhs_numpy(c, Y, w, rows, cond, coal_f)   # noqa: E731
    y, smax, series = y0.copy(), np.abs(y0[0] - 1), [y0.copy()]
    with np.errstate(all="ignore"):
        for _ in range(n_steps):
            y = _ssprk33_host(rhs, y, dt, 1)
            smax = np.maximum(smax, np.abs(y[0] - 1))
            series.append(y)
    return y, smax, np.array(series)


def plane_err(got, want, y0, smax):
    """per plane and parcel: |got - want| / (|y0| + |want|); the S plane as S - 1 against the trajectory's max |S - 1|"""
    err = np.abs(got - want) / np.maximum(np.abs(y0) + np.abs(want), 1e-300)
    err[0] = np.abs(got[0] - want[0]) / smax
    return err


def steps(cloudy, plan, y_in, y_out, n, ld, sources, w, dt, n_steps, params=None):
    """the C entry point itself: w a float or a DeviceArray"""
    w_ptr, w_val = (w.ptr, 0.0) if isinstance(w, cloudy.DeviceArray) else (None, float(w))
    c = (params or cloudy.ParcelParams()).to_c()
    return cloudy.lib().cloudy_parcel_ssprk33_steps(plan.handle, n, ld, y_in.ptr, y_out.ptr, sources, w_ptr, w_val, C.byref(c), dt,
                                                    n_steps, None)


@pytest.fixture(scope="module")
def driver_runs(gpu_cloudy, oracle):
    """the driver's three cases, 64 identical parcels, 40 steps of 0.5 s, w = 10: reference and fused device result, once"""
    cloudy = gpu_cloudy
    runs = {}
    for name in ("monodisperse", "gamma", "mixture"):
        dist_types, mom = driver_case(name)
        rows = mass_rows(dist_types)
        par, op, _ = make_case(cloudy, oracle, dist_types, [[1.0]], (INF,) * len(dist_types), NORMS)
        y1 = np.array(driver_initial_state(DEFAULTS, sum(mom[r] for r in rows)) + mom)
        y0 = np.tile(y1[:, None], (1, 64))
        want, smax, series = reference(oracle, op, DEFAULTS, y0, 10.0, 0.5, 40, rows)
        y = dev(cloudy, y0)
        assert cloudy.solve_parcel_ssprk33(par, y, 10.0, 0.5, 40) is y
        runs[name] = dict(par=par, op=op, rows=rows, y0=y0, want=want, smax=smax, series=series, got=y.to_numpy(), dist_types=dist_types)
    return runs


@pytest.mark.parametrize("name", ["monodisperse", "gamma", "mixture"])
def test_driver_cases_in_one_launch(gpu_cloudy, driver_runs, name):
    """parcel_example.jl's three initial conditions, norms (1e8, 1e-12), sources = COND: the 64 columns bit-equal, the result
    within TOL of the reference stepping, the number planes unchanged; the monodisperse case also within the Rogers bounds of
    test_restatement_against_rogers_1975 on the device's own series (40 calls of one step)."""
    cloudy = gpu_cloudy
    r = driver_runs[name]
    got, want, y0 = r["got"], r["want"], r["y0"]
    assert np.array_equal(got.view(np.uint64), np.tile(got[:, :1], (1, 64)).view(np.uint64))
    err = plane_err(got, want, y0, r["smax"])
    print(f"{name}: max err vs the reference stepping {err.max():.2e} (per plane {np.array2string(err.max(axis=1), precision=1)})")
    assert err.max() <= TOL, err.max(axis=1)
    number = [4 + m - 1 for m in r["rows"]]
    assert np.allclose(got[number], y0[number], rtol=1e-15, atol=0)
    assert abs(want[0, 0] - 1) > 5e-3 and want[5, 0] > 1.5 * y0[5, 0]   # (the parcel did something: S - 1 ~ 0.9 %, the mass grew)
    if name == "monodisperse":
        y = dev(cloudy, y0)
        series = [y0[:, 0]]
        for _ in range(40):
            cloudy.solve_parcel_ssprk33(r["par"], y, 10.0, 0.5, 1)
            series.append(y.to_numpy()[:, 0])
        s = np.array(series)
        d_ss, d_r = rogers_deviation(0.5 * np.arange(41), (s[:, 0] - 1) * 100, mean_radius_um(DEFAULTS, s[:, 4], s[:, 5]))
        print(f"device series vs Rogers 1975: supersaturation {d_ss:.4f} percentage points, radius {d_r:.4f} um")
        assert d_ss <= 0.12 and d_r <= 0.05, (d_ss, d_r)


@pytest.mark.parametrize("name", ["monodisperse", "gamma", "mixture"])
def test_staged_device_right_hand_side(gpu_cloudy, driver_runs, name):
    """the same 40 steps with cloudy_parcel_rhs called stage by stage agree with the fused call to 1e-13 (the bound
    test_condensation_drivers_in_one_launch uses for that comparison)"""
    cloudy = gpu_cloudy
    r = driver_runs[name]

    def device_rhs(x):
        dy = cloudy.DeviceArray.zeros(*x.shape)
        assert cloudy.parcel_rhs(r["par"], dy, dev(cloudy, x), 10.0) is dy
        return dy.to_numpy()

    staged = _ssprk33_host(device_rhs, r["y0"], 0.5, 40)
    print(f"{name}: max rel err vs the staged device right-hand side {np.abs(r['got'] / staged - 1).max():.2e}")
    assert np.allclose(r["got"], staged, rtol=1e-13, atol=0)


BATCH_TYPES = [0, 1, 2, 3]   # Exponential, Gamma, Monodisperse, Lognormal


def random_batch(n, seed):
    """-> (y0 (4 + 10, n), w (n,)): the driver's distributions, a quarter of its number each, with N and m0 scaled per mode and
    parcel by factors in [0.5, 2]; T, p, S and w as the test says; q_v = 0.622 S p_vs(T) / p"""
    rng = np.random.default_rng(seed)
    T, p, S = rng.uniform(265, 300, n), rng.uniform(5e4, 1e5, n), rng.uniform(0.98, 1.02, n)
    w = rng.uniform(-2, 10, n)
    rows = [S, p, T, 0.622 * S * p_vs(DEFAULTS, T) / p]
    for t in BATCH_TYPES:
        nn, m = N0 / 4 * rng.uniform(0.5, 2, n), M0_DROP * rng.uniform(0.5, 2, n)
        rows += [nn, nn * m]
        if t == 1:      # Gamma, k = 2
            rows.append(nn * (m / 2) ** 2 * 6)
        elif t == 3:    # Lognormal, sigma = 0.5
            rows.append(nn * m * m * np.exp(0.25))
    return np.ascontiguousarray(np.stack(rows)), w


@pytest.fixture(scope="module")
def batch_run(gpu_cloudy, oracle):
    """300 parcels in buffers of leading dimension 320, 2 steps of 0.1 s out of place, per-parcel w: computed once"""
    cloudy = gpu_cloudy
    n, ld, dt, n_steps = 300, 320, 0.1, 2
    par, op, _ = make_case(cloudy, oracle, BATCH_TYPES, [[1.0]], (INF,) * 4, NORMS)
    plan = par.coal_data.plan(BATCH_TYPES)
    y0, w = random_batch(n, seed=5)
    want, smax, _ = reference(oracle, op, DEFAULTS, y0, w, dt, n_steps, mass_rows(BATCH_TYPES))
    buf = np.full((y0.shape[0], ld), 7.0)
    buf[:, :n] = y0
    w_dev = dev(cloudy, w[None, :])
    y_in = dev(cloudy, buf)
    y_out = dev(cloudy, blank(*buf.shape))
    cloudy._lib.check(steps(cloudy, plan, y_in, y_out, n, ld, cloudy.SRC_COND, w_dev, dt, n_steps))
    return dict(plan=plan, par=par, n=n, ld=ld, dt=dt, n_steps=n_steps, y0=y0, w=w, want=want, smax=smax, buf=buf, y_in=y_in,
                w_dev=w_dev, got=y_out.to_numpy())


def test_random_batch_four_closure_families(gpu_cloudy, batch_run):
    """padding and input untouched, n_steps = 0 the identity, in place = out of place, scalar w = constant w_dev, and every
    parcel (downdraughts with S < 1 -- evaporation -- included) within TOL of the reference stepping"""
    cloudy = gpu_cloudy
    b = batch_run
    n, ld, plan, got, y0 = b["n"], b["ld"], b["plan"], b["got"], b["y0"]
    assert np.isfinite(b["want"]).all(), "the reference alone must keep every parcel finite"
    assert (b["w"] < 0).sum() > 20 and (y0[0] < 1).sum() > 100 and (b["want"][5] < y0[5]).sum() > 50   # (evaporating parcels)
    assert np.all(got[:, n:].view(np.uint64) == SENTINEL), "the padding columns were written"
    assert np.array_equal(b["y_in"].to_numpy(), b["buf"]), "the input changed"
    err = plane_err(got[:, :n], b["want"], y0, b["smax"])
    print(f"random batch: max err vs the reference stepping {err.max():.2e} (per plane {np.array2string(err.max(axis=1), precision=1)})")
    assert err.max() <= TOL, err.max(axis=1)
    fresh = lambda: dev(cloudy, blank(*b["buf"].shape))   # noqa: E731
    z = fresh()
    cloudy._lib.check(steps(cloudy, plan, b["y_in"], z, n, ld, cloudy.SRC_COND, b["w_dev"], b["dt"], 0))
    z = z.to_numpy()
    assert np.array_equal(z[:, :n], y0) and np.all(z[:, n:].view(np.uint64) == SENTINEL)
    inplace = dev(cloudy, b["buf"])
    cloudy._lib.check(steps(cloudy, plan, inplace, inplace, n, ld, cloudy.SRC_COND, b["w_dev"], b["dt"], b["n_steps"]))
    ip = inplace.to_numpy()
    assert np.array_equal(ip[:, :n].view(np.uint64), got[:, :n].view(np.uint64)) and np.array_equal(ip[:, n:], b["buf"][:, n:])
    a, c = fresh(), fresh()
    cloudy._lib.check(steps(cloudy, plan, b["y_in"], a, n, ld, cloudy.SRC_COND, 3.25, b["dt"], b["n_steps"]))
    cloudy._lib.check(steps(cloudy, plan, b["y_in"], c, n, ld, cloudy.SRC_COND, dev(cloudy, np.full((1, n), 3.25)), b["dt"], b["n_steps"]))
    assert np.array_equal(a.to_numpy().view(np.uint64), c.to_numpy().view(np.uint64))
    assert not np.array_equal(a.to_numpy()[:, :n], got[:, :n])


@pytest.mark.parametrize("n", [1, 65, 257])
def test_small_shapes_same_bits_as_inside_the_batch(gpu_cloudy, batch_run, n):
    """a single parcel with ld = 1 (as every reference driver), a partial wave, a partial workgroup"""
    cloudy = gpu_cloudy
    b = batch_run
    y = dev(cloudy, np.ascontiguousarray(b["y0"][:, :n]))
    out = cloudy.solve_parcel_ssprk33(b["par"], y, dev(cloudy, np.ascontiguousarray(b["w"][None, :n])), b["dt"], b["n_steps"],
                                      out=cloudy.DeviceArray.zeros(b["y0"].shape[0], n))
    assert np.array_equal(out.to_numpy().view(np.uint64), b["got"][:, :n].view(np.uint64))
    assert np.array_equal(y.to_numpy(), b["y0"][:, :n])


GOLOVIN = [[0.0, 50.0], [50.0, 0.0]]   # b (x + y), b = 50: 1e-2 / s of the number at the driver's N and m0


def two_gamma_state(n):
    N, m0 = N0, M0_DROP
    mom = [0.9 * N, 0.9 * N * m0, 0.9 * N * (m0 / 2) ** 2 * 6, 0.1 * N, 0.1 * N * 4 * m0, 0.1 * N * (2 * m0) ** 2 * 6]
    y1 = np.array(driver_initial_state(DEFAULTS, mom[1] + mom[4]) + mom)
    return np.tile(y1[:, None], (1, n))


def test_coalescence_and_condensation(gpu_cloudy, oracle):
    """two Gamma modes, order-1 tensor, thresholds Inf, 64 parcels, 2 steps: COAL | COND within TOL of the reference stepping,
    and different from COND alone.  A thresholded plan and a NumericalCoalStyle plan refuse COAL | COND and run COND."""
    cloudy = gpu_cloudy
    L, E = cloudy.lib(), cloudy._lib
    both = cloudy.SRC_COAL | cloudy.SRC_COND
    types, n, dt, n_steps = [1, 1], 64, 0.5, 2
    par, op, _ = make_case(cloudy, oracle, types, GOLOVIN, (INF, INF), NORMS)
    y0 = two_gamma_state(n)
    want, smax, _ = reference(oracle, op, DEFAULTS, y0, 10.0, dt, n_steps, mass_rows(types), coal=True)
    y = dev(cloudy, y0)
    cloudy.solve_parcel_ssprk33(par, y, 10.0, dt, n_steps, coal=True)
    got = y.to_numpy()
    err = plane_err(got, want, y0, smax)
    print(f"coalescence + condensation: max err vs the reference stepping {err.max():.2e}")
    assert err.max() <= TOL, err.max(axis=1)
    y = dev(cloudy, y0)
    cloudy.solve_parcel_ssprk33(par, y, 10.0, dt, n_steps)
    cond_only = y.to_numpy()
    shift = np.abs(got - cond_only) / (np.abs(y0) + np.abs(got))
    print(f"|with - without coalescence| / (|y0| + |y|): number planes {shift[[4, 7]].max():.2e}")
    assert shift[[4, 7]].min() > 1e-4
    dy_c, dy_b = cloudy.DeviceArray.zeros(*y0.shape), cloudy.DeviceArray.zeros(*y0.shape)
    cloudy.parcel_rhs(par, dy_c, dev(cloudy, y0), 10.0)
    cloudy.parcel_rhs(par, dy_b, dev(cloudy, y0), 10.0, coal=True)
    dc, db = dy_c.to_numpy(), dy_b.to_numpy()
    assert np.all(dc[[4, 7]] == 0) and np.all(db[4] < 0)
    assert np.allclose(dc[:4], db[:4], rtol=1e-13, atol=0)   # (only the condensation term enters the thermodynamic tendencies)
    # plans without the combined kernel: refused for COAL | COND, served for COND (one reference for both: nothing of the
    # coalescence data enters)
    par_b, op_b, _ = make_case(cloudy, oracle, types, GOLOVIN, (INF, INF), bench.NORMS)
    want_c, smax_c, _ = reference(oracle, op_b, DEFAULTS, y0, 10.0, dt, n_steps, mass_rows(types))
    par_t, _, _ = make_case(cloudy, oracle, types, GOLOVIN, (5e-9, INF), bench.NORMS)
    thresholded = par_t.coal_data.plan(types)
    numerical = cloudy.NumericalPlan(types, cloudy.LinearKernelFunction(5e-3), bench.NORMS, 10, quad_mode=cloudy.QUAD_FIXED)
    for plan, word in ((thresholded, b"thresholds"), (numerical, b"quadrature")):
        y = dev(cloudy, y0)
        assert steps(cloudy, plan, y, y, n, n, both, 10.0, dt, n_steps) == E.EUNSUPPORTED
        assert word in L.cloudy_last_error() and b"stage by stage" in L.cloudy_last_error()
        assert np.array_equal(y.to_numpy(), y0)
        assert steps(cloudy, plan, y, y, n, n, cloudy.SRC_COND, 10.0, dt, n_steps) == 0, L.cloudy_last_error()
        err = plane_err(y.to_numpy(), want_c, y0, smax_c)
        assert err.max() <= TOL, err.max(axis=1)


def test_refusals(gpu_cloudy, oracle):
    """status codes and a message, never an exception or a launch"""
    cloudy = gpu_cloudy
    L, E = cloudy.lib(), cloudy._lib
    types, n = [1, 1], 64
    par, _, _ = make_case(cloudy, oracle, types, GOLOVIN, (INF, INF), NORMS)
    y0 = two_gamma_state(n)
    y = dev(cloudy, y0)
    for dtype in (cloudy.F32, cloudy.F32_FAST):
        plan = par.coal_data.plan(types, dtype=dtype)
        for sources in (cloudy.SRC_COND, cloudy.SRC_COAL | cloudy.SRC_COND):
            assert steps(cloudy, plan, y, y, n, n, sources, 10.0, 0.5, 1) == E.EUNSUPPORTED
            assert b"float plane" in L.cloudy_last_error() and b"stage by stage" in L.cloudy_last_error()
    plan = par.coal_data.plan(types)
    assert steps(cloudy, plan, y, y, n, n, cloudy.SRC_COAL, 10.0, 0.5, 1) == E.EINVAL and b"CLOUDY_SRC_COND" in L.cloudy_last_error()
    assert steps(cloudy, plan, y, y, n, n - 1, cloudy.SRC_COND, 10.0, 0.5, 1) == E.EINVAL
    assert steps(cloudy, plan, y, y, n, n, cloudy.SRC_COND, 10.0, 0.5, -1) == E.EINVAL
    assert np.array_equal(y.to_numpy(), y0)
    # a CLOUDY_F64_RELAXED plan is served; an empty batch is fine; without plan-time compilation there is no kernel
    relaxed = par.coal_data.plan(types, dtype=cloudy.F64_RELAXED)
    assert steps(cloudy, relaxed, y, y, n, n, cloudy.SRC_COND, 10.0, 0.5, 1) == 0, L.cloudy_last_error()
    c = cloudy.ParcelParams().to_c()
    assert L.cloudy_parcel_ssprk33_steps(plan.handle, 0, 0, None, None, cloudy.SRC_COND, None, 10.0, C.byref(c), 0.5, 1, None) == 0
    aot = par.coal_data.plan(types, specialize=-1)
    y = dev(cloudy, y0)
    assert steps(cloudy, aot, y, y, n, n, cloudy.SRC_COND, 10.0, 0.5, 1) == E.EUNSUPPORTED and b"plan-time compilation" in L.cloudy_last_error()
    for bad in (dev(cloudy, np.zeros((1, n), dtype=np.float32)), dev(cloudy, np.zeros((1, n - 1))), dev(cloudy, np.zeros((2, n)))):
        with pytest.raises(ValueError):
            cloudy.solve_parcel_ssprk33(par, y, bad, 0.5, 1)
    assert np.array_equal(y.to_numpy(), y0)
