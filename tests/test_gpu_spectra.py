"""cloudy_moments / cloudy_density on the device against the unchanged oracle (tests/test_spectra_host.py chooses the batches, the
orders, the cutoffs and the grid, and asserts what this file relies on): four plan families, n = 257 parcels in planes of leading
dimension 272, out of place, sentinel-filled outputs with one guard plane behind the last.

The bound of every comparison is 1e-12, the project's bound for one-evaluation diagnostics built from these device functions
(TOL_NQ, TOL_THR of tests/test_gpu_special_goldens.py): relative for the full moments and for the densities at or above 1e-30 of a
mode's peak on the grid (an exponent of magnitude below 750 carries a few eps per unit), of the full moment for the partial ones.
Measured on an MI355X (max over the batch):

    family                 full moments   partial / full   density    normed density
    exp_gamma              4.70e-15       6.99e-15         2.07e-14   2.07e-14
    gamma_lognormal_mono   1.57e-14       1.22e-14         7.84e-14   (Monodisperse: refused)
    eight_gamma            4.70e-15       8.28e-15         2.44e-14   2.41e-14
    numerical              4.70e-15       6.99e-15         2.07e-14   2.07e-14
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import bench
import test_spectra_host as H
from gpu_support import GOLOVIN, INF, bits_equal, blank, converged_case, dev, is_blank, make_case

pytestmark = pytest.mark.gpu

TOL = 1e-12
N, LD = H.N_PARCELS, H.LD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY_NAMES = list(H.FAMILIES)


@functools.lru_cache(maxsize=None)
def family_plan(cloudy, oracle, family, dtype=0, specialize=0, fresh=0):
    types = H.FAMILIES[family]
    if family == "numerical":
        par, _, _ = converged_case(cloudy, oracle, types, "linear")
        return cloudy.NumericalPlan(types, par.kernel_func, bench.NORMS, 8, dtype=dtype, specialize=specialize, quad_mode=cloudy.QUAD_CONVERGED)
    par, _, _ = make_case(cloudy, oracle, types, GOLOVIN, (INF,) * len(types), bench.NORMS)
    return par.coal_data.plan(types, dtype=dtype, specialize=specialize)


def launch(cloudy, call, mom, planes, n=None, expect=0):
    """call(n, ld, in_ptr, out_ptr) -> status, on the first n parcels of mom in sentinel-padded planes of leading dimension n + 15
    and a sentinel-filled output of planes + 1 planes: -> (planes, n) after the guard plane, the 15 tail columns and the input have
    been asserted untouched (a refused call: the whole output)"""
    n = mom.shape[1] if n is None else n
    ld = n + 15
    dtype = mom.dtype.type
    buf = blank(mom.shape[0], ld, dtype)
    buf[:, :n] = mom[:, :n]
    src, dst = dev(cloudy, buf), dev(cloudy, blank(planes + 1, ld, dtype))
    rc = call(n, ld, src.ptr, dst.ptr)
    msg = cloudy.lib().cloudy_last_error().decode()
    assert rc == expect, (rc, msg)
    cloudy._lib.check(cloudy.lib().cloudy_stream_synchronize(None))
    out = dst.to_numpy()
    assert bits_equal(src.to_numpy(), buf), "the input changed"
    if expect != 0:
        assert is_blank(out).all(), "a refused call wrote"
        return msg
    assert is_blank(out[planes]).all(), "the guard plane was written"
    assert is_blank(out[:, n:]).all(), "the tail columns were written"
    assert not is_blank(out[:planes, :n]).any(), "an output was left unwritten"
    return out[:planes, :n]


def moments(cloudy, plan, mom, orders, x_t=INF, per_mode=1, n=None, expect=0):
    arr = (C.c_double * len(orders))(*orders)
    planes = (plan.N if per_mode else 1) * len(orders)
    return launch(cloudy, lambda n_, ld, a, b: cloudy.lib().cloudy_moments(plan.handle, n_, ld, a, len(orders), arr, x_t, per_mode, b, None),
                  mom, planes, n, expect)


def density(cloudy, plan, mom, grid, kind=0, per_mode=1, n=None, expect=0):
    x = dev(cloudy, np.asarray(grid, dtype=np.float64).reshape(1, -1))
    planes = len(grid) * (plan.N if per_mode else 1)
    return launch(cloudy, lambda n_, ld, a, b: cloudy.lib().cloudy_density(plan.handle, n_, ld, a, kind, len(grid), x.ptr, per_mode, b, None),
                  mom, planes, n, expect)


# ---- moments
@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_moments_against_the_oracle(gpu_cloudy, oracle, family):
    cloudy = gpu_cloudy
    plan = family_plan(cloudy, oracle, family)
    types, mom = H.batch(family)
    Nm = len(types)
    worst_full = worst_part = 0.0
    for orders in (H.ORDERS, H.ONE_ORDER):
        ref = H.reference_moments(oracle, family, orders)
        got = moments(cloudy, plan, mom, orders).reshape(Nm, len(orders), N)
        assert np.array_equal(got == 0.0, ref == 0.0), "a fallback mode gives 0 at every order, nothing else does"
        live = ref > 0.0
        err = np.abs(got[live] - ref[live]) / ref[live]
        worst_full = max(worst_full, float(err.max()))
        print(f"{family}: {len(orders)} orders, full moments, max relative error {err.max():.2e}")
        assert (err <= TOL).all(), f"{err.max():.3e}"
        # +Inf: the bits of the full call, twice; per_mode = 0: the mode-order fp64 sum of the per-mode planes
        assert bits_equal(moments(cloudy, plan, mom, orders, x_t=INF).reshape(got.shape), got)
        total = moments(cloudy, plan, mom, orders, per_mode=0)
        s = np.zeros_like(got[0])
        for m in range(Nm):
            s = s + got[m]
        assert bits_equal(total, s)
        for x_t in H.CUTOFFS:
            pref = H.reference_moments(oracle, family, orders, x_t)
            pgot = moments(cloudy, plan, mom, orders, x_t=x_t).reshape(got.shape)
            assert np.isfinite(pgot).all() and (pgot >= 0).all()
            perr = np.abs(pgot[live] - pref[live]) / ref[live]
            assert (pgot[~live] == 0.0).all()
            worst_part = max(worst_part, float(perr.max()))
            assert (perr <= TOL).all(), f"x_t = {x_t}: {perr.max():.3e}"
            ptot = moments(cloudy, plan, mom, orders, x_t=x_t, per_mode=0)
            s = np.zeros_like(pgot[0])
            for m in range(Nm):
                s = s + pgot[m]
            assert bits_equal(ptot, s)
    print(f"{family}: full moments {worst_full:.2e}, partial moments / full {worst_part:.2e}")


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_orders_0_and_1_at_a_cutoff_are_the_liquid_part_of_standard_N_q(gpu_cloudy, oracle, family):
    cloudy = gpu_cloudy
    plan = family_plan(cloudy, oracle, family)
    _, mom = H.batch(family)
    for x_t in H.CUTOFFS:
        liq = moments(cloudy, plan, mom, (0.0, 1.0), x_t=x_t, per_mode=0)
        nq = launch(cloudy, lambda n, ld, a, b: cloudy.lib().cloudy_standard_N_q(plan.handle, n, ld, a, x_t, b, None), mom, 4)
        tot = np.stack([nq[0] + nq[1], nq[2] + nq[3]])
        err = np.abs(liq - nq[[0, 2]])
        assert (err <= TOL * tot).all(), float((err / np.maximum(tot, 1e-300)).max())


# ---- densities
def density_errors(got, ref):
    """got, ref (n_x, N, n) without x = 0 -> the largest relative error at or above the floor; asserts smallness below it"""
    peak = ref.max(axis=0, keepdims=True)
    above = ref >= H.FLOOR * peak
    assert (got[~above] <= 2.0 * H.FLOOR * np.broadcast_to(peak, ref.shape)[~above]).all() and (got[~above] >= 0.0).all()
    zero = above & (ref == 0.0)
    assert (got[zero] == 0.0).all()
    pos = above & (ref > 0.0)
    return float((np.abs(got[pos] - ref[pos]) / ref[pos]).max()) if pos.any() else 0.0


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_densities_against_the_oracle(gpu_cloudy, oracle, family, kind):
    cloudy = gpu_cloudy
    plan = family_plan(cloudy, oracle, family)
    types, mom = H.batch(family)
    if kind == 1 and 2 in types:
        msg = density(cloudy, plan, mom, H.GRID, kind=1, expect=cloudy._lib.EINVAL)
        assert "no method normed_density_func for a Monodisperse distribution" in msg
        return
    Nm = len(types)
    ref = H.reference_density(oracle, family, bool(kind))
    got = density(cloudy, plan, mom, H.GRID, kind=kind).reshape(len(H.GRID), Nm, N)
    worst = density_errors(got[1:], ref[1:])
    print(f"{family}: {'normed density' if kind else 'density'}, max relative error at or above the floor {worst:.2e}")
    assert worst <= TOL, f"{worst:.3e}"
    # x = 0: the oracle's class, and its number where it has one
    g0, r0 = got[0], ref[0]
    assert np.array_equal(np.isnan(g0), np.isnan(r0)) and np.array_equal(np.isinf(g0), np.isinf(r0))
    assert (g0[np.isinf(r0)] > 0).all() and np.array_equal(g0 == 0.0, r0 == 0.0)
    num = np.isfinite(r0) & (r0 != 0.0)
    assert (np.abs(g0[num] - r0[num]) <= TOL * np.abs(r0[num])).all()
    if kind == 0:   # per_mode = 0: the mode-order fp64 sum
        total = density(cloudy, plan, mom, H.GRID, per_mode=0)
        s = np.zeros_like(got[:, 0])
        for m in range(Nm):
            s = s + got[:, m]
        assert bits_equal(total, s)
    # one grid value replaced by -1: NaN in every plane of that point, the bits of the other planes kept
    grid = H.GRID.copy()
    grid[5] = -1.0
    bad = density(cloudy, plan, mom, grid, kind=kind).reshape(got.shape)
    assert np.isnan(bad[5]).all()
    keep = np.arange(len(grid)) != 5
    assert bits_equal(bad[keep], got[keep])
    grid[5] = float("nan")
    assert np.isnan(density(cloudy, plan, mom, grid, kind=kind).reshape(got.shape)[5]).all()


# ---- the reference's known answers on the device
def test_reference_known_answers(gpu_cloudy, kats):
    cloudy = gpu_cloudy
    code = {"exponential": 0, "gamma": 1, "monodisperse": 2, "lognormal": 3}
    done = 0
    for e in kats["update_dist_from_moments"]:
        if not ("expected_moments" in e or "normed_density_at_0" in e or "normed_density_at_1" in e):
            continue
        t = code[e["type"]]
        plan = cloudy.Plan([t], [[1.0]], (INF,), (1.0, 1.0), 0, k_range=tuple(e.get("k_range", (H.EPS, 10.0))))
        mom = dev(cloudy, np.array(e["moments"], dtype=np.float64).reshape(-1, 1))
        if "expected_moments" in e:
            want = np.array(e["expected_moments"])
            got = cloudy.moment(plan, mom, [float(q) for q in range(len(want))]).to_numpy()[:, 0]
            assert np.allclose(got, want, rtol=e["rtol"], atol=1e-300), e["cite"]
        for key, x in (("normed_density_at_0", 0.0), ("normed_density_at_1", 1.0)):
            if key in e:
                got = cloudy.normed_density(plan, mom, x).to_numpy()[0, 0]
                assert got == pytest.approx(e[key], rel=e.get("rtol", 1e-12)), (e["cite"], key)
        done += 1
    assert done >= 4


# ---- shapes
@pytest.mark.parametrize("n_x", [1, H.MAX_GRID])
def test_grid_sizes_one_and_the_largest(gpu_cloudy, oracle, n_x):
    cloudy = gpu_cloudy
    plan = family_plan(cloudy, oracle, "exp_gamma")
    _, mom = H.batch("exp_gamma")
    grid = np.array([3e-10]) if n_x == 1 else np.logspace(-14, -5, n_x)
    got = density(cloudy, plan, mom, grid, n=65).reshape(n_x, 2, 65)   # (launch asserts the planes, the guard and the tails)
    ds = H.dists(oracle, "exp_gamma")
    n0, m0 = bench.NORMS
    for j in sorted({0, n_x // 3, n_x - 1}):
        ref = np.array([[n0 / m0 * oracle.density(ds[i][m], grid[j] / m0) for i in range(65)] for m in range(2)])
        big = ref >= 1e-250
        assert (np.abs(got[j] - ref)[big] <= TOL * ref[big]).all(), j


@pytest.mark.parametrize("n_orders", [1, 8])
def test_order_counts_one_and_the_largest(gpu_cloudy, oracle, n_orders):
    cloudy = gpu_cloudy
    plan = family_plan(cloudy, oracle, "exp_gamma")
    _, mom = H.batch("exp_gamma")
    orders = H.ORDERS[:n_orders]
    got = moments(cloudy, plan, mom, orders, n=65).reshape(2, n_orders, 65)
    ref = H.reference_moments(oracle, "exp_gamma", H.ORDERS)[:, :n_orders, :65]
    assert (np.abs(got - ref) <= TOL * ref).all()


# ---- bits
@pytest.mark.parametrize("family", ["gamma_lognormal_mono", "numerical"])
def test_same_bits_again_on_a_fresh_plan_and_for_the_reversed_batch(gpu_cloudy, oracle, family):
    cloudy = gpu_cloudy
    plan = family_plan(cloudy, oracle, family)
    _, mom = H.batch(family)
    rev = np.ascontiguousarray(mom[:, ::-1])
    for run in (lambda p, m: moments(cloudy, p, m, H.ORDERS, x_t=1e-9), lambda p, m: moments(cloudy, p, m, H.ORDERS),
                lambda p, m: density(cloudy, p, m, H.GRID)):
        first = run(plan, mom)
        assert bits_equal(run(plan, mom), first)
        assert bits_equal(run(family_plan(cloudy, oracle, family, 0, 0, 1), mom), first)
        assert bits_equal(run(plan, rev)[:, ::-1], first)


# ---- float planes
@pytest.mark.parametrize("family", ["exp_gamma", "gamma_lognormal_mono"])
def test_float_planes_are_the_fp64_result_rounded_once(gpu_cloudy, oracle, family):
    cloudy = gpu_cloudy
    p64, p32 = family_plan(cloudy, oracle, family), family_plan(cloudy, oracle, family, cloudy.F32)
    _, mom = H.batch(family)
    m32 = mom.astype(np.float32)
    m64 = m32.astype(np.float64)
    tiny = float(np.finfo(np.float32).tiny)
    for run in (lambda p, m: moments(cloudy, p, m, H.ORDERS), lambda p, m: moments(cloudy, p, m, H.ORDERS, x_t=1e-9, per_mode=0),
                lambda p, m: density(cloudy, p, m, H.GRID[1:])):
        want, got = run(p64, m64), run(p32, m32)
        assert got.dtype == np.float32
        normal = np.isfinite(want) & (np.abs(want) >= tiny) & (np.abs(want) <= float(np.finfo(np.float32).max))
        assert normal.sum() > normal.size // 4
        assert (np.abs(got.astype(np.float64) - want)[normal] <= 2.0**-24 * np.abs(want)[normal]).all()


# ---- refusals that need a plan
def test_refusals_with_a_plan_write_nothing(gpu_cloudy, oracle):
    cloudy, E = gpu_cloudy, gpu_cloudy._lib
    _, mom = H.batch("gamma_lognormal_mono")
    msg = density(cloudy, family_plan(cloudy, oracle, "gamma_lognormal_mono"), mom, H.GRID, kind=1, expect=E.EINVAL)
    assert "no method normed_density_func for a Monodisperse distribution" in msg
    off = family_plan(cloudy, oracle, "exp_gamma", 0, -1)
    _, mom = H.batch("exp_gamma")
    assert "plan-time compilation is off or failed" in moments(cloudy, off, mom, H.ORDERS, expect=E.EUNSUPPORTED)
    assert "plan-time compilation is off or failed" in density(cloudy, off, mom, H.GRID, expect=E.EUNSUPPORTED)
