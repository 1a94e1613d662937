"""cloudy_moments / cloudy_density without a GPU: the two symbols in the header, the ctypes table, the library and the Julia shim; the
refusals that need no plan, in their order; the plan-time unit (csrc/spectra.hpp) compiled for gfx950; and the inputs of
tests/test_gpu_spectra.py, chosen here on the oracle alone, with the conditions that file relies on asserted here.

The reference of both files is the unchanged oracle: update_dist_batch gives the normalised (n, theta, k) of a parcel, moment /
partial_moment / density / normed_density of oracle/cloudy_oracle.py the normalised values, and the physical ones follow as the
header says: n0 m0^q times a moment, n0 / m0 (1 / m0) times a (normed) density at x / m0."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import bench
from gpu_support import EPS, GOLOVIN, INF, many_mode_moments, mixed_moments
from tsit5_restated import assert_symbol_agrees

N_PARCELS = 257                       # one full workgroup and a one-lane second one
LD = N_PARCELS + 15
ORDERS = (0.0, 0.25, 2.0 / 3.0, 1.0, 7.0 / 6.0, 2.0, 3.5, 6.0)
ONE_ORDER = (1.0 / 3.0,)
CUTOFFS = (1e-10, 1e-9, 3e-8)         # kg
GRID = np.concatenate([[0.0], np.logspace(-14, -5, 36)])   # kg
FLOOR = 1e-30                         # of a mode's peak on the grid: the bound of the densities holds at and above it
FAMILIES = {"exp_gamma": [0, 1], "gamma_lognormal_mono": [1, 3, 2], "eight_gamma": [1] * 8, "numerical": [1, 1]}
MAX_ORDERS, MAX_GRID = 8, 1024


def header_constant(name):
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return int(re.search(rf"#define {name} (\d+)", open(os.path.join(root, "include", "cloudy_hip.h")).read()).group(1))


@functools.lru_cache(maxsize=None)
def batch(family):
    """(dist_types, physical moments (nmom, 257)) of a family: the generators' batch with five kinds of parcels put in by hand --
    parcel 1 empty in every mode, parcel 2 empty in its first Gamma mode, parcels 4 and 6 with that mode's shape at the upper and
    at the lower clamp (k = 25 and a negative variance at 1e7 drops of 1e-10 kg), and every fourth parcel of a Monodisperse mode 3 %
    off a grid point (its pulse of half width theta / 10 would otherwise miss a grid of four points per decade)."""
    types = FAMILIES[family]
    mom = mixed_moments(types, N_PARCELS, seed=20 + len(types)).copy()
    offs = np.cumsum([0] + [3 if t in (1, 3) else 2 for t in types])
    g = types.index(1)
    r = offs[g]
    mom[:, 1] = 0.0
    mom[r:r + 3, 2] = 0.0
    m0, m1 = 1e7, 1e7 * 1e-10
    mom[r:r + 3, 4] = (m0, m1, m1 * m1 / m0 * (1.0 + 1.0 / 25.0))   # (k = 25: zero variance itself is decided by the last bit)
    mom[r:r + 3, 6] = (m0, m1, 0.5 * m1 * m1 / m0)
    for i, t in enumerate(types):
        if t == 2:
            for p in range(8, N_PARCELS, 4):
                mom[offs[i] + 1, p] = mom[offs[i], p] * GRID[1 + p % 36] * 1.03
    return types, np.ascontiguousarray(mom)


def oracle_params(oracle, family):
    types = FAMILIES[family]
    return oracle.make_params(list(types), np.asarray(GOLOVIN), (INF,) * len(types), norms=bench.NORMS)


@functools.lru_cache(maxsize=None)
def dists(oracle, family):
    """[parcel][mode] -> the oracle's distribution of the normalised moments"""
    types, mom = batch(family)
    prm = oracle.update_dist_batch(oracle_params(oracle, family), mom)
    return [[oracle.make_dist(t, *prm[3 * m:3 * m + 3, i]) for m, t in enumerate(types)] for i in range(mom.shape[1])]


@functools.lru_cache(maxsize=None)
def reference_moments(oracle, family, orders, x_threshold=INF):
    """(N, len(orders), n) physical"""
    n0, m0 = bench.NORMS
    ds = dists(oracle, family)
    out = np.empty((len(ds[0]), len(orders), len(ds)))
    for i, row in enumerate(ds):
        for m, d in enumerate(row):
            for j, q in enumerate(orders):
                v = oracle.moment(d, q) if np.isinf(x_threshold) else oracle.partial_moment(d, q, x_threshold / m0)
                out[m, j, i] = (n0 * m0**q) * v
    return out


@functools.lru_cache(maxsize=None)
def reference_density(oracle, family, normed):
    """(len(GRID), N, n) physical"""
    n0, m0 = bench.NORMS
    ds = dists(oracle, family)
    f = oracle.normed_density if normed else oracle.density
    out = np.empty((len(GRID), len(ds[0]), len(ds)))
    with np.errstate(all="ignore"):
        for i, row in enumerate(ds):
            for m, d in enumerate(row):
                for j, x in enumerate(GRID):
                    out[j, m, i] = ((1.0 if normed else n0) / m0) * f(d, x / m0)
    return out


def fallback(oracle, family):
    """(N, n): the mode is the fallback (0, 1, 1)"""
    ds = dists(oracle, family)
    return np.array([[d.n == 0.0 and d.theta == 1.0 and d.k == 1.0 for d in row] for row in ds]).T


# ---- 1. the symbols
def test_symbols_agree_in_header_ctypes_library_and_julia(cloudy):
    assert_symbol_agrees(cloudy, "cloudy_moments", ["ptr", "size_t", "size_t", "ptr", "int", "ptr", "double", "int", "ptr", "ptr"])
    assert_symbol_agrees(cloudy, "cloudy_density", ["ptr", "size_t", "size_t", "ptr", "int", "size_t", "ptr", "int", "ptr", "ptr"])
    assert (header_constant("CLOUDY_MAX_ORDERS"), header_constant("CLOUDY_MAX_GRID")) == (MAX_ORDERS, MAX_GRID)
    assert (cloudy._lib.MAX_ORDERS, cloudy._lib.MAX_GRID, cloudy._lib.DENSITY, cloudy._lib.NORMED_DENSITY) == (8, 1024, 0, 1)
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "julia", "CloudyHIP.jl")).read()
    assert "function moments!(" in src and "function density!(" in src
    for name in ("moment", "partial_moment", "density", "normed_density"):
        assert name in cloudy.__all__


# ---- 2. the refusals that need no plan, in their order
def test_plan_free_refusals_of_cloudy_moments(cloudy):
    L, E = cloudy.lib(), cloudy._lib
    dummy = C.c_void_p(64)   # never dereferenced
    good = (C.c_double * 8)(*ORDERS)

    def call(n=4, ld=4, mom=dummy, n_orders=8, orders=good, x_t=INF, per_mode=1, out=dummy):
        return L.cloudy_moments(None, n, ld, mom, n_orders, orders, x_t, per_mode, out, None)

    def refused(words, **kw):
        assert call(**kw) == E.EINVAL and words in L.cloudy_last_error().decode(), (kw, L.cloudy_last_error())

    assert call() == E.EINVAL and L.cloudy_last_error().decode() == "plan is NULL"
    assert call(x_t=1e-9, per_mode=0, n_orders=1) == E.EINVAL and L.cloudy_last_error().decode() == "plan is NULL"
    assert call(n=0, ld=0, mom=None, out=None) == E.EINVAL and L.cloudy_last_error().decode() == "plan is NULL"
    for bad in (0, -1, MAX_ORDERS + 1):
        refused("n_orders", n_orders=bad)
    refused("orders is NULL", orders=None)
    for bad in (float("nan"), INF, -0.5, 16.5):
        refused("orders[2]", orders=(C.c_double * 8)(0.0, 1.0, bad, *ORDERS[3:]))
    assert call(orders=(C.c_double * 8)(16.0, *ORDERS[1:])) == E.EINVAL and L.cloudy_last_error().decode() == "plan is NULL"
    for bad in (float("nan"), 0.0, -1e-9, -INF):
        refused("x_threshold", x_t=bad)
    for bad in (-1, 2):
        refused("per_mode", per_mode=bad)
    refused("ld (3) must be >= n_parcels (4)", ld=3)
    refused("device buffer is NULL", mom=None)
    refused("device buffer is NULL", out=None)
    # in their order: an earlier argument out of order is named beside a later one
    refused("n_orders", n_orders=0, orders=None, x_t=-1.0, per_mode=5, ld=3)
    refused("orders is NULL", orders=None, x_t=-1.0, per_mode=5, ld=3)
    refused("x_threshold", x_t=-1.0, per_mode=5, ld=3)
    refused("per_mode", per_mode=5, ld=3, mom=None)
    refused("ld (3)", ld=3, mom=None)


def test_plan_free_refusals_of_cloudy_density(cloudy):
    L, E = cloudy.lib(), cloudy._lib
    dummy = C.c_void_p(64)   # never dereferenced

    def call(n=4, ld=4, mom=dummy, kind=0, n_x=37, x=dummy, per_mode=1, out=dummy):
        return L.cloudy_density(None, n, ld, mom, kind, n_x, x, per_mode, out, None)

    def refused(words, **kw):
        assert call(**kw) == E.EINVAL and words in L.cloudy_last_error().decode(), (kw, L.cloudy_last_error())

    for ok in (dict(), dict(kind=1), dict(per_mode=0), dict(n_x=1), dict(n_x=MAX_GRID), dict(n=0, ld=0, mom=None, out=None)):
        assert call(**ok) == E.EINVAL and L.cloudy_last_error().decode() == "plan is NULL", ok
    for bad in (-1, 2):
        refused("kind", kind=bad)
    for bad in (0, MAX_GRID + 1):
        refused("n_x", n_x=bad)
    refused("x_dev is NULL", x=None)
    for bad in (-1, 2):
        refused("per_mode", per_mode=bad)
    refused("CLOUDY_NORMED_DENSITY", kind=1, per_mode=0)
    refused("ld (3) must be >= n_parcels (4)", ld=3)
    refused("device buffer is NULL", mom=None)
    refused("device buffer is NULL", out=None)
    refused("kind", kind=7, n_x=0, x=None, per_mode=3, ld=3)
    refused("n_x", n_x=0, x=None, per_mode=3, ld=3)
    refused("x_dev is NULL", x=None, per_mode=3, ld=3)
    refused("per_mode", per_mode=3, ld=3)
    refused("CLOUDY_NORMED_DENSITY", kind=1, per_mode=0, ld=3)
    refused("ld (3)", ld=3, out=None)


# ---- 3. the plan-time unit
@pytest.mark.parametrize("case", ["gamma", "cfg3b", "moving", "eight", "numerical"])
def test_spectra_unit_compiles_without_a_gpu(cloudy, case, tmp_path, monkeypatch):
    """cloudy_jit_selfcheck compiles every unit the runtime could request for a plan: exactly one dumped unit names spectra.hpp, it
    defines exactly the two kernels and has a code object; no other unit holds a spectra kernel"""
    monkeypatch.setenv("CLOUDY_HIP_JIT_DUMP", str(tmp_path))
    L = cloudy.lib()
    keep = None
    if case == "numerical":
        d = cloudy.NumericalPlan.make_desc([1, 1], cloudy.LinearKernelFunction(5e-3), bench.NORMS, 10, quad_mode=cloudy.QUAD_FIXED)
    elif case == "cfg3b":
        spec = bench.workload_spec(case)
        d, keep = cloudy.Plan.make_desc([1] * spec["n_modes"], bench.kernel_matrix(spec), spec["thresholds"], bench.NORMS, 0)
    elif case == "moving":
        d, keep = cloudy.Plan.make_desc([1, 1], bench.kernel_matrix(bench.workload_spec("cfg3a")), (0.9, 1.0), bench.NORMS, 1)
    elif case == "eight":
        d, keep = cloudy.Plan.make_desc([1] * 8, np.array(GOLOVIN), (INF,) * 8, bench.NORMS, 0)
    else:
        d, keep = cloudy.Plan.make_desc([1], np.array(GOLOVIN), (INF,), bench.NORMS, 0)
    assert L.cloudy_jit_selfcheck(C.byref(d), b"gfx950") == 0, L.cloudy_last_error().decode()
    texts = {f: open(tmp_path / f).read() for f in sorted(os.listdir(tmp_path)) if f.endswith(".hip")}
    units = [f for f, t in texts.items() if "spectra.hpp" in t]
    assert len(units) == 1, units
    text = texts[units[0]]
    assert text.count("__global__") == 2
    assert text.count(" cloudy_jit_spectra_moments_") == 1 and text.count(" cloudy_jit_spectra_density_") == 1
    assert os.path.getsize(tmp_path / units[0].replace(".hip", ".co")) > 1000
    assert not [f for f, t in texts.items() if f != units[0] and "cloudy_jit_spectra" in t]


# ---- 4. the inputs of the GPU file, and what it relies on
@pytest.mark.parametrize("family", list(FAMILIES))
def test_batches_hold_fallbacks_and_both_clamps(oracle, family):
    types, mom = batch(family)
    assert mom.shape == (sum(3 if t in (1, 3) else 2 for t in types), N_PARCELS)
    stats = oracle.closure_stats(oracle_params(oracle, family), mom)   # columns: fallback, k at the lower, at the upper clamp
    assert stats[:, 0].min() >= 1, stats
    assert stats[:, 1].max() >= 1 and stats[:, 2].max() >= 1, stats
    fb = fallback(oracle, family)
    assert fb[:, 1].all() and fb[types.index(1), 2] and not fb[:, 8].any()
    ks = np.array([[d.k for d in row] for row in dists(oracle, family)])
    assert (ks == EPS).any() and (ks == 10.0).any()


@pytest.mark.parametrize("family", list(FAMILIES))
def test_grid_covers_both_sides_of_the_floor_and_the_oracle_is_finite(oracle, family):
    """The grid is x = 0 plus 36 log-spaced masses from 1e-14 to 1e-5 kg.  For every mode of every family the batch has densities
    both at or above 1e-30 of the mode's peak on the grid (where the bound of the GPU file holds) and below it (where only
    smallness is asked) -- over the batch, not parcel by parcel: a Monodisperse pulse that misses the grid is zero on all of it,
    and a Gamma mode whose shape sits at the lower clamp spans nine decades on nine decades of mass.  The oracle is finite
    everywhere but at x = 0, where it has the classes of the header: Inf (Gamma, k < 1), a number or 0, NaN (Lognormal)."""
    types, _ = batch(family)
    assert GRID[0] == 0.0 and len(GRID) == 37 and GRID[1] == 1e-14 and abs(GRID[-1] - 1e-5) < 1e-20
    fb = fallback(oracle, family)
    ks = np.array([[d.k for d in row] for row in dists(oracle, family)]).T
    for normed in (False, True):
        if normed and 2 in types:
            continue
        ref = reference_density(oracle, family, normed)
        assert np.isfinite(ref[1:]).all()
        at0, any_low = ref[0], False
        for m, t in enumerate(types):
            if t == 3:
                assert np.isnan(at0[m]).all()
            elif t == 1:
                low = (ks[m] < 1.0) & ~fb[m]
                any_low = any_low or low.any()
                assert np.isinf(at0[m][low]).all() and np.isfinite(at0[m][~low]).all()
                assert (at0[m][(ks[m] > 1.0)] == 0.0).all()
                if not normed:
                    assert (at0[m][fb[m]] == 0.0).all()
            else:
                assert np.isfinite(at0[m]).all() and (t == 2 or (at0[m][~fb[m]] > 0.0).all())
            live = ref[1:, m][:, ~fb[m]]
            peak = live.max(axis=0)
            assert (peak > 0).sum() >= (8 if t == 2 else live.shape[1] - 8)
            above = live >= FLOOR * peak
            assert (above & (live > 0)).sum() >= 50 and (~above | (live == 0)).sum() >= 1
        assert any_low


def test_cutoffs_give_small_large_and_middling_fractions_for_each_closure(oracle):
    """over the eight orders of the GPU file (an Exponential cloud mode keeps more than 1e-6 of its number below any of the cutoffs;
    its sixth moment does not)"""
    seen = {t: set() for t in (0, 1, 2, 3)}
    for family, types in FAMILIES.items():
        fb = fallback(oracle, family)
        full = reference_moments(oracle, family, ORDERS)
        for x_t in CUTOFFS:
            part = reference_moments(oracle, family, ORDERS, x_t)
            assert np.isfinite(part).all() and (part >= 0).all() and (part <= full * (1 + 1e-12)).all()
            for m, t in enumerate(types):
                frac = part[m][:, ~fb[m]] / full[m][:, ~fb[m]]
                seen[t] |= {"small"} if (frac < 1e-6).any() else set()
                seen[t] |= {"large"} if (frac > 1 - 1e-6).any() else set()
                seen[t] |= {"middle"} if ((frac > 1e-3) & (frac < 1 - 1e-3)).any() else set()
    assert seen[0] == seen[1] == seen[3] == {"small", "large", "middle"}, seen
    assert seen[2] == {"small", "large"}, seen   # (a Monodisperse mode is below the cutoff or above it)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_reference_moments_are_finite_and_zero_for_fallback_modes(oracle, family):
    fb = fallback(oracle, family)
    for orders in (ORDERS, ONE_ORDER):
        ref = reference_moments(oracle, family, orders)
        assert np.isfinite(ref).all() and (ref >= 0).all()
        for m in range(ref.shape[0]):
            assert (ref[m][:, fb[m]] == 0.0).all() and (ref[m][:, ~fb[m]] > 0.0).all()
