"""GPU tests of the RANKED FIXED-STEP kernels: on a plan with a finite or moving threshold every right-hand-side evaluation ranks
the workgroup's parcels through LDS (regime_rank), each lane integrates the parcel of its rank and hands the result back through
sh_T / sh_par (coal_ints_ranked_impl, coal_rhs_sorted_body.inc).  kernels.hpp says of this exchange that "any permutation gives
the same results, parcels are independent": here a parcel's bits are compared across runs in which its lane, wave, workgroup and
neighbours change, with zero, NaN, Inf and negative parcels among the neighbours.  Besides: the order of columns in the column
integrator, and the unrolled loop of plane_partial_sums_kernel at the sizes where it starts.

Run with `-m gpu`.  Every batch, seed, step and parcel picked is chosen and justified on the oracle alone in
tests/test_ranked_fixed_host.py.  Every call is out of place with ld = n + 15, padding columns of 7.0 in the input and outputs
filled with the sentinel NaN; after every call the padding is untouched and the input unchanged.

Plans (test_ranked_fixed_host.PLANS): `fixed` = the bench's cfg3b (two Gamma modes, thresholds (5e-10, Inf) as bench.workload_spec
has them), `two_thr` = cfg4 (three modes, order-4 tensor, two thresholds), `moving` = moving4 (four modes, MovingThreshold).

(entry, plan) combinations that run: rhs, rhs_f32, ssprk33, tsit5 and box on each of fixed, two_thr and moving; sources on fixed
(the issue asks for no other).  The library refuses none of them with CLOUDY_EUNSUPPORTED; a refusal would skip the combination
with the library's text (run()).

Bounds of test 1, all the project's own: TOL_QUAD x scale and the relative 1e-10 of assert_close_scaled for rhs
(test_bench_workloads_vs_oracle); 6e-8 |want| + 1e-12 scale + 1.5e-45 for rhs_f32 (test_fp32_planes_vs_fp64_oracle); TOL_QUAD x
scale for the coalescence source and rtol 1e-11 for the flux of sources (test_sedimentation_flux_kat_and_rainshaft_sources);
max(1e3 TOL_QUAD, 1e-9) of |u0| + |u| on the regular parcels for ssprk33, tsit5
(test_fused_integrators_two_moment_mode_partial_workgroup_and_padding) and box (test_gpu_box_sources), 2 steps of 1e-3 s (cfg4,
which no existing test steps: 1e-7 s, chosen on the oracle in the host file).  Regular parcels are those of the existing stepping
tests that the oracle stepping itself resolves to a tenth of that bound under a one-ulp change of its input (host file:
resolved()); that drops one parcel of one case (tsit5 on moving), where the oracle moves by 8e-3.

Measured on an MI355X at n = 1025, worst value of each comparison of test 1: rhs 1.61e-14 / 1.73e-14 / 6.23e-15 of scale (fixed /
two_thr / moving); rhs_f32 0.974 / 0.973 / 0.988 of its bound; ssprk33 5.92e-11 / 1.43e-13 / 1.01e-12; tsit5 4.54e-11 / 1.09e-13 /
3.86e-12; box 5.93e-11 / 1.31e-13 / 7.77e-13; sources 1.61e-14 of scale, flux 1.01e-14 relative."""
import functools

import numpy as np
import pytest

import bench
import test_ranked_fixed_host as R
from gpu_support import TOL_QUAD, _ssprk33_host, _tsit5_host, assert_close_scaled, bits_equal, blank, dev, is_blank, rel_err

pytestmark = pytest.mark.gpu

ENTRIES = ("rhs", "rhs_f32", "ssprk33", "tsit5", "box")
CASES = [(e, p) for e in ENTRIES for p in R.PLANS] + [("sources", "fixed")]
both = pytest.mark.parametrize("entry,plan", CASES)
N = R.N


@functools.lru_cache(maxsize=None)
def device_plan(cloudy, plan, dtype=0, vel=False):
    wl = bench.make_workload(R.PLANS[plan], 1)
    return wl["coal_data"].plan(wl["dist_types"], dtype=dtype, **({"vel": R.VEL} if vel else {}))


def run(cloudy, entry, plan, u0, s):
    """one call of an entry point on the parcels (u0, s): ld = n + 15, out of place, padding of 7.0, sentinel-filled outputs
    -> dict(out: the output planes, one array per output of the entry; pad, u_in, buf)"""
    L = cloudy.lib()
    dtype = np.float32 if entry == "rhs_f32" else np.float64
    p = device_plan(cloudy, plan, dtype=1 if entry == "rhs_f32" else 0, vel=entry == "sources")
    planes, n = u0.shape
    ld = n + 15
    buf = np.full((planes, ld), 7.0, dtype=dtype)
    buf[:, :n] = u0
    u_in = dev(cloudy, buf)
    outs = [dev(cloudy, blank(planes, ld, dtype)) for _ in range(2 if entry == "sources" else 1)]
    if entry in ("rhs", "rhs_f32"):
        rc = L.cloudy_coal_rhs(p.handle, n, ld, u_in.ptr, outs[0].ptr, None)
    elif entry == "ssprk33":
        rc = L.cloudy_ssprk33_steps(p.handle, n, ld, u_in.ptr, outs[0].ptr, R.DT[plan], R.N_STEPS, None)
    elif entry == "tsit5":
        rc = L.cloudy_tsit5_steps(p.handle, n, ld, u_in.ptr, outs[0].ptr, R.DT[plan], R.N_STEPS, None)
    elif entry == "box":
        s_d = dev(cloudy, np.pad(np.asarray(s, dtype=np.float64), (0, ld - n))[None, :])
        rc = L.cloudy_box_ssprk33_steps(p.handle, n, ld, u_in.ptr, outs[0].ptr, cloudy.SRC_COAL | cloudy.SRC_COND, s_d.ptr, 0.0, R.XI,
                                        R.DT[plan], R.N_STEPS, None)
    else:
        rc = L.cloudy_rainshaft_sources(p.handle, n, ld, u_in.ptr, outs[0].ptr, outs[1].ptr, None)
    if rc == cloudy._lib.EUNSUPPORTED:
        pytest.skip(f"{entry} on {plan}: {L.cloudy_last_error().decode()}")
    assert rc == 0, (rc, L.cloudy_last_error().decode())
    got = [o.to_numpy() for o in outs]
    res = dict(out=[g[:, :n] for g in got], pad=[g[:, n:] for g in got], u_in=u_in.to_numpy(), buf=buf)
    assert all(np.all(is_blank(q)) for q in res["pad"]), "the padding columns were written"
    assert bits_equal(res["u_in"], res["buf"]), "the input changed"
    return res


def inputs(entry, plan, hostile=False):
    u0, s, role = R.batch(plan, hostile)
    return (u0.astype(np.float32) if entry == "rhs_f32" else u0), s, role


@functools.lru_cache(maxsize=None)
def whole(cloudy, entry, plan, hostile=False):
    """the run of the whole batch at n = 1025, once per session"""
    u0, s, _ = inputs(entry, plan, hostile)
    return run(cloudy, entry, plan, u0, s)


def assert_same_bits(base, part, idx, flip=False):
    """the parcels idx of the whole run have the bits of the run `part` (flip: whose batch was reversed), in every output plane"""
    assert len(base["out"]) == len(part["out"])
    for k, (b, q) in enumerate(zip(base["out"], part["out"])):
        assert bits_equal(b[:, idx], q[:, ::-1] if flip else q), (k, idx)


# ---- 1. parity at 1025
@both
def test_parity_at_1025(gpu_cloudy, oracle, entry, plan):
    got = whole(gpu_cloudy, entry, plan)
    u0, s, _ = inputs(entry, plan)
    op = bench.oracle_params(R.PLANS[plan])
    out = got["out"][0]
    if entry == "rhs":
        want, scale = oracle.rhs_coal_batch(op, u0, with_scale=True)
        worst = assert_close_scaled(out, want, scale, TOL_QUAD, f"{entry} {plan}")
        print(f"{entry} {plan} n={N}: max |hip - oracle| / scale = {worst:.2e} (bound {TOL_QUAD:g})")
    elif entry == "rhs_f32":
        assert out.dtype == np.float32
        want, scale = oracle.rhs_coal_batch(op, u0.astype(np.float64), with_scale=True)
        with np.errstate(over="ignore"):
            fin = np.isfinite(want.astype(np.float32))
        both_fin = fin & np.isfinite(out)
        err = np.abs(out.astype(np.float64)[both_fin] - want[both_fin])
        bound = 6.0e-8 * np.abs(want[both_fin]) + 1e-12 * scale[both_fin] + 1.5e-45
        print(f"{entry} {plan} n={N}: {int((np.isfinite(out) != fin).sum())} entries differ in finiteness; max err / bound = "
              f"{(err / bound).max():.3f} (bound 6e-8 |want| + 1e-12 scale + 1.5e-45)")
        assert np.array_equal(np.isfinite(out), fin)
        assert np.all(err <= bound), (err / bound).max()
    elif entry == "sources":
        vop = R.bench_oracle_params_with_velocity()
        wcs, wsf = oracle.rainshaft_cell_batch(vop, u0)
        _, scale = oracle.rhs_coal_batch(vop, np.maximum(u0, 0.0), with_scale=True)
        cs, sf = got["out"]
        worst = (np.abs(cs - wcs) / np.maximum(scale, 1e-300)).max()
        with np.errstate(all="ignore"):
            flux = np.nanmax(np.where(wsf != 0.0, np.abs(sf - wsf) / np.abs(wsf), np.abs(sf)))
        print(f"{entry} {plan} n={N}: coalescence source max |hip - oracle| / scale = {worst:.2e} (bound {TOL_QUAD:g}); flux max "
              f"relative error {flux:.2e} (bound 1e-11)")
        assert np.all(np.abs(cs - wcs) <= TOL_QUAD * np.maximum(scale, 1e-300))
        assert np.allclose(sf, wsf, rtol=1e-11, atol=0)
    else:
        want, ok = R.stepping_reference(plan, entry)   # (box: gpu_support.oracle_reference)
        assert ok.sum() >= 0.9 * N, ok.sum()
        err = rel_err(out, want, u0, ok)
        bound = max(1e3 * TOL_QUAD, 1e-9)
        print(f"{entry} {plan} n={N}: {int(ok.sum())} regular parcels, max |hip - oracle stepping| / (|u0| + |u|) = {err.max():.2e} "
              f"(bound {bound:g})")
        assert err.max() < bound, err.max()


# ---- 2. the reversed batch
@both
def test_reversed_batch(gpu_cloudy, entry, plan):
    """parcel i at column n - 1 - i (its supersaturation with it): every lane, wave and workgroup changes, parcel 0 is the tail"""
    u0, s, _ = inputs(entry, plan)
    part = run(gpu_cloudy, entry, plan, np.ascontiguousarray(u0[:, ::-1]), s[::-1])
    assert_same_bits(whole(gpu_cloudy, entry, plan), part, slice(None), flip=True)


# ---- 3. sub-batches
@both
def test_sub_batches(gpu_cloudy, entry, plan):
    """[0, 65), [224, 289), [480, 545) and [n - 65, n) alone -- the middle ones straddle the 256 and 512 boundaries, so their
    parcels change workgroup -- and the prefixes of 257 and 513 parcels (a full workgroup + one lane): the bits of the whole run,
    NaN for NaN with the same payload"""
    u0, s, _ = inputs(entry, plan)
    base = whole(gpu_cloudy, entry, plan)
    for lo, hi in R.WINDOWS:
        idx = slice(lo, hi)
        assert_same_bits(base, run(gpu_cloudy, entry, plan, np.ascontiguousarray(u0[:, idx]), s[idx]), idx)


# ---- 4. parcels alone
@both
def test_parcels_alone(gpu_cloudy, oracle, entry, plan):
    """test_ranked_fixed_host.singletons: at most 12 launches of one parcel"""
    u0, s, _ = inputs(entry, plan)
    base = whole(gpu_cloudy, entry, plan)
    picked, _, _ = R.singletons(oracle, plan)
    assert len(picked) <= 12
    for i in picked:
        idx = slice(i, i + 1)
        assert_same_bits(base, run(gpu_cloudy, entry, plan, np.ascontiguousarray(u0[:, idx]), s[idx]), idx)


# ---- 5. hostile neighbours
def oracle_on(oracle, entry, plan, u0, s):
    """what the oracle gives for the parcels (u0, s) through an entry -> one array per output"""
    op = bench.oracle_params(R.PLANS[plan])
    with np.errstate(all="ignore"):
        if entry in ("rhs", "rhs_f32"):
            want = oracle.rhs_coal_batch(op, u0.astype(np.float64))
            return [want.astype(np.float32) if entry == "rhs_f32" else want]
        if entry == "sources":
            return list(oracle.rainshaft_cell_batch(R.bench_oracle_params_with_velocity(), u0))
        host = _tsit5_host if entry == "tsit5" else _ssprk33_host
        return [host(R.oracle_rhs(oracle, plan, entry, s), u0, R.DT[plan], R.N_STEPS)]


@both
def test_hostile_neighbours(gpu_cloudy, oracle, entry, plan):
    """Four of five roles of test_ranked_fixed_host.hostile_batch are bad parcels beside every kept one: the call returns
    CLOUDY_OK (run() asserts it, and the padding and the input); the kept parcels have the bits of the clean whole run in every
    plane; the copies of the densest parcel have its bits; an all-zero parcel gives what the oracle gives for it where that is
    finite; of the NaN, Inf and negative parcels only the contract of test_error_behaviour_on_device: the modes whose shape the
    oracle's inversion gives as NaN have NaN in their planes."""
    u0, s, _ = inputs(entry, plan)
    h0, hs, role = inputs(entry, plan, hostile=True)
    base, got = whole(gpu_cloudy, entry, plan), whole(gpu_cloudy, entry, plan, hostile=True)
    kept = np.flatnonzero(role == -1)
    for b, g in zip(base["out"], got["out"]):
        assert bits_equal(b[:, kept], g[:, kept])
    dense = int(np.argmax(u0[0]))
    for b, g in zip(base["out"], got["out"]):
        lanes = g[:, role == 4]
        assert bits_equal(lanes, np.repeat(b[:, dense:dense + 1], lanes.shape[1], axis=1))
    zero = role == 0
    for g, w in zip(got["out"], oracle_on(oracle, entry, plan, np.ascontiguousarray(h0[:, zero]), hs[zero])):
        fin = np.isfinite(w)
        assert fin.any() and np.array_equal(g[:, zero][fin], w[fin])
    modes = R.nan_modes(oracle, plan, sources=entry == "sources")
    for r, ms in modes.items():
        for m in ms:
            assert np.isnan(got["out"][0][3 * m:3 * m + 3][:, role == r]).all(), (R.ROLES[r], m)


# ---- 6. the order of columns
COLUMN_ENTRIES = ("steps", "rhs")


def run_columns(cloudy, entry, u0, ncol):
    """cloudy_rainshaft_ssprk33_steps (2 steps) or cloudy_rainshaft_rhs on ncol columns of NZ cells of the `fixed` plan with
    velocity; ld = n + 15, out of place, sentinel-filled outputs -> the output planes (the right-hand side: and the flux planes)"""
    L = cloudy.lib()
    p = device_plan(cloudy, "fixed", vel=True)
    planes, n = u0.shape
    assert n == ncol * R.NZ
    ld = n + 15
    buf = np.full((planes, ld), 7.0)
    buf[:, :n] = u0
    u_in, out, work = dev(cloudy, buf), dev(cloudy, blank(planes, ld)), dev(cloudy, blank(planes, ld))
    if entry == "steps":
        rc = L.cloudy_rainshaft_ssprk33_steps(p.handle, R.NZ, ncol, ld, u_in.ptr, out.ptr, R.DZ, R.COL_DT, R.COL_STEPS, None)
    else:
        rc = L.cloudy_rainshaft_rhs(p.handle, R.NZ, ncol, ld, u_in.ptr, R.DZ, work.ptr, out.ptr, None)
    assert rc == 0, (rc, L.cloudy_last_error().decode())
    got = [out.to_numpy()] + ([work.to_numpy()] if entry == "rhs" else [])
    assert all(np.all(is_blank(g[:, n:])) for g in got) and bits_equal(u_in.to_numpy(), buf)
    return [g[:, :n] for g in got]


@functools.lru_cache(maxsize=None)
def column_batch():
    """the bench's cfg3b batch stacked as NCOL columns of NZ cells, as test_degenerate_cells_with_the_source_on stacks it"""
    u0 = np.maximum(bench.make_workload("cfg3b", R.NZ * R.NCOL, seed=7)["mom"], 0.0)
    u0.setflags(write=False)
    return u0


@functools.lru_cache(maxsize=None)
def whole_columns(cloudy, entry):
    return run_columns(cloudy, entry, column_batch(), R.NCOL)


def columns(a, sel):
    """the columns `sel` (a slice or an index array) of planes stacked as columns, cells inside a column kept"""
    return np.ascontiguousarray(a.reshape(a.shape[0], -1, R.NZ)[:, sel, :].reshape(a.shape[0], -1))


@pytest.mark.parametrize("entry", COLUMN_ENTRIES)
def test_columns_reversed(gpu_cloudy, entry):
    """NCOL columns fill two workgroups and part of a third (test_ranked_fixed_host.test_column_count); reversing the order of the
    columns reverses the result bit for bit"""
    got = run_columns(gpu_cloudy, entry, columns(column_batch(), slice(None, None, -1)), R.NCOL)
    for b, g in zip(whole_columns(gpu_cloudy, entry), got):
        assert bits_equal(columns(b, slice(None, None, -1)), g)


@pytest.mark.parametrize("entry", COLUMN_ENTRIES)
def test_columns_alone(gpu_cloudy, entry):
    """the first three and the last three columns run alone have their bits"""
    for sel in (slice(0, 3), slice(R.NCOL - 3, R.NCOL)):
        got = run_columns(gpu_cloudy, entry, columns(column_batch(), sel), 3)
        for b, g in zip(whole_columns(gpu_cloudy, entry), got):
            assert bits_equal(columns(b, sel), g)


@pytest.mark.parametrize("entry", COLUMN_ENTRIES)
def test_columns_beside_zero_and_nan_columns(gpu_cloudy, entry):
    """every third column replaced, in turn by an all-zero and an all-NaN column: the other columns' bits are unchanged"""
    u = column_batch().copy().reshape(-1, R.NCOL, R.NZ)
    bad = np.arange(2, R.NCOL, 3)
    u[:, bad[0::2], :] = 0.0
    u[:, bad[1::2], :] = np.nan
    others = np.setdiff1d(np.arange(R.NCOL), bad)
    got = run_columns(gpu_cloudy, entry, np.ascontiguousarray(u.reshape(u.shape[0], -1)), R.NCOL)
    for b, g in zip(whole_columns(gpu_cloudy, entry), got):
        assert bits_equal(columns(b, others), columns(g, others))


# ---- 7. plane sums where the unrolled loop starts
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", R.SUM_SIZES)
def test_plane_sums_are_exact(gpu_cloudy, n, dtype):
    """cloudy_moment_sums of three planes of integers 1 .. 1021 in ld = n + 5 with a padding of 1e30 that no sum may read: the
    exact integer sums (every partial sum is an integer below 2^53: test_ranked_fixed_host.test_plane_sum_sizes), compared as
    Python ints, where an element dropped or counted twice at the boundary of the unrolled loop and its tail changes the sum."""
    cloudy = gpu_cloudy
    p = device_plan(cloudy, "fixed", dtype=0 if dtype == np.float64 else 1)
    ld = n + 5
    buf = np.full((R.SUM_PLANES, ld), 1e30, dtype=dtype)
    buf[:, :n] = R.sum_planes(n)
    x, sums = dev(cloudy, buf), dev(cloudy, blank(R.SUM_PLANES, 1))
    cloudy._lib.check(cloudy.lib().cloudy_moment_sums(p.handle, n, ld, R.SUM_PLANES, x.ptr, sums.ptr, None))
    got = sums.to_numpy().reshape(-1)
    assert np.isfinite(got).all() and np.all(got == np.floor(got))
    assert [int(v) for v in got] == R.exact_sums(n), (n, dtype)
