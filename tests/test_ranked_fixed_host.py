"""CPU-only half of the tests of the RANKED FIXED-STEP kernels: cloudy_coal_rhs, cloudy_ssprk33_steps, cloudy_tsit5_steps,
cloudy_box_ssprk33_steps (COAL | COND), cloudy_rainshaft_sources and the column integrator on plans with a finite or moving
threshold, where every right-hand-side evaluation ranks the workgroup's parcels through LDS (regime_rank, coal_ints_ranked_impl,
coal_rhs_sorted_body.inc), and of the unrolled loop of plane_partial_sums_kernel.  Every input of tests/test_gpu_ranked_fixed.py is
chosen here, on the oracle alone, and every condition the GPU file relies on is asserted here:

  * the batches (PLANS, SEED), the step (DT, N_STEPS: the 1e-3 s and 2 steps of the fused-stepping tests of cfg3b and moving4,
    test_fused_integrators_two_moment_mode_partial_workgroup_and_padding, test_cfg0_single_box_tsit5_fixed_step,
    test_tsit5_serves_every_plan_family_ssprk33_serves; cfg4, which none of them steps: 1e-7 s, see DT) and that the oracle
    stepping leaves >= 90 % of the 1025 parcels regular and resolved by the oracle itself (regular(), resolved());
  * the hostile batch (hostile_batch) and what the oracle makes of each role (nan_modes);
  * the parcels run alone (singletons) and that the extreme ranking keys fall in different buckets of regime_bucket;
  * the number of columns of the column test, from the workgroup size jit_rainshaft_part picks (restated from csrc/jit.hpp);
  * the sizes of the plane sums around the start of the unrolled loop, from kSumBlocks and kBlock read as text.

The `fixed` plan is the bench's cfg3b as bench.workload_spec defines it: thresholds (5e-10, Inf)."""
import functools
import os
import re

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cloudy.jl_amd", "csrc")

PLANS = {"fixed": "cfg3b", "two_thr": "cfg4", "moving": "moving4"}
STEPPERS = ("ssprk33", "tsit5", "box")
SIZES = (257, 513, 1025)     # a full workgroup + one lane, and the same past two and four: for 256 and 512 threads alike
N = SIZES[-1]
# fixed, moving: the step of the fused-stepping tests of cfg3b and moving4.  No such test steps cfg4, whose fitted hydrodynamic
# tensor is stiff on the bench's batch: on the oracle alone, 2 steps of 1e-3 / 1e-4 / 1e-5 / 1e-6 s leave 776 / 834 / 880 / 919 of
# 1025 parcels regular under Tsit5 (791 / 845 / 891 / 934 under SSPRK33), 1e-7 s leaves 972 (977): the largest power of ten that
# meets the 90 % under both schemes
DT = {"fixed": 1e-3, "two_thr": 1e-7, "moving": 1e-3}
N_STEPS = 2
RESOLVED = 1e-10             # a tenth of the 1e-9 of |u0| + |u| the steppers are held to (resolved())
XI = 1e-8                    # test_gpu_box_sources.XI
VEL = ((50.0, 1.0 / 6),)     # test_sedimentation_flux_kat_and_rainshaft_sources
# seeds of bench.synth_moments per plan, picked so that the oracle stepping of every stepper leaves >= 90 % regular parcels
# (test_regular_parcels asserts it and prints the counts)
SEED = {"fixed": 31, "two_thr": 31, "moving": 31}
ROLES = ("zero", "nan", "inf", "negative", "dense")
WINDOWS = ((0, 65), (224, 289), (480, 545), (N - 65, N), (0, 257), (0, 513))
# the column test: nz cells per column, the cfg3b batch stacked as columns
NZ, DZ, COL_DT, COL_STEPS = 20, 150.0, 1e-3, 2   # (dz, dt: test_workgroup_size_of_the_column_integrator_changes_no_bit)
COL_BLOCK = 512              # what jit_rainshaft_part picks for two modes, a threshold, 20 cells (test_column_count)
NCOL = 2 * (COL_BLOCK // NZ) + 7   # two workgroups of 25 columns and 7 columns of a third
# cloudy_moment_sums
SUM_PLANES = 3
SUM_SIZES = (786_431, 786_432, 786_433, 1_048_575, 1_048_576, 1_048_577, 1_310_723, 4_194_309)


def n_modes(plan):
    return bench.workload_spec(PLANS[plan])["n_modes"]


def is_moving(plan):
    return bool(bench.workload_spec(PLANS[plan]).get("moving"))


def supersaturation(n):
    """test_gpu_box_sources.supersaturation"""
    return np.random.default_rng(0).uniform(-0.02, 0.05, n)


def hostile_batch(u0, s):
    """every fourth parcel kept; the others replaced in rotation by an all-zero parcel, an all-NaN parcel, a parcel with +Inf in
    M2 of the first mode, a parcel with M0 < 0 in the first mode, and a copy of the parcel with the largest M0 (its
    supersaturation with it) -> (batch, s, role per parcel: -1 kept, else index into ROLES)"""
    u, s = u0.copy(), s.copy()
    n = u0.shape[1]
    role = np.full(n, -1)
    replaced = np.flatnonzero(np.arange(n) % 4 != 0)
    role[replaced] = np.arange(replaced.size) % len(ROLES)
    dense = int(np.argmax(u0[0]))
    u[:, role == 0] = 0.0
    u[:, role == 1] = np.nan
    u[2, role == 2] = np.inf
    u[0, role == 3] = -np.maximum(u0[0, role == 3], 1.0)   # (an empty mode of the batch has M0 = 0)
    u[:, role == 4] = u0[:, [dense]]
    s[role == 4] = s[dense]
    return u, s, role


@functools.lru_cache(maxsize=None)
def batch(plan, hostile=False):
    """-> (u0 (3 modes x 3, N), s (N,), role): the bench's synthetic batch of the plan and a supersaturation per parcel (read by
    `box` alone); shared, read-only"""
    u0 = bench.synth_moments(n_modes(plan), N, SEED[plan])
    s = supersaturation(N)
    role = np.full(N, -1)
    if hostile:
        u0, s, role = hostile_batch(u0, s)
    for a in (u0, s, role):
        a.setflags(write=False)
    return u0, s, role


def oracle_rhs(oracle, plan, stepper, s):
    op = bench.oracle_params(PLANS[plan])
    if stepper == "box":
        return lambda u: oracle.rhs_coal_batch(op, u) + oracle.rhs_condensation_batch(op, XI, s, u)
    return lambda u: oracle.rhs_coal_batch(op, u)


@functools.lru_cache(maxsize=None)
def stepping_reference(plan, stepper):
    """the scheme of `stepper` driven by the oracle's right-hand side on the clean batch, once per session -> (end state, regular and resolved)"""
    from oracle import cloudy_oracle as oracle
    from gpu_support import _ssprk33_host, _tsit5_host, oracle_reference

    u0, s, _ = batch(plan)
    with np.errstate(all="ignore"):
        if stepper == "box":   # the restatement of test_gpu_box_sources.py
            want = oracle_reference(oracle, bench.oracle_params(PLANS[plan]), u0, DT[plan], N_STEPS, XI, s, True, True)
        else:
            host = _tsit5_host if stepper == "tsit5" else _ssprk33_host
            want = host(oracle_rhs(oracle, plan, stepper, s), u0, DT[plan], N_STEPS)
    want.setflags(write=False)
    return want, regular(oracle, plan, u0, want) & resolved(oracle, plan, stepper, u0, s, want)


def regular(oracle, plan, u0, want):
    """The criterion of the existing stepping tests of these plans: finite and within a factor 10 of the initial state in the
    first mode (test_fused_ssprk33_batch_vs_oracle_stepping), and no mode on a clamp of its shape, where one ulp of a stage
    state decides between k = 10 and k = eps and the device forms the stage states with FMAs
    (test_cfg0_single_box_tsit5_fixed_step, test_tsit5_serves_every_plan_family_ssprk33_serves)."""
    prm = oracle.update_dist_batch(bench.oracle_params(PLANS[plan]), u0)
    with np.errstate(all="ignore"):
        ok = np.isfinite(want).all(axis=0) & (np.abs(want[:3]) <= 10 * np.abs(u0[:3]) + 1e-300).all(axis=0)
        for mode in range(n_modes(plan)):
            ok &= (prm[3 * mode + 2] > 1e-3) & (prm[3 * mode + 2] < 9.999)
    return ok


def resolved(oracle, plan, stepper, u0, s, want):
    """The reference's own resolution, as test_five_gamma_modes_beyond_the_ahead_of_time_families takes it: the parcels whose
    oracle end state moves by at most RESOLVED of |u0| + |u| when M2 of every mode of the input moves by one ulp, either way.
    Where it moves by more, the oracle stepping is no reference at the 1e-9 the device is held to: parcel 417 of the `moving`
    batch keeps its first mode within 10 % under Tsit5 -- regular by the criterion above -- while its second and third modes
    leave the stability region (moments of -3e24 .. 3e39 from 1e-17 .. 1e-3), and its oracle end state moves by 8e-3."""
    from gpu_support import _ssprk33_host, _tsit5_host

    host = _tsit5_host if stepper == "tsit5" else _ssprk33_host
    ref = np.maximum(np.abs(u0) + np.abs(want), 1e-300)
    ok = np.ones(u0.shape[1], bool)
    for toward in (np.inf, -np.inf):
        nudged = u0.copy()
        nudged[2::3] = np.nextafter(u0[2::3], toward)
        with np.errstate(all="ignore"):
            moved = np.abs(host(oracle_rhs(oracle, plan, stepper, s), nudged, DT[plan], N_STEPS) - want) / ref
        ok &= (moved <= RESOLVED).all(axis=0)   # (a NaN compares false)
    return ok


def ranking_key(oracle, plan, u0):
    """the key coal_rhs_sorted_body.inc ranks the first thresholded mode (mode 0 of every plan here) by, from the oracle's closure
    inversion: thr / theta (normalised) on fixed thresholds, k on moving ones -> (key as the kernel's float, valid)"""
    prm = oracle.update_dist_batch(bench.oracle_params(PLANS[plan]), u0)
    nn, th, kk = prm[0], prm[1], prm[2]
    with np.errstate(all="ignore"):
        if is_moving(plan):
            key = kk.astype(np.float32)
        else:
            thr = bench.workload_spec(PLANS[plan])["thresholds"][0] / bench.NORMS[1]
            key = (thr / th).astype(np.float32)
    return key, (nn > 0.0) & ~np.isnan(key)


def regime_bucket(key, bs):
    """kernels.hpp, regime_bucket<BS>: eight logarithmic buckets per binade from 2^-8 up, read off the float's exponent and top
    three mantissa bits: code = (bits(max(key, 0)) >> 20) - (127 - 8) * 8, clamped to [0, BS - 2]"""
    bits = np.maximum(np.asarray(key, dtype=np.float32), np.float32(0.0)).view(np.uint32)
    code = (bits >> 20).astype(np.int64) - (127 - 8) * 8
    return np.clip(code, 0, bs - 2)


def singletons(oracle, plan):
    """at most 12 parcels to run alone: the corners of the 256- and 512-thread workgroups, the last parcel, and the valid parcels
    with the smallest and the largest ranking key -> (sorted picks, parcel of the smallest key, of the largest)"""
    key, valid = ranking_key(oracle, plan, batch(plan)[0])
    idx = np.flatnonzero(valid)
    lo, hi = int(idx[np.argmin(key[idx])]), int(idx[np.argmax(key[idx])])
    return sorted({0, 255, 256, 511, 512, N - 1, lo, hi}), lo, hi


def nan_modes(oracle, plan, sources=False):
    """role -> the modes whose shape parameter the oracle's closure inversion returns as NaN for EVERY parcel of that role in
    the hostile batch (sources: of the clamped batch, as the rainshaft body clamps first): the only thing the GPU test asserts
    of the nan, inf and negative roles is that those modes' tendencies are NaN (test_error_behaviour_on_device)"""
    u0, _, role = batch(plan, hostile=True)
    x = np.maximum(u0, 0.0) if sources else u0
    with np.errstate(all="ignore"):
        prm = oracle.update_dist_batch(bench.oracle_params(PLANS[plan]), x)
    return {r: [m for m in range(n_modes(plan)) if np.isnan(prm[3 * m + 2][role == r]).all()] for r in (1, 2, 3)}


def sum_planes(n):
    """x[q, i] = (i (q + 1)) % 1021 + 1: integers, exact as float and as double, whose sums add exactly in fp64 in any order"""
    i = np.arange(n, dtype=np.int64)
    return np.stack([(i * (q + 1)) % 1021 + 1 for q in range(SUM_PLANES)])


def exact_sums(n):
    return [int(v) for v in sum_planes(n).sum(axis=1)]


# ---- 1. regular parcels
@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("stepper", STEPPERS)
def test_regular_parcels(oracle, plan, stepper):
    """A condition on the inputs: the oracle-driven stepping leaves at least 90 % of the 1025 parcels regular and resolved."""
    want, ok = stepping_reference(plan, stepper)
    print(f"{plan} {stepper}: {int(ok.sum())} regular parcels of {N}")
    assert want.shape == batch(plan)[0].shape and ok.sum() >= 0.9 * N, ok.sum()


# ---- 2. the hostile batch
@pytest.mark.parametrize("plan", list(PLANS))
def test_hostile_batch_on_the_oracle(oracle, plan):
    """The oracle returns on the hostile batch; on the kept parcels and on the copies of the densest parcel it gives what it
    gives on the clean batch (the restatement is per parcel); its all-zero parcel is finite (zero).  Printed: the modes with a NaN
    shape per role, which is all the GPU test asserts of the bad roles -- none on these batches: a NaN or negative M0 or M1 fails the
    `> eps` guard and selects the fallback distribution as in the reference, and +Inf in M2 gives k = 0, clamped."""
    u0, s, _ = batch(plan)
    h0, hs, role = batch(plan, hostile=True)
    assert np.array_equal(role == -1, np.arange(N) % 4 == 0) and all((role == r).sum() >= N // 8 for r in range(len(ROLES)))
    dense = int(np.argmax(u0[0]))
    assert np.all(h0[0, role == 3] < 0.0) and np.all(np.isposinf(h0[2, role == 2])) and np.all(hs[role == 4] == s[dense])
    op = bench.oracle_params(PLANS[plan])
    with np.errstate(all="ignore"):
        clean, bad = oracle.rhs_coal_batch(op, u0), oracle.rhs_coal_batch(op, h0)
        clean_c, bad_c = oracle.rhs_condensation_batch(op, XI, s, u0), oracle.rhs_condensation_batch(op, XI, hs, h0)
    kept = role == -1
    assert np.array_equal(clean[:, kept], bad[:, kept], equal_nan=True) and np.array_equal(clean_c[:, kept], bad_c[:, kept], equal_nan=True)
    for got, ref in ((bad, clean), (bad_c, clean_c)):
        lanes = got[:, role == 4]
        assert np.array_equal(lanes, np.repeat(ref[:, [dense]], lanes.shape[1], axis=1), equal_nan=True)
        assert not got[:, role == 0].any()
    modes = nan_modes(oracle, plan)
    print(f"{plan}: modes with a NaN shape per role: " + ", ".join(f"{ROLES[r]} {modes[r]}" for r in modes))
    for r, ms in modes.items():    # the contract itself, on the oracle: a mode whose shape is NaN has NaN tendencies
        for m in ms:
            assert np.isnan(bad[3 * m:3 * m + 3][:, role == r]).all(), (ROLES[r], m)
    if plan == "fixed":            # the cell body of cloudy_rainshaft_sources clamps first
        vop = bench_oracle_params_with_velocity()
        with np.errstate(all="ignore"):
            cs_clean, sf_clean = oracle.rainshaft_cell_batch(vop, u0)
            cs, sf = oracle.rainshaft_cell_batch(vop, h0)
        assert np.array_equal(cs[:, kept], cs_clean[:, kept], equal_nan=True) and np.array_equal(sf[:, kept], sf_clean[:, kept], equal_nan=True)
        assert not cs[:, role == 0].any() and np.isfinite(sf[:, role == 0]).all()
        smodes = nan_modes(oracle, plan, sources=True)
        print(f"{plan} sources: modes with a NaN shape per role: " + ", ".join(f"{ROLES[r]} {smodes[r]}" for r in smodes))
        for r, ms in smodes.items():
            for m in ms:
                assert np.isnan(cs[3 * m:3 * m + 3][:, role == r]).all(), (ROLES[r], m)


def bench_oracle_params_with_velocity():
    """bench.oracle_params("cfg3b") with the velocity of test_sedimentation_flux_kat_and_rainshaft_sources"""
    from oracle import cloudy_oracle as O

    spec = bench.workload_spec("cfg3b")
    return O.make_params([O.GAMMA] * 2, bench.kernel_matrix(spec), spec["thresholds"], norms=bench.NORMS, vel=VEL)


# ---- 3. the parcels run alone
@pytest.mark.parametrize("plan", list(PLANS))
def test_singleton_picks(oracle, plan):
    picked, lo, hi = singletons(oracle, plan)
    key, valid = ranking_key(oracle, plan, batch(plan)[0])
    assert len(picked) <= 12 and len(set(picked)) == len(picked) and {0, 255, 256, 511, 512, N - 1, lo, hi} == set(picked)
    assert valid[lo] and valid[hi] and valid.sum() >= 0.9 * N
    for bs in (256, 512):
        b = regime_bucket(key, bs)
        print(f"{plan}: keys {key[lo]:.3g} (parcel {lo}) .. {key[hi]:.3g} (parcel {hi}); buckets {b[lo]} .. {b[hi]} of {bs}; "
              f"{np.unique(b[valid]).size} buckets in use")
        assert b[lo] != b[hi] and np.all((b >= 0) & (b <= bs - 2))
    # the formula itself: eight buckets per binade, bucket 0 up to 2^-8, the last one for everything from 2^24 on (BS = 256)
    assert list(regime_bucket([0.0, 2.0 ** -9, 2.0 ** -8, 1.0, 1.125, 2.0, 2.0 ** 24, np.inf, -1.0], 256)) == \
        [0, 0, 0, 64, 65, 72, 254, 254, 0]
    text = open(os.path.join(CSRC, "kernels.hpp")).read()
    assert "const int code = (int)(__float_as_uint(fmaxf(key, 0.0f)) >> 20) - (127 - 8) * 8;" in text
    assert "return code < 0 ? 0 : (code > BS - 2 ? BS - 2 : code);" in text


# ---- 4. the columns
def test_column_count():
    """jit_rainshaft_part (csrc/jit.hpp: the shared rule jit_column_part on jit_rainshaft_fits) restated for the column test's plan
    -- cfg3b: two modes, a threshold -- and nz = 20: more columns than a 256-thread workgroup holds, so the pick is the size with
    the smallest time per cell among those whose LDS fits, full[i] * bs / ((bs / nz) * nz).  NCOL fills two workgroups of that size
    and part of a third."""
    jit = open(os.path.join(CSRC, "jit.hpp")).read()
    start = jit.index("inline int jit_column_part(")
    body = jit[start:jit.index("\n}\n", start)]
    sizes = [int(v) for v in re.search(r"static const int sizes\[3\] = \{(\d+), (\d+), (\d+)\};", body).groups()]
    full = [float(v) for v in re.search(r"const double full\[3\] = \{([\d.]+), ([\d.]+), ([\d.]+)\};", body).groups()]
    assert "if (nz <= 256 && n_columns <= 256 / nz && fits(256)) {" in body
    assert "const double t = full[i] * double(bs) / double((bs / nz) * nz);" in body
    caller = jit[jit.index("inline int jit_rainshaft_part("):]
    assert "return jit_column_part(nz, n_columns, [&](int bs) { return jit_rainshaft_fits(h, bs, nz); });" in caller[:caller.index("\n}\n")]
    assert "return (size_t)bs >= nz && jit_rainshaft_lds_bytes(h, bs) <= kLdsPerWorkgroup;" in jit
    limit = int(re.search(r"constexpr size_t kLdsPerWorkgroup = (\d+);", jit).group(1))

    def lds_bytes(n_modes, bs):   # jit_rainshaft_lds_bytes of a thresholded plan
        row = bs * 8
        used = 3 * n_modes * row + (3 * n_modes + 3 * max(n_modes - 1, 1)) * row + bs * 6
        budget = 40960 * (bs // 256)
        if budget > used:
            used += min((budget - used) // row, 3 * n_modes) * row
        return used + bs + 4 * (bs // 64) + 64

    lds = jit[jit.index("inline size_t jit_rainshaft_lds_bytes("):jit.index("constexpr size_t kLdsPerWorkgroup")]
    for line in ("size_t used = 3 * N * row;", "used += (3 * N + 3 * (N > 1 ? N - 1 : 1)) * row + (size_t)bs * 6;",
                 "const size_t budget = (size_t)40960 * ((size_t)bs / 256);",
                 "if (budget > used) used += std::min((budget - used) / row, 3 * N) * row;",
                 "used += (size_t)bs + 4 * ((size_t)bs / 64);", "return used + 64;"):
        assert line in lds, line
    assert NCOL > 256 // NZ
    fits = [bs for bs in sizes if bs >= NZ and lds_bytes(2, bs) <= limit]
    assert fits == sizes
    times = {bs: full[i] * bs / ((bs // NZ) * NZ) for i, bs in enumerate(sizes)}
    pick = min(times, key=times.get)
    per = pick // NZ
    print(f"column workgroup size for two modes, nz = {NZ}: {pick} ({per} columns per workgroup); {NCOL} columns")
    assert pick == COL_BLOCK and 2 * per < NCOL < 3 * per and NCOL % 3 == 0


# ---- 5. the plane sums
def test_plane_sum_sizes():
    """The unrolled loop of plane_partial_sums_kernel runs for a lane while i + 3 stride < n, stride = gridDim.x kBlock, and the
    grid is capped at kSumBlocks workgroups: some lane enters it exactly when n > 3 kSumBlocks kBlock.  The sizes bracket that
    point, one whole trip of every lane (4 strides) and four (16 strides) with a tail; every partial sum is an integer below 2^53."""
    k_block = int(re.search(r"constexpr int kBlock = (\d+);", open(os.path.join(CSRC, "kernels.hpp")).read()).group(1))
    hip = open(os.path.join(CSRC, "cloudy_hip.hip")).read()
    k_sum = int(re.search(r"constexpr int kSumBlocks = (\d+);", hip).group(1))
    assert "if (blocks > (size_t)kSumBlocks) blocks = kSumBlocks;" in hip
    red = open(os.path.join(CSRC, "reduce_kernels.hpp")).read()
    assert "for (; i + 3 * stride < n; i += 4 * stride) {" in red and "const size_t stride = (size_t)gridDim.x * kBlock;" in red
    stride = k_sum * k_block
    assert 3 * stride == 786_432
    enters = {786_431: False, 786_432: False, 786_433: True, 1_048_575: True, 1_048_576: True, 1_048_577: True, 1_310_723: True,
              4_194_309: True}
    assert tuple(enters) == SUM_SIZES
    for n, want in enters.items():
        assert (n > 3 * stride) == want and (n + k_block - 1) // k_block >= k_sum   # (the grid is at its cap for every size)
    assert 1_048_576 == 4 * stride and 4_194_309 == 16 * stride + 5 and 1_310_723 == 5 * stride + 3
    for n in SUM_SIZES:
        x = sum_planes(n)
        assert x.min() >= 1 and x.max() <= 1021 and np.array_equal(x.astype(np.float32).astype(np.int64), x)
        assert all(0 < v < 2 ** 53 for v in exact_sums(n)) and n * 1021 < 2 ** 53
