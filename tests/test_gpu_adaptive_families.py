"""GPU tests of the adaptive Tsit5 loop (tsit5_adaptive_loop, csrc/adaptive.hpp) on plan families beyond two Gamma modes: mixed
plane counts (a two-moment mode that is not the last), three to eight modes, Monodisperse and Lognormal closures, the ranked loop
with two to four ranked modes.  cloudy_tsit5_adaptive and cloudy_tsit5_adaptive_saveat run only the kernel compiled for the plan, so
the references are the NumPy restatement on the unchanged oracle's right-hand side, a fine fixed-step run, and the device itself
(bit equality).

Run with `-m gpu`.  Every family, batch, t_span and first step is chosen in tests/test_adaptive_families_host.py, on the oracle
alone, with the conditions this file relies on asserted there; ld = n + 15, out of place, sentinel-filled outputs.  The bounds are
the project's: F.TOL_EVAL x evaluations on the parcels with the restatement's (accepted, rejected), at most 5 % of parcels without,
2 x the restatement's error + 1e-12 against the fine run."""
import functools

import numpy as np
import pytest

import bench
import test_adaptive_families_host as F
import test_box_adaptive_host as B
import test_tsit5_adaptive_host as H
from gpu_support import adaptive, bits_equal, box_adaptive, is_blank, make_case, same_counts, saveat

pytestmark = pytest.mark.gpu

KEYS = ("u", "t", "dt", "accepted", "rejected", "status")
SAVEAT_IDS = F.SAVEAT_IDS
COAL, COND = 1, 2
# the bit-level tests need no reference: four_gamma_thr runs them at BS + 1 (a full workgroup of the ranked loop and a one-lane
# second one), where its fine fixed-step reference alone would take a third of the host file's time; its parity batch has 65 parcels
BITS_N = {"six_modes": None, "eight_gamma": None, "four_gamma_thr": F.BS + 1}


def new_plan(cloudy, oracle, fid, dtype=0):
    f = F.FAMILIES[fid]
    par, _, _ = make_case(cloudy, oracle, list(f["types"]), F.kernel_tensor(fid), f["thr"], bench.NORMS, moving=f["moving"])
    return par.coal_data.plan(list(f["types"]), dtype=dtype)


plan_of = functools.lru_cache(maxsize=None)(new_plan)   # one plan per (family, dtype) and session


@functools.lru_cache(maxsize=None)
def device_run(cloudy, oracle, fid, warm=True):
    """cloudy_tsit5_adaptive on the family's batch, once per session; warm = False: every first step automatic (dt_dev of zeros)"""
    u0, dt = F.batch(fid)
    return adaptive(cloudy, plan_of(cloudy, oracle, fid), u0, F.FAMILIES[fid]["t_span"], ld=u0.shape[1] + 15, dt_in=dt if warm else "zeros")


def assert_same_bits(a, b, flip=False):
    for k in KEYS:
        assert bits_equal(a[k], b[k][..., ::-1] if flip else b[k]), k


# ---- 1. decision parity
@pytest.mark.parametrize("fid", F.IDS)
def test_decision_parity(gpu_cloudy, oracle, fid):
    """The assertions of test_gpu_tsit5_adaptive.decision_parity on every family: status 0 and t == t_span bit for bit; at most 5 %
    of the parcels differ from the restatement in (accepted, rejected); the others agree to F.TOL_EVAL x the evaluations the parcel
    took, of |u0| + |want| per plane; every parcel agrees with the fine fixed-step run to 2 x the restatement's error + 1e-12; padding
    columns and input untouched."""
    u0, _ = F.batch(fid)
    n, t_span = u0.shape[1], F.FAMILIES[fid]["t_span"]
    got, ref, fine = device_run(gpu_cloudy, oracle, fid), F.reference(fid), F.fine_reference(fid)
    assert np.all(got["status"] == 0) and np.all(got["t"] == t_span)
    same = same_counts(got, ref)
    rel = np.abs(got["u"] - ref["u"]) / np.maximum(np.abs(u0) + np.abs(ref["u"]), 1e-300) / ref["evals"]
    worst = rel[:, same].max()
    ref_err, err = H.plane_errors(ref["u"], fine, u0), H.plane_errors(got["u"], fine, u0)
    print(f"{fid} n={n}: {(~same).sum()} of {n} parcels differ in (accepted, rejected) {np.flatnonzero(~same)}; the others agree to "
          f"{worst:.2e} x evaluations (worst parcel {int(rel[:, same].max(axis=0).argmax())}); against the fine fixed-step run: "
          f"restatement {ref_err.max():.2e}, device {err.max():.2e}")
    assert (~same).sum() <= 0.05 * n, (~same).sum()
    assert np.all(err <= 2 * ref_err + 1e-12), (err, ref_err)
    assert worst <= F.TOL_EVAL[F.all_inf(fid)], worst
    assert got["pad"].shape == (u0.shape[0], 15) and np.all(is_blank(got["pad"])) and bits_equal(got["u_in"], got["buf"])


# ---- 2. snapshots
saveat_times = F.saveat_times


@pytest.mark.parametrize("fid", SAVEAT_IDS)
def test_snapshots(gpu_cloudy, oracle, fid):
    """u, dt, t and the counts have the bits of the plain call; every snapshot of the parcels with the restatement's counts is within
    F.TOL_EVAL x evaluations of the restatement's at the save times the restatement resolves (F.SNAPSHOTS_RESOLVED, asserted on the
    host: among them the input, the one inside the first step, an interpolated one, 0.999 t_span and t_span), and printed at the
    others; snapshot 0 has the bits of u_in, the one at t_span those of u_out; u_save has exactly n_save x sum(np)
    planes: the plane behind it and the tail of every plane keep their sentinel (a two-moment mode writing a third plane would land in the next mode's number plane or, for the last snapshot, in the guard)."""
    cloudy = gpu_cloudy
    u0, _ = F.batch(fid)
    t_span = F.FAMILIES[fid]["t_span"]
    times = saveat_times(t_span)
    got = saveat(cloudy, plan_of(cloudy, oracle, fid), u0, t_span, times, ld=u0.shape[1] + 15)
    assert_same_bits(got, device_run(cloudy, oracle, fid, warm=False))
    ref = F.reference(fid, saveat=tuple(times), warm=False)
    assert np.all(got["status"] == 0) and np.all(ref["status"] == 0) and np.isfinite(ref["saved"]).all()
    same = same_counts(got, ref)
    rel = np.abs(got["saved"] - ref["saved"]) / np.maximum(np.abs(u0)[None] + np.abs(ref["saved"]), 1e-300) / ref["evals"][None, None, :]
    worst = rel[:, :, same].max(axis=(1, 2))
    print(f"{fid}: {(~same).sum()} of {same.size} parcels differ in (accepted, rejected); the snapshots of the others agree to "
          f"{worst.max():.2e} x evaluations (per save time: {worst})")
    assert (~same).sum() <= 0.05 * same.size
    assert got["saved"].shape == (len(times), sum(F.nprog(fid)), u0.shape[1])
    assert bits_equal(got["saved"][0], u0) and bits_equal(got["saved"][-1], got["u"])
    assert np.all(is_blank(got["guard"])) and np.all(is_blank(got["saved_pad"])) and np.all(is_blank(got["pad"]))
    assert bits_equal(got["u_in"], got["buf"])
    assert worst[list(F.SNAPSHOTS_RESOLVED[fid])].max() <= F.TOL_EVAL[F.all_inf(fid)], worst


@pytest.mark.parametrize("fid", SAVEAT_IDS)
def test_snapshots_under_a_budget(gpu_cloudy, oracle, fid):
    """max_steps = 3: the restatement's status per parcel; a parcel that stopped early has NaN in every plane of every snapshot
    beyond the time it reached and finite values before; guard plane and tails untouched."""
    cloudy = gpu_cloudy
    u0, _ = F.batch(fid)
    t_span = F.FAMILIES[fid]["t_span"]
    times = saveat_times(t_span)
    got = saveat(cloudy, plan_of(cloudy, oracle, fid), u0, t_span, times, ld=u0.shape[1] + 15, max_steps=3)
    ref = F.reference(fid, max_steps=3, saveat=tuple(times), warm=False)
    slow = ref["status"] == 1
    assert slow.sum() >= 3 and np.array_equal(got["status"], ref["status"])
    beyond = times[:, None] > got["t"][None, :]
    assert beyond[:, slow].any() and not beyond[:, ~slow].any()
    assert np.all(np.isnan(got["saved"]).all(axis=1) == beyond) and np.all(np.isfinite(got["saved"]).all(axis=1) == ~beyond)
    assert np.all(is_blank(got["guard"])) and np.all(is_blank(got["saved_pad"]))


# ---- 3. the box entry point
@pytest.mark.parametrize("fid", tuple(F.BOX_N))
def test_box_decision_parity_and_xi_zero(gpu_cloudy, oracle, fid):
    """cloudy_box_tsit5_adaptive with COAL | COND, a supersaturation per parcel through s_dev, at BS + 1 of the box kernel (257; 513 on
    the three-mode thresholded plan): status 0 and t == t_span; at most 5 % of the parcels differ from the restatement on
    rhs_coal_batch + rhs_condensation_batch in (accepted, rejected); the others agree to B.TOL_EVAL x evaluations (the bound of
    test_gpu_box_adaptive.test_decision_parity); padding and input untouched.  With xi = 0 the call has the bits of
    cloudy_tsit5_adaptive."""
    cloudy = gpu_cloudy
    n, t_span = F.BOX_N[fid], F.FAMILIES[fid]["t_span"]
    u0, dt = F.batch(fid, n=n)
    s, plan = B.box_supersaturation(n), plan_of(cloudy, oracle, fid)
    got = box_adaptive(cloudy, plan, u0, t_span, s, F.BOX_XI[fid], sources=COAL | COND, ld=n + 15, dt_in=dt)
    ref = F.box_reference(fid)
    assert np.all(got["status"] == 0) and np.all(got["t"] == t_span)
    same = same_counts(got, ref)
    rel = np.abs(got["u"] - ref["u"]) / np.maximum(np.abs(u0) + np.abs(ref["u"]), 1e-300) / ref["evals"]
    worst = rel[:, same].max()
    print(f"box {fid} n={n}: {(~same).sum()} of {n} parcels differ in (accepted, rejected); the others agree to {worst:.2e} x evaluations")
    assert (~same).sum() <= 0.05 * n, (~same).sum()
    assert worst <= B.TOL_EVAL, worst
    assert np.all(is_blank(got["pad"])) and bits_equal(got["u_in"], got["buf"])
    plain = adaptive(cloudy, plan, u0, t_span, ld=n + 15, dt_in=dt)
    assert_same_bits(plain, box_adaptive(cloudy, plan, u0, t_span, s, 0.0, sources=COAL | COND, ld=n + 15, dt_in=dt))
    assert not bits_equal(plain["u"], got["u"])


# ---- 4. bit-level properties that need no reference
@pytest.mark.parametrize("fid", ["six_modes", "eight_gamma", "four_gamma_thr"])
def test_same_bits_again_in_place_and_reversed(gpu_cloudy, oracle, fid):
    """Many-mode kernels (eight [N][3] arrays per lane: accumulation registers and scratch): the same call three times and once on a
    fresh plan gives the same bits in u, dt, t and info (the guard DESIGN 3.7 (viii) put on the converged kernel); in place equals
    out of place; the batch reversed gives each parcel the bits it had (lane, wave, workgroup and, where the parcels are ranked,
    the ranking)."""
    cloudy = gpu_cloudy
    u0, dt = F.batch(fid, n=BITS_N[fid])
    n, t_span = u0.shape[1], F.FAMILIES[fid]["t_span"]
    plan = plan_of(cloudy, oracle, fid)
    base = adaptive(cloudy, plan, u0, t_span, ld=n + 15, dt_in=dt)
    assert np.all(base["status"] == 0) and (base["accepted"] + base["rejected"]).max() >= 5
    for _ in range(2):
        assert_same_bits(base, adaptive(cloudy, plan, u0, t_span, ld=n + 15, dt_in=dt))
    assert_same_bits(base, adaptive(cloudy, new_plan(cloudy, oracle, fid), u0, t_span, ld=n + 15, dt_in=dt))
    assert_same_bits(base, adaptive(cloudy, plan, u0, t_span, ld=n + 15, dt_in=dt, in_place=True))
    assert_same_bits(base, adaptive(cloudy, plan, np.ascontiguousarray(u0[:, ::-1]), t_span, ld=n + 15, dt_in=dt[::-1].copy()), flip=True)


@pytest.mark.parametrize("fid", ["exp_gamma", "gamma_exp_gamma_thr"])
def test_float_planes(gpu_cloudy, oracle, fid):
    """test_gpu_tsit5_adaptive.test_float_planes on mixed plane counts: a CLOUDY_F32 plan from float-rounded input against the fp64
    plan from the same rounded input -- equal counts, the output the fp64 result rounded once (2^-24 relative)."""
    cloudy = gpu_cloudy
    u0, dt = F.batch(fid)
    u32 = u0.astype(np.float32)
    n, t_span = u0.shape[1], F.FAMILIES[fid]["t_span"]
    want = adaptive(cloudy, plan_of(cloudy, oracle, fid), u32.astype(np.float64), t_span, ld=n + 15, dt_in=dt)
    got = adaptive(cloudy, plan_of(cloudy, oracle, fid, 1), u32, t_span, ld=n + 15, dt_in=dt)
    assert got["u"].dtype == np.float32 and np.all(got["status"] == 0)
    assert np.array_equal(got["accepted"], want["accepted"]) and np.array_equal(got["rejected"], want["rejected"])
    fin = np.isfinite(want["u"].astype(np.float32))
    err = np.abs(got["u"].astype(np.float64) - want["u"])[fin] / np.abs(want["u"])[fin]
    print(f"float planes, {fid}: max relative difference {err.max():.2e}")
    assert err.max() <= 2.0 ** -24, err.max()


@pytest.mark.parametrize("fid", ["exp_gamma", "six_modes"])
def test_zero_t_span_copies_every_plane(gpu_cloudy, oracle, fid):
    cloudy = gpu_cloudy
    u0, dt = F.batch(fid)
    zero = adaptive(cloudy, plan_of(cloudy, oracle, fid), u0, 0.0, ld=u0.shape[1] + 15, dt_in=dt)
    assert bits_equal(zero["u"], u0) and np.all(zero["t"] == 0) and np.all(is_blank(zero["pad"]))
    assert not zero["accepted"].any() and not zero["rejected"].any() and not zero["status"].any()


# ---- 5. the relaxed dtype
def test_f64_relaxed_on_four_ranked_modes(gpu_cloudy, oracle):
    """CLOUDY_F64_RELAXED on four_gamma_thr: status 0 everywhere, and on the parcels with the fp64 run's counts the result is within
    1e-9 (what test_f64_relaxed_dtype_error_report allows the relaxed right-hand side per evaluation) x evaluations of the fp64 run's,
    of |u0| + |u| per plane."""
    cloudy = gpu_cloudy
    fid = "four_gamma_thr"
    u0, dt = F.batch(fid, n=BITS_N[fid])
    want = adaptive(cloudy, plan_of(cloudy, oracle, fid), u0, F.FAMILIES[fid]["t_span"], ld=u0.shape[1] + 15, dt_in=dt)
    got = adaptive(cloudy, plan_of(cloudy, oracle, fid, cloudy.F64_RELAXED), u0, F.FAMILIES[fid]["t_span"], ld=u0.shape[1] + 15, dt_in=dt)
    assert np.all(got["status"] == 0) and np.all(got["t"] == F.FAMILIES[fid]["t_span"])
    same = same_counts(got, want)
    evals = 1 + 6 * (want["accepted"] + want["rejected"])
    rel = np.abs(got["u"] - want["u"]) / np.maximum(np.abs(u0) + np.abs(want["u"]), 1e-300) / evals
    print(f"CLOUDY_F64_RELAXED {fid}: {(~same).sum()} parcels differ in counts; the others within {rel[:, same].max():.2e} x evaluations")
    assert (~same).sum() <= 0.05 * same.size
    assert rel[:, same].max() <= 1e-9, rel[:, same].max()
