"""GPU tests of the RANKED adaptive Tsit5 kernels (tsit5_adaptive_loop<RANKED = true>, csrc/adaptive.hpp): cloudy_tsit5_adaptive,
cloudy_tsit5_adaptive_saveat and cloudy_box_tsit5_adaptive (COAL | COND, with and without snapshots) on the two-Gamma plans with
fixed (5e-9, Inf) and moving (0.9, 1.0) thresholds, where every right-hand-side evaluation re-ranks the workgroup through LDS and a
finished or absent lane sits through the barriers.  kernels.hpp says of the ranking that "any permutation gives the same results,
parcels are independent": here a parcel's bits are compared across runs in which its lane, wave, workgroup and neighbours change.

Run with `-m gpu`.  n = BS + 1 and 2 BS + 1 with BS the workgroup size of the kernel that runs (test_ranked_adaptive_host.BLOCK, read
from the kernel generator): a full workgroup, a second one and a one-lane tail; ld = n + 15, out of place, sentinel-filled outputs.
Every batch, budget and parcel picked is chosen and justified on the oracle alone in tests/test_ranked_adaptive_host.py; the
references are the restatement there, a fine fixed-step run, and the device itself (bit equality).  The bounds are the project's:
1e-13 (B.TOL_EVAL for the box) x evaluations on the parcels with the restatement's (accepted, rejected), at most 5 % of parcels
without, 2 x the restatement's error + 1e-12 against the fine run.

No case reaches status 2 after an attempt: the host file's docstring says what was tried."""
import functools

import numpy as np
import pytest

import test_box_adaptive_host as B
import test_ranked_adaptive_host as R
import test_tsit5_adaptive_host as H
from gpu_support import _tsit5_host, adaptive, bits_equal, box_adaptive, is_blank, same_counts, saveat, two_gamma_plan
from tsit5_restated import save_times

pytestmark = pytest.mark.gpu

KEYS = ("u", "t", "dt", "accepted", "rejected", "status")
FAMILY = {"adaptive": "coal", "saveat": "coal", "box": "box", "box_saveat": "box"}
SAVES = {"adaptive": False, "saveat": True, "box": False, "box_saveat": True}
CASES = [(e, k) for e in FAMILY for k in R.KINDS]
both = pytest.mark.parametrize("entry,kind", CASES)


def run(cloudy, oracle, entry, kind, u0, s, t_span, **kw):
    """one call of an entry point on (u0, s); ld = n + 15 unless given.  -> the driver's dict"""
    _, _, plan = two_gamma_plan(cloudy, oracle, kind)
    kw.setdefault("ld", u0.shape[1] + 15)
    u0 = np.ascontiguousarray(u0)
    times = save_times(t_span) if SAVES[entry] else ()
    if FAMILY[entry] == "coal":
        return (saveat if SAVES[entry] else adaptive)(cloudy, plan, u0, t_span, times, **kw)
    return box_adaptive(cloudy, plan, u0, t_span, np.ascontiguousarray(s), B.XI_BOX, times=times, **kw)


def keys(entry):
    return KEYS + (("saved",) if SAVES[entry] else ())


@functools.lru_cache(maxsize=None)
def whole(cloudy, oracle, entry, kind, t_mult=1, hostile=False):
    """the run of the whole batch at n = 2 BS + 1, once per session -> (u0, s, role, result)"""
    n = R.sizes(FAMILY[entry], kind)[1]
    u0, s, role = R.batch(FAMILY[entry], kind, n, hostile)
    return u0, s, role, run(cloudy, oracle, entry, kind, u0, s, H.TWO_GAMMA_T[kind] * t_mult)


def assert_same_bits(entry, base, part, idx, flip=False):
    """the parcels idx of the whole run have the bits of the run `part` (flip: whose batch was reversed)"""
    for k in keys(entry):
        assert bits_equal(base[k][..., idx], part[k][..., ::-1] if flip else part[k]), (k, idx)


def untouched(entry, got):
    assert np.all(is_blank(got["pad"])) and bits_equal(got["u_in"], got["buf"])
    if SAVES[entry]:
        assert np.all(is_blank(got["saved_pad"]))


@functools.lru_cache(maxsize=None)
def fine_reference(family, kind, n):
    """every parcel by the fixed-step tableau at 25 steps (test_gpu_tsit5_adaptive.fine_reference), once per session"""
    from oracle import cloudy_oracle as oracle

    u0, s, _ = R.batch(family, kind, n)
    with np.errstate(all="ignore"):
        return _tsit5_host(R.rhs(oracle, family, kind, s), u0, H.TWO_GAMMA_T[kind] / 25, 25)


def parity(entry, u0, got, ref, same):
    """the worst agreement per evaluation of the final state (and of every snapshot) over the parcels `same`"""
    rel = np.abs(got["u"] - ref["u"]) / np.maximum(np.abs(u0) + np.abs(ref["u"]), 1e-300) / ref["evals"]
    worst = rel[:, same].max()
    if SAVES[entry]:
        fin = np.isfinite(ref["saved"])
        rel = np.abs(got["saved"] - ref["saved"]) / np.maximum(np.abs(u0)[None] + np.abs(ref["saved"]), 1e-300) / ref["evals"][None, None, :]
        assert np.array_equal(np.isfinite(got["saved"])[:, :, same], fin[:, :, same])
        worst = max(worst, np.where(fin, rel, 0.0)[:, :, same].max())
    return float(worst)


# ---- 1. parity at two workgroups and a tail
@both
def test_parity_past_two_workgroups(gpu_cloudy, oracle, entry, kind):
    """decision_parity / test_decision_parity / test_snapshot_parity_with_the_restatement at n = 2 BS + 1."""
    family = FAMILY[entry]
    u0, s, _, got = whole(gpu_cloudy, oracle, entry, kind)
    n = u0.shape[1]
    ref = R.reference(family, kind, n)
    assert np.all(got["status"] == 0) and np.all(got["t"] == H.TWO_GAMMA_T[kind])
    same = same_counts(got, ref)
    worst = parity(entry, u0, got, ref, same)
    fine = fine_reference(family, kind, n)
    assert np.isfinite(fine).all()
    ref_err, err = H.plane_errors(ref["u"], fine, u0), H.plane_errors(got["u"], fine, u0)
    print(f"{entry} {kind} n={n}: {(~same).sum()} of {n} parcels differ in (accepted, rejected); the others agree to {worst:.2e} x "
          f"evaluations; against a fine fixed-step run: restatement {ref_err}, device {err}")
    assert (~same).sum() <= 0.05 * n, (~same).sum()
    assert worst <= R.TOL_EVAL[family], worst
    assert np.all(err <= 2 * ref_err + 1e-12), (err, ref_err)
    untouched(entry, got)
    if SAVES[entry]:
        assert bits_equal(got["saved"][0], u0) and bits_equal(got["saved"][-1], got["u"])


# ---- 2. neighbour and batch-shape invariance
@both
def test_reversed_batch(gpu_cloudy, oracle, entry, kind):
    """parcel i at column n - 1 - i (its supersaturation with it): every lane, wave and workgroup changes, parcel 0 is the tail"""
    u0, s, _, base = whole(gpu_cloudy, oracle, entry, kind)
    part = run(gpu_cloudy, oracle, entry, kind, u0[:, ::-1], s[::-1], H.TWO_GAMMA_T[kind])
    assert_same_bits(entry, base, part, slice(None), flip=True)
    untouched(entry, part)


@both
def test_sub_batches(gpu_cloudy, oracle, entry, kind):
    """[0, 65), [BS - 32, BS + 33) -- it straddles the workgroup boundary, so its parcels change workgroup -- and [n - 65, n)"""
    u0, s, _, base = whole(gpu_cloudy, oracle, entry, kind)
    bs, n = R.BLOCK[FAMILY[entry], kind], u0.shape[1]
    for idx in (slice(0, 65), slice(bs - 32, bs + 33), slice(n - 65, n)):
        assert_same_bits(entry, base, run(gpu_cloudy, oracle, entry, kind, u0[:, idx], s[idx], H.TWO_GAMMA_T[kind]), idx)


@both
def test_parcels_alone(gpu_cloudy, oracle, entry, kind):
    """test_ranked_adaptive_host.singletons: at most 12 launches of one parcel"""
    u0, s, _, base = whole(gpu_cloudy, oracle, entry, kind)
    picked = R.singletons(R.reference(FAMILY[entry], kind, u0.shape[1]), R.BLOCK[FAMILY[entry], kind])
    assert len(picked) <= 12
    for i in picked:
        idx = slice(i, i + 1)
        assert_same_bits(entry, base, run(gpu_cloudy, oracle, entry, kind, u0[:, idx], s[idx], H.TWO_GAMMA_T[kind]), idx)


# ---- 2. / 4. hostile neighbours
@both
def test_hostile_neighbours(gpu_cloudy, oracle, entry, kind):
    """Three of four parcels replaced by all-zero, all-NaN, +Inf-in-M2 parcels and copies of the densest parcel: the call returns
    CLOUDY_OK; the kept parcels have the bits of the whole run; the zero, NaN and Inf parcels have the restatement's status (0, 2,
    2), counts and t, u_out as it came in for the status-2 ones, and every snapshot beyond t a NaN in every plane; the copies of the
    densest parcel finish and -- without condensation, whose supersaturation belongs to the column -- have its bits."""
    family = FAMILY[entry]
    u0, s, _, base = whole(gpu_cloudy, oracle, entry, kind)
    h0, _, role, got = whole(gpu_cloudy, oracle, entry, kind, hostile=True)
    n = u0.shape[1]
    ref = R.reference(family, kind, n, hostile=True)
    kept = np.flatnonzero(role == -1)
    for k in keys(entry):
        assert bits_equal(base[k][..., kept], got[k][..., kept]), k
    bad, zero = np.isin(role, (1, 2)), role == 0
    sick = bad | zero
    for k in ("status", "accepted", "rejected", "t"):
        assert np.array_equal(got[k][sick], ref[k][sick]), (k, got[k][sick], ref[k][sick])
    assert np.all(got["status"][bad] == 2) and np.all(got["status"][zero] == 0)
    assert bits_equal(got["u"][:, bad], h0[:, bad]) and not got["u"][:, zero].any()
    assert np.all(got["status"][role == 3] == 0) and np.all(got["t"][role == 3] == H.TWO_GAMMA_T[kind])
    if family == "coal":
        dense = int(np.argmax(u0[0]))
        for k in keys(entry):
            lanes = got[k][..., role == 3]
            assert bits_equal(lanes, np.repeat(base[k][..., dense:dense + 1], lanes.shape[-1], axis=-1)), k
    if SAVES[entry]:
        assert bits_equal(got["saved"][0], h0)
        assert np.isnan(got["saved"][1:, :, bad]).all() and not np.any(is_blank(got["saved"][:, :, bad]))
        assert np.isfinite(got["saved"][:, :, zero | (role == 3)]).all()
    untouched(entry, got)


# ---- 3. the budget
@both
def test_budget(gpu_cloudy, oracle, entry, kind):
    """test_ranked_adaptive_host.BUDGET[kind] at the standard t_span (the host file says why these and no larger budgets: only there
    does the restatement resolve t_reached): the statuses of the restatement; the stopped parcels with accepted + rejected ==
    max_steps and t < t_span, compared with the restatement where each stopped as test_max_steps_budget does (t to 1e-5, the state
    beyond |f| |dt| to the per-evaluation bound); every snapshot beyond a stopped parcel's t a NaN in every plane, the others finite
    and within the per-evaluation bound of the restatement's; the finished parcels of the same workgroups with the bits they have
    in the run without a budget."""
    cloudy, family, budget = gpu_cloudy, FAMILY[entry], R.BUDGET[kind]
    u0, s, _, free = whole(cloudy, oracle, entry, kind, t_mult=budget["t_mult"])
    n, t_span = u0.shape[1], H.TWO_GAMMA_T[kind] * budget["t_mult"]
    ref = R.reference(family, kind, n, **budget)
    got = run(cloudy, oracle, entry, kind, u0, s, t_span, max_steps=budget["max_steps"])
    slow = ref["status"] == 1
    assert np.array_equal(got["status"], ref["status"])
    assert np.all((got["accepted"] + got["rejected"])[slow] == budget["max_steps"]) and np.all(got["t"][slow] < t_span)
    done = np.flatnonzero(~slow)
    for k in keys(entry):
        assert bits_equal(got[k][..., done], free[k][..., done]), k
    same = same_counts(got, ref)
    assert (~same).sum() <= 0.05 * n, (~same).sum()
    dt_rel = np.abs(got["t"] - ref["t"]) / ref["t"]
    drift = np.abs(R.rhs(oracle, family, kind, s)(ref["u"])) * np.abs(got["t"] - ref["t"])
    excess = np.maximum(np.abs(got["u"] - ref["u"]) - 1.001 * drift, 0.0)
    rel = excess / np.maximum(np.abs(u0) + np.abs(ref["u"]), 1e-300) / ref["evals"]
    print(f"{entry} {kind}: {slow.sum()} of {n} parcels stopped; t_reached within {dt_rel[same].max():.2e} of the restatement's, the state "
          f"beyond |f| |dt| within {rel[:, same].max():.2e} x evaluations")
    assert dt_rel[same].max() <= 1e-5, dt_rel[same].max()
    assert rel[:, same].max() <= R.TOL_EVAL[family], rel[:, same].max()
    if SAVES[entry]:
        beyond = save_times(t_span)[:, None] > got["t"][None, :]
        assert beyond[:, slow].any() and (~beyond[:, slow]).any() and not beyond[:, ~slow].any()
        nan, fin = np.isnan(got["saved"]), np.isfinite(got["saved"])
        assert np.all(nan.all(axis=1) == beyond) and np.all(fin.all(axis=1) == ~beyond)
        assert not np.any(is_blank(got["saved"]))
        both_fin = fin & np.isfinite(ref["saved"])
        srel = np.abs(got["saved"] - ref["saved"]) / np.maximum(np.abs(u0)[None] + np.abs(ref["saved"]), 1e-300) / ref["evals"][None, None, :]
        worst = np.where(both_fin, srel, 0.0)[:, :, same].max()
        assert np.array_equal(fin[:, :, same], np.isfinite(ref["saved"])[:, :, same])
        assert worst <= R.TOL_EVAL[family], worst
    untouched(entry, got)


# ---- 4. a non-finite estimate inside the loop
@pytest.mark.parametrize("entry", list(FAMILY))
def test_nonfinite_estimate_is_rejected_and_recovered_from(gpu_cloudy, oracle, entry):
    """test_ranked_adaptive_host.H5 (the `moving` batch, 65 parcels, t_span = 1 and a first step of 1 through dt_dev): every parcel
    finishes; at most 5 % differ from the restatement in (accepted, rejected) and the others agree to the per-evaluation bound in
    the final state and in every snapshot; the parcels that took the h / 5 rejection in the restatement, flipped or not, agree with
    a fine fixed-step run (test_ranked_adaptive_host.h5_fine) to 2 x the restatement's error + 1e-12 and have at least as many
    rejections as in the restatement, but for flipped decisions: over those parcels the rejections missing sum to no more than the
    5 % of parcels that may differ."""
    family, kind, n, t_span = FAMILY[entry], R.H5["kind"], R.H5["n"], R.H5["t_span"]
    ref, took = R.h5_reference(family)
    u0, s, _ = R.batch(family, kind, n)
    got = run(gpu_cloudy, oracle, entry, kind, u0, s, t_span, dt_in=np.full(n, R.H5["dt"]))
    assert took.any() and np.all(got["status"] == 0) and np.all(got["t"] == t_span) and np.isfinite(got["u"]).all()
    same = same_counts(got, ref)
    worst = parity(entry, u0, got, ref, same)
    idx, fine = R.h5_fine(family)
    assert np.array_equal(idx, np.flatnonzero(took)) and np.isfinite(fine).all()
    ref_err, err = H.plane_errors(ref["u"][:, idx], fine, u0[:, idx]), H.plane_errors(got["u"][:, idx], fine, u0[:, idx])
    missing = np.maximum(ref["rejected"] - got["rejected"], 0)[took]
    print(f"{entry}: {(~same).sum()} of {n} parcels differ in (accepted, rejected); the others agree to {worst:.2e} x evaluations; "
          f"rejections of the h / 5 parcels: restatement {ref['rejected'][took]}, device {got['rejected'][took]}; those parcels against a "
          f"fine fixed-step run: restatement {ref_err}, device {err}")
    assert (~same).sum() <= 0.05 * n, (~same).sum()
    assert worst <= R.TOL_EVAL[family], worst
    assert np.all(err <= 2 * ref_err + 1e-12), (err, ref_err)
    assert np.all(got["rejected"][took] >= 1) and missing.sum() <= 0.05 * n, (got["rejected"][took], ref["rejected"][took])
    untouched(entry, got)
    if SAVES[entry]:
        assert bits_equal(got["saved"][0], u0) and bits_equal(got["saved"][-1], got["u"])


# ---- 5. warm start and in place
@pytest.mark.parametrize("entry", ["adaptive", "box"])
def test_warm_start_and_in_place(gpu_cloudy, oracle, entry):
    """The `fixed` plan at n = BS + 1: fed with the dt it returned, every parcel takes one attempt without a rejection under
    max_steps = 1, and the warm run takes no more attempts than the cold one; dt_dev = NULL has the bits of a zero-filled dt_dev in
    u, t, accepted, rejected and status; in place has the bits of out of place."""
    cloudy, kind = gpu_cloudy, "fixed"
    n = R.sizes(FAMILY[entry], kind)[0]
    u0, s, _ = R.batch(FAMILY[entry], kind, n)
    t_span = H.TWO_GAMMA_T[kind]
    first = run(cloudy, oracle, entry, kind, u0, s, t_span)
    assert np.all(first["status"] == 0) and np.all(first["dt"] > 0) and np.all(np.isfinite(first["dt"]))
    second = run(cloudy, oracle, entry, kind, first["u"], s, t_span, dt_in=first["dt"], max_steps=1)
    assert np.all(second["rejected"] == 0) and np.all(second["accepted"] == 1)
    warm = run(cloudy, oracle, entry, kind, first["u"], s, t_span, dt_in=first["dt"])
    cold = run(cloudy, oracle, entry, kind, first["u"], s, t_span)
    assert np.all(warm["status"] == 0)
    assert (warm["accepted"] + warm["rejected"]).sum() <= (cold["accepted"] + cold["rejected"]).sum()
    auto = run(cloudy, oracle, entry, kind, u0, s, t_span, dt_in=None)
    assert auto["dt"] is None
    for k in ("u", "t", "accepted", "rejected", "status"):
        assert bits_equal(auto[k], first[k]), k
    untouched(entry, auto)
    inplace = run(cloudy, oracle, entry, kind, u0, s, t_span, in_place=True)
    for k in KEYS:
        assert bits_equal(inplace[k], first[k]), k
