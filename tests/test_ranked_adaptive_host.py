"""CPU-only half of the tests of the RANKED adaptive Tsit5 kernels (tsit5_adaptive_loop<RANKED = true>, csrc/adaptive.hpp: the
instances of cloudy_tsit5_adaptive, cloudy_tsit5_adaptive_saveat and cloudy_box_tsit5_adaptive on plans with fixed or moving
thresholds, which re-rank the workgroup through LDS in every right-hand-side evaluation).  Every input of
tests/test_gpu_ranked_adaptive.py is chosen here, on the oracle alone, and every condition the GPU file relies on is asserted here:

  * the workgroup sizes (BLOCK) are read out of the code that generates the plan-time units, so that n = BS + 1 and n = 2 BS + 1 are a full
    workgroup + one lane and two full workgroups + one lane for the kernel that actually runs;
  * the restatement (tsit5_restated.adaptive_tsit5 with t_save on the unchanged oracle) answers last-bit noise of its right-hand
    side at those n with at most 5 % of changed (accepted, rejected) and RESOLUTION x evaluations of movement of the others;
  * the parcels run alone (SINGLETONS), the budget (BUDGET), the hostile neighbours (hostile_batch) and the batch whose stages
    leave the domain of the right-hand side (H5).

Status 2 AFTER at least one attempt: the issue's candidate was tried on the oracle -- both sources on the two-Gamma batches, 65
parcels, every parcel evaporating at s = -0.02, in six runs: `fixed` and `moving`, each with (xi, t_span) = (1e-5, 1), (1e-5, 30)
and (1e-4, 30), under a budget of 300 attempts.  No parcel ended with status 2; 0, 20, 11 (`fixed`) and 0, 7, 3 (`moving`) parcels
ran into the budget with status 1, and for those the search says nothing.  The (`fixed`, 1e-4, 30) run repeated with 5000 attempts
(four minutes): 55 parcels finish, 10 are still being followed with accepted steps at attempt 5000 (the slowest with n = 0.07 left in
its cloud mode), none is under dt_min = 1e-14 t_span.  No input tried reaches status 2 after an attempt, so the GPU file has no such
case; test_status_2_after_an_attempt_is_not_reached_by_a_physical_input keeps the (`fixed`, 1e-4, 30, 300 attempts) run."""
import functools
import os
import re

import numpy as np
import pytest

import test_box_adaptive_host as B
import test_tsit5_adaptive_host as H
from tsit5_restated import DONE, DT_MIN, MAX_STEPS, adaptive_tsit5, last_bit_noise, plane_norms, save_times

KINDS = ("fixed", "moving")
FAMILIES = ("coal", "box")   # coal: cloudy_tsit5_adaptive[_saveat]; box: cloudy_box_tsit5_adaptive with COAL | COND
# workgroup size per (family, kind): test_block_sizes_are_those_the_kernel_generator_uses reads them out of csrc/jit.hpp
BLOCK = {("coal", "fixed"): 256, ("coal", "moving"): 256, ("box", "fixed"): 512, ("box", "moving"): 256}
CASES = [(f, k) for f in FAMILIES for k in KINDS]
# the per-evaluation bound the project asserts per family (test_gpu_tsit5_adaptive.decision_parity, test_gpu_box_adaptive)
TOL_EVAL = {"coal": 1e-13, "box": B.TOL_EVAL}
# what the restatement may move by under last-bit noise, per evaluation, as the two tests extended here assert it
# (test_decisions_are_insensitive_to_the_last_bit_of_the_rhs: 1e-14; ..._of_the_combined_rhs: below TOL_EVAL)
RESOLUTION = {"coal": 1e-14, "box": B.TOL_EVAL}
ROLES = ("zero", "nan", "inf", "dense")
# The budget on ranked plans, per kind, at the standard t_span.  A stopped parcel's t_reached is a sum of controller proposals, and
# a proposal after a step whose error estimate is small but above the clamp of q carries rounding noise of eps / (reltol EEst)
# (test_max_steps_budget has the reasoning): on these batches the restatement itself, its right-hand side multiplied by 1 +- 1e-15
# per entry, moves its t_reached by 1e-5 .. 5e-2 for every (max_steps, t_span) scanned -- max_steps 1 .. 5, t_span x 0.5 .. 16 --
# that stops >= 5 parcels per workgroup, except these: `fixed` with max_steps = 1 (t_reached is the first step, Hairer's guess: 1e-15;
# 42 .. 118 stopped per workgroup) and `moving` with max_steps = 2 (the second proposal is on the clamp: 1e-15; 12 and 16 stopped).
# (`moving` with max_steps = 2 over 2 t_span also resolves it, 1e-15 with 19 stopped per workgroup; the standard t_span is kept so that
# the run without a budget is the one the other tests share.)
# Only there is the restatement a reference for t_reached at the 1e-5 the GPU test asks; test_budget_choice asserts 1e-7.
BUDGET = {"fixed": dict(max_steps=1, t_mult=1), "moving": dict(max_steps=2, t_mult=1)}
# finite parcels whose stage states leave the domain of the right-hand side: a first step of the whole t_span = 1 (1000 x the
# standard one of the `moving` batch), handed in through dt_dev
H5 = dict(kind="moving", n=65, t_span=1.0, dt=1.0)
# the fine fixed-step run of the H5 parcels that take the h / 5 rejection: 100 steps where the restatement takes up to 58 attempts of
# very unequal size; the restatement's error against it is the same to three digits with 100, 200, 400, 800 and 1600 steps
H5_FINE_STEPS = 100


def sizes(family, kind):
    """(BS + 1, 2 BS + 1): a full workgroup + a one-lane tail, and the same past a second workgroup"""
    bs = BLOCK[family, kind]
    return bs + 1, 2 * bs + 1


def rhs(oracle, family, kind, s, perturb=None, seen=None):
    """the oracle right-hand side of a family on a two-Gamma plan; seen (n,) bool: set where a column came back non-finite"""
    op, _, _, _ = H.two_gamma_case(oracle, kind)
    if family == "coal":
        f = lambda u: oracle.rhs_coal_batch(op, u)  # noqa: E731
    else:
        f = lambda u: oracle.rhs_coal_batch(op, u) + oracle.rhs_condensation_batch(op, B.XI_BOX, s, u)  # noqa: E731

    def g(u):
        out = f(u)
        if seen is not None:
            np.logical_or(seen, ~np.isfinite(out).all(axis=0), out=seen)
        return out if perturb is None else out * perturb(u.shape)
    return g


def hostile_batch(u0):
    """every fourth parcel kept; the others replaced in rotation by an all-zero parcel, an all-NaN parcel, a parcel with +Inf in
    M2 of the cloud mode, and a copy of the densest parcel of the batch -> (batch, role per parcel: -1 kept, else index into ROLES)"""
    u = u0.copy()
    n = u0.shape[1]
    role = np.full(n, -1)
    replaced = np.flatnonzero(np.arange(n) % 4 != 0)
    role[replaced] = np.arange(replaced.size) % 4
    dense = int(np.argmax(u0[0]))
    u[:, role == 0] = 0.0
    u[:, role == 1] = np.nan
    u[2, role == 2] = np.inf
    u[:, role == 3] = u0[:, [dense]]
    return u, role


def batch(family, kind, n, hostile=False):
    """-> (u0, s, role): H.two_gamma_batch and B.box_supersaturation (read by the box family alone)"""
    u0 = H.two_gamma_batch(n, kind=kind)
    role = np.full(n, -1)
    if hostile:
        u0, role = hostile_batch(u0)
    return u0, B.box_supersaturation(n), role


def restatement(oracle, family, kind, n, max_steps=10000, t_mult=1, hostile=False, dt=None, t_span=None, perturb=None, seen=None):
    """adaptive_tsit5 with t_save (it integrates as without and adds the snapshots) at the twelve save times"""
    u0, s, _ = batch(family, kind, n, hostile)
    t_span = H.TWO_GAMMA_T[kind] * t_mult if t_span is None else t_span
    opts = dict(reltol=1e-6, abstol=1e-9, max_steps=max_steps, dt=dt, plane_norms=plane_norms((3, 3)), normalised=False)
    return adaptive_tsit5(rhs(oracle, family, kind, s, perturb, seen), u0, t_span, opts, t_save=save_times(t_span))


@functools.lru_cache(maxsize=None)
def reference(family, kind, n, max_steps=10000, t_mult=1, hostile=False):
    """the unperturbed restatement, once per session and shared (treat the arrays as read-only)"""
    from oracle import cloudy_oracle

    return restatement(cloudy_oracle, family, kind, n, max_steps, t_mult, hostile)


@functools.lru_cache(maxsize=None)
def h5_reference(family):
    """-> (the restatement on the H5 batch, parcels that took the h / 5 rejection: a non-finite stage derivative makes the error
    estimate non-finite whatever the weights, the parcel was active, and it finished with status 0)"""
    from oracle import cloudy_oracle

    seen = np.zeros(H5["n"], bool)
    ref = restatement(cloudy_oracle, family, H5["kind"], H5["n"], t_span=H5["t_span"], dt=H5["dt"], seen=seen)
    return ref, seen & (ref["status"] == DONE) & (ref["rejected"] >= 1)


@functools.lru_cache(maxsize=None)
def h5_fine(family):
    """-> (the parcels of the H5 batch that take the h / 5 rejection, their end state by the fixed-step tableau at H5_FINE_STEPS
    steps on the oracle's right-hand side), once per session"""
    from oracle import cloudy_oracle
    from gpu_support import _tsit5_host

    idx = np.flatnonzero(h5_reference(family)[1])
    u0, s, _ = batch(family, H5["kind"], H5["n"])
    with np.errstate(all="ignore"):
        return idx, _tsit5_host(rhs(cloudy_oracle, family, H5["kind"], s[idx]), np.ascontiguousarray(u0[:, idx]),
                                H5["t_span"] / H5_FINE_STEPS, H5_FINE_STEPS)


def singletons(ref, bs):
    """At most 12 parcels to run alone, picked from the restatement: per workgroup the parcel with the fewest and the one with
    the most attempts; 0, BS - 1, BS and n - 1; a parcel that finishes in a single step beside one that takes >= 3, and that one"""
    att = ref["accepted"] + ref["rejected"]
    n = att.size
    picked = [0, bs - 1, bs, n - 1]
    for lo in range(0, n, bs):
        picked += [lo + int(np.argmin(att[lo:lo + bs])), lo + int(np.argmax(att[lo:lo + bs]))]
    pair = np.flatnonzero((att[:-1] == 1) & (att[1:] >= 3))
    picked += [int(pair[0]), int(pair[0]) + 1]
    return sorted(set(picked))


def changed_and_moved(u0, base, pert):
    diff = (base["accepted"] != pert["accepted"]) | (base["rejected"] != pert["rejected"])
    rel = np.abs(pert["u"] - base["u"]) / np.maximum(np.abs(u0) + np.abs(base["u"]), 1e-300) / base["evals"]
    return diff, float(rel[:, ~diff].max())


# ---- 0. the workgroup sizes, from the code that generates the kernels
def test_block_sizes_are_those_the_kernel_generator_uses():
    """csrc/jit.hpp: adaptive_kernel gives both kernels of cloudy_tsit5_adaptive[_saveat] a literal workgroup size;
    box_adaptive_kernel takes jit_sorted_block_size(h) where the parcels are ranked, which jit_sorted_block_size_resolve sets to
    kBlock unless the plan has fixed thresholds, at most three modes and at least one finite threshold.  (Read from the text: the
    generated units say the same in __launch_bounds__, but compiling them takes half a minute per plan.)"""
    src = os.path.join(H.ROOT, "cloudy.jl_amd", "csrc")
    jit = open(os.path.join(src, "jit.hpp")).read()
    k_block = int(re.search(r"constexpr int kBlock = (\d+);", open(os.path.join(src, "kernels.hpp")).read()).group(1))

    def body(name):
        start = jit.index("inline " + name)
        return jit[start:jit.index("\n}\n", start)]

    plain = re.search(r'"cloudy_jit_adaptive_tsit5"\) \+ jit_suffix\(h\), (\d+), tensor_waves\(h\)', body("JitKernel adaptive_kernel("))
    assert plain and ", true, " + plain.group(1) + ", true" in body("JitKernel adaptive_kernel(")
    assert "const int bs = box_bs(h, coal);" in body("JitKernel box_adaptive_kernel(")   # (the choice it shares with box_kernel)
    assert "int box_bs(const HostPlan &h, bool coal) { return coal && h.mode != MODE_ALLINF ? jit_sorted_block_size(h) : kBlock; }" in jit
    resolve = body("int jit_sorted_block_size_resolve(")
    assert "if (h.mode != MODE_FIXED || h.N > 3) return kBlock;" in resolve
    wide = re.search(r"for \(int i = 0; i < h.N - 1; \+\+i\) passes \+= h.finite\[i\] \? 1 : 0;\s+return passes >= 1 \? (\d+) : kBlock;", resolve)
    assert wide
    want = {("coal", "fixed"): int(plain.group(1)), ("coal", "moving"): int(plain.group(1)),
            ("box", "fixed"): int(wide.group(1)),   # two modes, thresholds (5e-9, Inf): one finite threshold
            ("box", "moving"): k_block}
    assert BLOCK == want, want


# ---- 1. the 5 % cap and the restatement's own resolution at the new shapes
@pytest.mark.parametrize("family,kind", CASES)
def test_decisions_are_insensitive_to_the_last_bit_of_the_rhs_at_two_workgroups(oracle, family, kind):
    """test_decisions_are_insensitive_to_the_last_bit_of_the_rhs and its box analogue at n = 2 BS + 1: with every entry of the
    right-hand side multiplied by 1 +- 1e-15 at most 5 % of the parcels change (accepted, rejected) and the end state of the
    others moves by at most RESOLUTION x evaluations of |u0| + |u|; every status is 0; some parcel takes one step beside one that
    takes three or more, and the slowest takes at least four attempts (these batches are drawn per n: at n = 513 the `fixed` one has
    no parcel with five)."""
    n = sizes(family, kind)[1]
    u0, _, _ = batch(family, kind, n)
    base = reference(family, kind, n)
    pert = restatement(oracle, family, kind, n, perturb=last_bit_noise(1))
    diff, moved = changed_and_moved(u0, base, pert)
    att = base["accepted"] + base["rejected"]
    print(f"{family} {kind} n={n}: attempts {att.min()} .. {att.max()}; {int(diff.sum())} parcels change (accepted, rejected) under "
          f"last-bit noise; the others move by {moved:.1e} x evaluations")
    assert np.all(base["status"] == DONE) and np.all(pert["status"] == DONE)
    assert att.min() == 1 and att.max() >= 4 and np.any((att[:-1] == 1) & (att[1:] >= 3))
    assert diff.sum() <= 0.05 * n, diff.sum()
    assert moved <= RESOLUTION[family], moved
    assert np.isfinite(base["saved"]).all() and np.array_equal(base["saved"][-1], base["u"])


# ---- 2. the parcels run alone
@pytest.mark.parametrize("family,kind", CASES)
def test_singletons(family, kind):
    bs, n = BLOCK[family, kind], sizes(family, kind)[1]
    ref = reference(family, kind, n)
    att = ref["accepted"] + ref["rejected"]
    picked = singletons(ref, bs)
    assert len(picked) <= 12 and {0, bs - 1, bs, n - 1} <= set(picked)
    for lo in range(0, n, bs):
        mine = att[[i for i in picked if lo <= i < lo + bs]]
        assert att[lo:lo + bs].min() in mine and att[lo:lo + bs].max() in mine
    assert any(att[i] == 1 and att[i + 1] >= 3 and i + 1 in picked for i in picked if i + 1 < n)


# ---- 3. the budget
@pytest.mark.parametrize("family,kind", CASES)
def test_budget_choice(oracle, family, kind):
    """BUDGET[kind] on every case at n = 2 BS + 1: in each full workgroup at least 5 parcels stop with status 1 and at least half
    finish with status 0 (the one-lane tail holds a single parcel: it finishes); no other status; every stopped parcel has
    accepted a step (t > 0); what it did not reach is NaN in the snapshots.  Under last-bit noise of the right-hand side (two
    seeds) no parcel changes its status or its counts and t_reached moves by at most 1e-7 relative: two orders below the 1e-5 the
    GPU test holds the device to, the margin of test_max_steps_budget."""
    bs, n = BLOCK[family, kind], sizes(family, kind)[1]
    budget = BUDGET[kind]
    ref = reference(family, kind, n, **budget)
    per = [((ref["status"][lo:lo + bs] == MAX_STEPS).sum(), (ref["status"][lo:lo + bs] == DONE).sum()) for lo in range(0, n, bs)]
    assert np.all((ref["status"] == MAX_STEPS) | (ref["status"] == DONE))
    assert all(stopped >= 5 and 2 * done >= bs for stopped, done in per[:-1]), per
    assert per[-1] == (0, 1)
    slow = ref["status"] == MAX_STEPS
    t_span = H.TWO_GAMMA_T[kind] * budget["t_mult"]
    assert np.all((ref["accepted"] + ref["rejected"])[slow] == budget["max_steps"])
    assert np.all(ref["t"][slow] < t_span) and np.all(ref["t"][slow] > 0) and np.all(ref["t"][~slow] == t_span)
    beyond = save_times(t_span)[:, None] > ref["t"][None, :]
    assert beyond[:, slow].any() and (~beyond[:, slow]).any() and not beyond[:, ~slow].any()
    assert np.array_equal(np.isnan(ref["saved"]).all(axis=1), beyond) and np.array_equal(np.isfinite(ref["saved"]).all(axis=1), ~beyond)
    moved = 0.0
    for seed in (1, 2):
        pert = restatement(oracle, family, kind, n, perturb=last_bit_noise(seed), **budget)
        assert np.array_equal(pert["status"], ref["status"])
        assert np.array_equal(pert["accepted"], ref["accepted"]) and np.array_equal(pert["rejected"], ref["rejected"])
        moved = max(moved, float((np.abs(pert["t"] - ref["t"]) / ref["t"]).max()))
    print(f"{family} {kind} n={n}: (stopped, finished) per workgroup {[(int(a), int(b)) for a, b in per]}; under last-bit noise the "
          f"restatement moves its own t_reached by {moved:.1e}")
    assert moved <= 1e-7, moved


# ---- 4. bad parcels
@pytest.mark.parametrize("family,kind", CASES)
def test_hostile_parcels_in_the_restatement(family, kind):
    """The NaN and the Inf parcel: status 2 without an attempt, t = 0, the state as it came; the all-zero parcel: one accepted step
    to t_span, status 0; the copies of the densest parcel and the kept parcels: what they are in the whole batch."""
    n = sizes(family, kind)[1]
    u0, _, role = batch(family, kind, n, hostile=True)
    ref, whole = reference(family, kind, n, hostile=True), reference(family, kind, n)
    t_span = H.TWO_GAMMA_T[kind]
    assert all((role == r).sum() >= n // 6 for r in range(4)) and np.array_equal(role == -1, np.arange(n) % 4 == 0)
    bad = (role == 1) | (role == 2)
    assert np.all(ref["status"][bad] == DT_MIN) and not ref["accepted"][bad].any() and not ref["rejected"][bad].any()
    assert np.all(ref["t"][bad] == 0.0) and np.isnan(ref["saved"][1:, :, bad]).all()
    zero = role == 0
    assert np.all(ref["status"][zero] == DONE) and np.all(ref["accepted"][zero] == 1) and not ref["rejected"][zero].any()
    assert np.all(ref["t"][zero] == t_span) and not ref["u"][:, zero].any()
    kept = role == -1
    for k in ("u", "t", "dt", "accepted", "rejected", "status"):
        assert np.array_equal(ref[k][..., kept], whole[k][..., kept]), k
    dense = int(np.argmax(H.two_gamma_batch(n, kind=kind)[0]))
    assert np.all(ref["status"][role == 3] == DONE)
    if family == "coal":   # (the box's copies keep the supersaturation of their own column)
        assert np.all(ref["u"][:, role == 3] == whole["u"][:, [dense]])


@pytest.mark.parametrize("family", FAMILIES)
def test_nonfinite_estimate_is_rejected_and_recovered_from(oracle, family):
    """H5: at least one finite parcel gets a non-finite stage derivative, takes the dt <- h / 5 rejection and finishes with status
    0, as every parcel of the batch does; the restatement answers last-bit noise there as on the standard batches (5 %, RESOLUTION
    x evaluations), so that the GPU test may hold the device to the same bounds."""
    ref, took = h5_reference(family)
    u0, _, _ = batch(family, H5["kind"], H5["n"])
    pert = restatement(oracle, family, H5["kind"], H5["n"], t_span=H5["t_span"], dt=H5["dt"], perturb=last_bit_noise(1))
    diff, moved = changed_and_moved(u0, ref, pert)
    att = ref["accepted"] + ref["rejected"]
    print(f"{family}: parcels {np.flatnonzero(took)} take the h / 5 rejection (rejected {ref['rejected'][took]}, attempts {att[took]}); "
          f"{int(diff.sum())} parcels change under last-bit noise, the others move by {moved:.1e} x evaluations")
    assert took.sum() >= 1 and np.isfinite(u0).all()
    assert np.all(ref["status"] == DONE) and np.all(ref["t"] == H5["t_span"]) and np.isfinite(ref["u"]).all()
    assert diff.sum() <= 0.05 * H5["n"], diff.sum()
    assert moved <= RESOLUTION[family], moved
    idx, fine = h5_fine(family)
    ref_err = H.plane_errors(ref["u"][:, idx], fine, u0[:, idx])
    print(f"{family}: the restatement's error on those parcels against {H5_FINE_STEPS} fixed steps: {ref_err}")
    assert np.isfinite(fine).all() and np.all(ref_err <= 1e-4)   # (reltol = 1e-6 over up to 58 attempts)


def test_status_2_after_an_attempt_is_not_reached_by_a_physical_input(oracle):
    """One run of the search the module docstring reports: the `fixed` two-Gamma batch, 65 parcels, both sources, every parcel
    evaporating (s = -0.02) ten times faster than in the other tests (xi = 1e-4) over t_span = 30 with a budget of 300 attempts.  No
    parcel ends with status 2; 54 finish and 11 run into the budget (status 1), for which this run is inconclusive -- with 5000
    attempts 10 of them still are, and a budget under which all finish does not fit a test."""
    s = np.full(65, -0.02)
    op, _, _, _ = H.two_gamma_case(oracle, "fixed")
    f = lambda u: oracle.rhs_coal_batch(op, u) + oracle.rhs_condensation_batch(op, 1e-4, s, u)  # noqa: E731
    res = adaptive_tsit5(f, H.two_gamma_batch(65, kind="fixed"), 30.0,
                         dict(reltol=1e-6, abstol=1e-9, max_steps=300, plane_norms=plane_norms((3, 3)), normalised=False))
    print(f"statuses {np.bincount(res['status'], minlength=3)}")
    assert np.array_equal(np.bincount(res["status"], minlength=3), [54, 11, 0])
