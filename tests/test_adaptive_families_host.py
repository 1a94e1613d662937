"""CPU-only half of the tests of the adaptive Tsit5 loop (tsit5_adaptive_loop, csrc/adaptive.hpp) on plan families beyond two Gamma
modes: mixed plane counts, three to eight modes, Monodisperse and Lognormal closures, fixed and moving thresholds past two modes.
Every input of tests/test_gpu_adaptive_families.py is chosen here, on the oracle alone, and every condition the GPU file relies on
is asserted here: the batch (statuses, attempt range, a one-step parcel beside a slow one, a rejected step, no parcel on a closure
clamp), the restatement's own answer to last-bit noise of its right-hand side, and a fine fixed-step run of every parcel.

The norm's denominator.  A loop that takes the mean over the 3 N padded slots, not over the planes the modes have (5 of 6 on
exp_gamma, 17 of 18 on six_modes), moves step sizes by 1.3 % and 0.4 %.  Few parcels of these batches change (accepted, rejected) for
that (6 and 0 of 257: most finish in one step or grow at the controller's cap), far from the 5 % the issue hoped for; what
test_the_batch_sees_a_norm_over_3n_slots asserts is what the GPU file's decision parity would catch it by: parcels that change
their counts or, with equal counts, leave the proper run by more than 10 x TOL_EVAL x evaluations (measured: 11 and 2 of 257).

The kernel tensors are those of the tests that pin the right-hand side of the same families (test_gpu_parity:
test_mode_and_order_families_vs_oracle up to four modes, test_plans_beyond_the_ahead_of_time_families beyond, the Golovin tensor of
test_monodisperse_and_lognormal_closures_vs_oracle).

The batches.  Every mode is POPULATED (test_tsit5_adaptive_host.two_gamma_batch says why): mode i holds N_RATIO^i of the cloud mode's
number, shapes k in 1 .. 6, mean masses inside the size class its thresholds give it; one dilution factor per parcel, log-uniform
over three decades and shuffled, multiplies every mode, so that collision rates span three decades over the batch and a parcel for
which t_span is one step sits beside one that takes many.  The PI controller does not reject a step on these smooth problems from
its own cautious first step (no family had a rejected step at any t_span short of the finite-time blow-up of its densest parcels),
so every WARM-th parcel comes with a first step of its own through dt_dev -- t_span itself, too long for the dense ones: those
reject it, the others take the automatic first step (dt_dev = 0), and one batch runs both.

The fine reference takes FINE x the accepted steps of the slowest parcel, i.e. a fifth of its MEAN accepted step, as
test_gpu_tsit5_adaptive.fine_reference does (50 steps for up to 10).  A fifth of the SMALLEST accepted step is out of reach: that is
the automatic first step, t_span / 430 on exp_gamma and t_span / 440 on gamma_exp_gamma_thr at their standard t_span, 2000 steps of
a thresholded oracle."""
import functools

import numpy as np
import pytest

import bench
import test_box_adaptive_host as B
import test_ranked_adaptive_host as R
import test_tsit5_adaptive_host as H
from test_host_abi import INF
from tsit5_restated import DONE, EPS, adaptive_tsit5, last_bit_noise, plane_norms, save_times

NP_OF = {0: 2, 1: 3, 2: 2, 3: 3}   # planes of an Exponential, Gamma, Monodisperse, Lognormal mode
GOLOVIN = "golovin"
BS = R.BLOCK["coal", "fixed"]      # cloudy_tsit5_adaptive[_saveat]: one literal workgroup size for every plan (asserted below)
# id -> dist types, tensor order P (or GOLOVIN), thresholds, MovingThreshold, parcels (BS + 1, or 65 where the thresholded oracle is
# slow: the whole file has to stay below the run time of test_ranked_adaptive_host.py), t_span
FAMILIES = {
    "exp_gamma": dict(types=(0, 1), P=3, thr=(INF, INF), moving=False, n=BS + 1, t_span=3e-4),
    "gamma_exp_gamma_thr": dict(types=(1, 0, 1), P=2, thr=(1e-10, 3e-8, INF), moving=False, n=BS + 1, t_span=1e-9),
    "four_gamma_thr": dict(types=(1, 1, 1, 1), P=3, thr=(1e-9, 1e-7, 1e-5, INF), moving=False, n=65, t_span=5e-9),
    "six_modes": dict(types=(1, 0, 1, 1, 1, 1), P=2, thr=(INF,) * 6, moving=False, n=BS + 1, t_span=3.8e-8),
    "eight_gamma": dict(types=(1,) * 8, P=2, thr=(INF,) * 8, moving=False, n=BS + 1, t_span=1e-8),
    "five_modes_thr": dict(types=(1, 1, 1, 0, 1), P=3, thr=(1e-10, 1e-9, 1e-8, 1e-7, INF), moving=False, n=65, t_span=3e-8),
    "mono_gamma_thr": dict(types=(2, 1), P=GOLOVIN, thr=(5e-10, INF), moving=False, n=BS + 1, t_span=0.1),
    "lognormal_pair_thr": dict(types=(3, 3), P=GOLOVIN, thr=(5e-10, INF), moving=False, n=BS + 1, t_span=0.1),
    "mono_lognormal_gamma": dict(types=(2, 3, 1), P=GOLOVIN, thr=(INF, INF, INF), moving=False, n=BS + 1, t_span=2e-3),
}
# DROPPED: six_moving -- types (1,) * 6, P = 2, MovingThreshold percentiles (0.9, 0.95, 0.99, 0.9, 0.99, 1.0), 65 parcels, t_span = 1e-7
# (attempts 1 .. 9).  Under last-bit noise of its right-hand side the restatement changes no (accepted, rejected) but moves its own end
# state by 8.1e-14 and 8.7e-14 x evaluations (noise seeds 1 and 2; the same with and without the warm first steps; three parcels
# above 1e-14, the worst in M2 of the third mode), against the 1e-14 asked of a reference: the percentile thresholds amplify the
# last bit of a stage state.  It is no reference at the 1e-13 the device would be held to, so the family has no adaptive test here.
IDS = tuple(FAMILIES)
N_RATIO = 0.1      # number of mode i + 1 over mode i
WARM = 4           # every WARM-th parcel starts from dt = t_span
FINE = 5           # fine steps per accepted step of the slowest parcel
RELTOL, ABSTOL = 1e-6, 1e-9
# the per-evaluation bound of the device against the restatement, per plan type: 1e-13 for all-Inf plans (decision_parity), and for
# thresholded and moving plans what test_gpu_ranked_adaptive.py holds its two-mode plans to
TOL_EVAL = {True: 1e-13, False: R.TOL_EVAL["coal"]}
RESOLUTION = R.RESOLUTION["coal"]   # what the restatement may move by under last-bit noise, per evaluation


def types_of(fid):
    return FAMILIES[fid]["types"]


def nprog(fid):
    return tuple(NP_OF[t] for t in types_of(fid))


def all_inf(fid):
    """the plan runs the per-lane loop on a normalised state (no thresholds); otherwise the ranked loop on a physical one"""
    f = FAMILIES[fid]
    return not f["moving"] and not any(np.isfinite(f["thr"]))


def kernel_tensor(fid):
    """(N, N, P, P): random symmetric tensors per pair, seeded and scaled as the parity test of the family's right-hand side does;
    GOLOVIN: CoalescenceTensor(LinearKernelFunction(5.0), 1, 1e-6).c for every pair"""
    f = FAMILIES[fid]
    N, P = len(f["types"]), f["P"]
    if P == GOLOVIN:
        return np.broadcast_to(np.array([[EPS * 1e-6, 5.0], [5.0, 0.0]]), (N, N, 2, 2)).copy()
    many = N > 4
    rng = np.random.default_rng((1000 if many else 100) * N + P)
    kc = np.zeros((N, N, P, P))
    for j in range(N):
        for k in range(j, N):
            a = rng.uniform(0, 1, (P, P)) * (rng.uniform(0, 1, (P, P)) < (0.6 if many else 0.7))
            a = (a + a.T) * np.array([[10.0 ** ((1 if many else 3) * (x + y)) for y in range(P)] for x in range(P)])
            kc[j, k] = kc[k, j] = a
    return kc


def size_classes(fid):
    """per mode the range of its mean mass: between its fixed thresholds (1.5 x the lower .. 0.7 x the upper one; two decades where
    one is missing), else the classes of bench.synth_moments (up to four modes) and of gpu_support.many_mode_moments"""
    f = FAMILIES[fid]
    N, thr = len(f["types"]), f["thr"]
    if f["moving"] or all_inf(fid):
        if N <= 4:
            return [(1e-11, 1e-9), (1e-9, 1e-7), (1e-7, 1e-5), (1e-5, 1e-3)][:N]
        e = np.logspace(-12, -4, N + 1)
        return [(e[i], e[i + 1]) for i in range(N)]
    out = []
    for i in range(N):
        hi = thr[i] if np.isfinite(thr[i]) else thr[i - 1] * 100
        lo = thr[i - 1] if i else hi / 100
        out.append((1.5 * lo, 0.7 * hi))
    return out


def batch(fid, seed=21, n=None):
    """-> (u0 (sum np, n), dt (n,): t_span for every WARM-th parcel, 0 = automatic for the others); n: the family's unless given"""
    f = FAMILIES[fid]
    n = f["n"] if n is None else n
    rng = np.random.Generator(np.random.Philox(key=seed))
    dilution = 10.0 ** (-3.0 * (np.arange(n) / (n - 1)))
    rng.shuffle(dilution)
    rows = []
    for i, (t, (x_lo, x_hi)) in enumerate(zip(f["types"], size_classes(fid))):
        top = 1e9 * N_RATIO ** i
        m = bench._gamma_mode(rng, n, 0.3 * top, top, 1.0, 6.0, x_lo, x_hi) * dilution
        rows += [m[0], m[1]] + ([m[2]] if NP_OF[t] == 3 else [])
    dt = np.where(np.argsort(np.argsort(dilution)[::-1]) % WARM == 1, f["t_span"], 0.0)   # (by rank of density: the second densest, ...)
    return np.ascontiguousarray(np.stack(rows)), dt


def params(oracle, fid):
    f = FAMILIES[fid]
    return oracle.make_params(list(f["types"]), kernel_tensor(fid), f["thr"], norms=bench.NORMS, threshold_style=1 if f["moving"] else 0)


def coal_rhs(oracle, fid, perturb=None):
    op = params(oracle, fid)
    f = lambda u: oracle.rhs_coal_batch(op, u)  # noqa: E731
    return f if perturb is None else (lambda u: f(u) * perturb(u.shape))


def opts_of(fid, dt, max_steps=10000):
    return dict(reltol=RELTOL, abstol=ABSTOL, max_steps=max_steps, dt=dt, plane_norms=plane_norms(nprog(fid)), normalised=all_inf(fid))


def restatement(oracle, fid, perturb=None, max_steps=10000, t_save=None, warm=True):
    """warm = False: every first step automatic (the snapshot entry point's driver hands in a dt_dev of zeros)"""
    u0, dt = batch(fid)
    return adaptive_tsit5(coal_rhs(oracle, fid, perturb), u0, FAMILIES[fid]["t_span"], opts_of(fid, dt if warm else None, max_steps), t_save=t_save)


@functools.lru_cache(maxsize=None)
def reference(fid, max_steps=10000, saveat=None, warm=True):
    """the unperturbed restatement, once per session and shared (treat the arrays as read-only); saveat: a tuple of save times"""
    from oracle import cloudy_oracle

    return restatement(cloudy_oracle, fid, max_steps=max_steps, t_save=None if saveat is None else np.array(saveat), warm=warm)


@functools.lru_cache(maxsize=None)
def fine_reference(fid):
    """every parcel by the fixed-step tableau at FINE x the accepted steps of the restatement's slowest parcel"""
    from oracle import cloudy_oracle
    from gpu_support import _tsit5_host

    n_fine = FINE * int(reference(fid)["accepted"].max())
    with np.errstate(all="ignore"):
        return _tsit5_host(coal_rhs(cloudy_oracle, fid), batch(fid)[0], FAMILIES[fid]["t_span"] / n_fine, n_fine)


def on_a_clamp(oracle, fid, u):
    """per parcel: some mode's closure is on a clamp -- the fallback (0, 1, 1), a Gamma shape at k_min = eps or k_max = 10, a
    Lognormal sigma at eps"""
    prm = oracle.update_dist_batch(params(oracle, fid), u)
    bad = np.zeros(u.shape[1], bool)
    for m, t in enumerate(types_of(fid)):
        bad |= prm[3 * m] == 0.0
        if t == 1:
            bad |= (prm[3 * m + 2] <= EPS) | (prm[3 * m + 2] >= 10.0)
        if t == 3:
            bad |= prm[3 * m + 2] <= EPS
    return bad


def changed(a, b):
    return (a["accepted"] != b["accepted"]) | (a["rejected"] != b["rejected"])


def test_one_workgroup_size_for_every_plan():
    """adaptive_kernel of csrc/jit.hpp gives cloudy_tsit5_adaptive[_saveat] one literal workgroup size, whatever the plan's modes
    and thresholds (test_block_sizes_are_those_the_kernel_generator_uses reads it); n = BS + 1 is a full workgroup and one lane"""
    assert R.BLOCK["coal", "fixed"] == R.BLOCK["coal", "moving"] == BS == 256
    assert all(f["n"] in (BS + 1, 65) and len(f["thr"]) == len(f["types"]) for f in FAMILIES.values())


@pytest.mark.parametrize("fid", IDS)
def test_conditions_on_the_batch(oracle, fid):
    u0, dt = batch(fid)
    ref = reference(fid)
    att = ref["accepted"] + ref["rejected"]
    pair = (att[:-1] == 1) & (att[1:] >= 3) | (att[:-1] >= 3) & (att[1:] == 1)
    print(f"{fid}: n={u0.shape[1]} planes={u0.shape[0]} t_span={FAMILIES[fid]['t_span']:g}: attempts {att.min()} .. {att.max()}, "
          f"{(att == 1).sum()} parcels in one step, {ref['rejected'].sum()} rejected steps in {(ref['rejected'] > 0).sum()} parcels")
    assert u0.shape == (sum(nprog(fid)), FAMILIES[fid]["n"]) and np.isfinite(u0).all() and (u0 > 0).all()
    assert np.all(ref["status"] == DONE) and np.all(ref["t"] == FAMILIES[fid]["t_span"]) and np.isfinite(ref["u"]).all()
    assert att.max() >= 5 and pair.any() and ref["rejected"].sum() >= 1
    assert (dt > 0).sum() >= u0.shape[1] // WARM and np.any(ref["rejected"][dt == 0] == 0)
    assert not on_a_clamp(oracle, fid, u0).any() and not on_a_clamp(oracle, fid, ref["u"]).any()


@pytest.mark.parametrize("fid", IDS)
def test_decisions_are_insensitive_to_the_last_bit_of_the_rhs(oracle, fid):
    """test_tsit5_adaptive_host's test of the same name on every family: with every entry of the right-hand side multiplied by
    1 +- 1e-15 at most 1 % of the parcels change (accepted, rejected), and the end state of the others moves by at most 1e-14 x
    evaluations of |u0| + |u| per plane -- a tenth of what the GPU file asks of the device."""
    u0, _ = batch(fid)
    base = reference(fid)
    pert = restatement(oracle, fid, perturb=last_bit_noise(1))
    diff = changed(base, pert)
    rel = np.abs(pert["u"] - base["u"]) / np.maximum(np.abs(u0) + np.abs(base["u"]), 1e-300) / base["evals"]
    moved = float(rel[:, ~diff].max())
    print(f"{fid}: {int(diff.sum())} of {diff.size} parcels change (accepted, rejected) under last-bit noise of the right-hand side; the "
          f"end state of the others moves by {moved:.1e} x evaluations")
    assert diff.sum() <= 0.01 * diff.size, diff.sum()
    assert moved <= RESOLUTION, moved


@pytest.mark.parametrize("fid", IDS)
def test_fine_fixed_step_reference(fid):
    u0, _ = batch(fid)
    ref, fine = reference(fid), fine_reference(fid)
    err = H.plane_errors(ref["u"], fine, u0)
    print(f"{fid}: the restatement against {FINE * int(ref['accepted'].max())} fixed steps, per plane: max {err.max():.2e} ({err})")
    assert np.isfinite(fine).all()
    assert err.max() <= 100 * RELTOL, err   # (the bound of test_restatement_against_the_golovin_closed_form)


# ---- the norm's denominator
def restatement_over_3n(oracle, fid):
    """the bug the batch must see: the same loop with the norm's mean over all 3 N slots -- every two-moment mode gets a third plane
    of zeros with a zero tendency, as the device's padded slot has -> (result, the rows of the planes the modes have)"""
    u0, dt = batch(fid)
    np_ = nprog(fid)
    keep = np.concatenate([3 * m + np.arange(p) for m, p in enumerate(np_)])
    f = coal_rhs(oracle, fid)

    def padded(v):
        out = np.zeros_like(v)
        out[keep] = f(np.ascontiguousarray(v[keep]))
        return out

    u_pad = np.zeros((3 * len(np_), u0.shape[1]))
    u_pad[keep] = u0
    o = opts_of(fid, dt)
    o["plane_norms"] = plane_norms((3,) * len(np_))
    return adaptive_tsit5(padded, u_pad, FAMILIES[fid]["t_span"], o), keep


@pytest.mark.parametrize("fid", ["exp_gamma", "six_modes"])
def test_the_batch_sees_a_norm_over_3n_slots(oracle, fid):
    """test_decision_parity fails on a device with that bug if more than 5 % of the parcels change (accepted, rejected) or ONE parcel
    with equal counts leaves the restatement by more than TOL_EVAL x evaluations.  Asserted here, with a margin of ten over the bound
    (the device's own distance from the restatement is below a tenth of it) and for more than one parcel: at least two parcels change
    counts or move by more than 10 x TOL_EVAL x evaluations."""
    u0, _ = batch(fid)
    base = reference(fid)
    wrong, keep = restatement_over_3n(oracle, fid)
    diff = changed(base, wrong)
    rel = (np.abs(wrong["u"][keep] - base["u"]) / np.maximum(np.abs(u0) + np.abs(base["u"]), 1e-300) / base["evals"]).max(axis=0)
    moved = ~diff & (rel > 10 * TOL_EVAL[True])
    print(f"{fid}: with the norm over 3 N slots {int(diff.sum())} of {diff.size} parcels change (accepted, rejected), {int(moved.sum())} "
          f"others move by more than {10 * TOL_EVAL[True]:g} x evaluations (the worst by {rel[~diff].max():.1e})")
    assert np.all(wrong["status"] == DONE)
    assert diff.sum() + moved.sum() >= 2 and (diff.sum() > 0.05 * diff.size or moved.sum() >= 1)


# ---- snapshots: which save times the restatement resolves
SAVEAT_IDS = ("exp_gamma", "gamma_exp_gamma_thr", "six_modes", "lognormal_pair_thr")
# Per family the indices into saveat_times at which the restatement, under last-bit noise of its right-hand side, moves its own
# snapshot by at most RESOLUTION x evaluations: there the GPU file holds the device's snapshots to TOL_EVAL.  At the others it does
# not (the interpolant's weights reach 48 and cancel; largest at 0.37 .. 0.97 t_span: 2.0e-12 on gamma_exp_gamma_thr, 8.5e-13 on
# six_modes, 1.2e-14 on exp_gamma, 1.7e-14 on lognormal_pair_thr) and the restatement is no reference at 1e-13; the device's
# figure is printed there.  test_snapshot_resolution_of_the_restatement asserts both halves, so a save time comes back when it can.
SNAPSHOTS_RESOLVED = {"exp_gamma": (0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12), "gamma_exp_gamma_thr": (0, 1, 2, 11, 12),
                      "six_modes": (0, 1, 2, 11, 12), "lognormal_pair_thr": (0, 1, 2, 3, 4, 7, 9, 10, 11, 12)}


def saveat_times(t_span):
    """the twelve save times of every test (0 and t_span among them) and one inside the first step"""
    return np.sort(np.append(save_times(t_span), 1e-4 * t_span))


@pytest.mark.parametrize("fid", SAVEAT_IDS)
def test_snapshot_resolution_of_the_restatement(oracle, fid):
    times = saveat_times(FAMILIES[fid]["t_span"])
    u0, _ = batch(fid)
    base = reference(fid, saveat=tuple(times), warm=False)
    pert = restatement(oracle, fid, perturb=last_bit_noise(1), t_save=times, warm=False)
    same = ~changed(base, pert)
    rel = np.abs(pert["saved"] - base["saved"]) / np.maximum(np.abs(u0)[None] + np.abs(base["saved"]), 1e-300) / base["evals"][None, None, :]
    moved = rel[:, :, same].max(axis=(1, 2))
    print(f"{fid}: the restatement's own snapshots under last-bit noise, x evaluations per save time: {moved}")
    ok = np.isin(np.arange(times.size), SNAPSHOTS_RESOLVED[fid])
    assert same.all() and np.all(base["status"] == DONE)
    assert times[1] > 0 and all(steps[0] >= 1 for steps in base["in_step"])   # (every parcel's first accepted step holds times[1])
    assert np.all(moved[ok] <= RESOLUTION) and np.all(moved[~ok] > RESOLUTION), moved
    assert {0, 1, 2, 11, 12} <= set(SNAPSHOTS_RESOLVED[fid])   # the input, inside the first step, an interpolated one, 0.999 t_span, t_span


# ---- the box entry point: coalescence + condensation
# workgroup sizes of cloudy_box_tsit5_adaptive (test_block_sizes_are_those_the_kernel_generator_uses: kBlock on all-Inf plans, the
# wide ranked size on fixed thresholds with at most three modes): n = BS + 1 of the kernel that runs
BOX_N = {"exp_gamma": BS + 1, "gamma_exp_gamma_thr": R.BLOCK["box", "fixed"] + 1}
# xi per family: XI_BOX of test_box_adaptive_host where t_span is long enough for condensation to move the state (9e-4 of it on
# exp_gamma); over the 1e-9 s of gamma_exp_gamma_thr (its random tensors make coalescence that fast) XI_BOX moves it by 2e-8, so
# xi is raised until condensation moves it by 1e-3 as well: a source the test can see, not a physical one
BOX_XI = {"exp_gamma": B.XI_BOX, "gamma_exp_gamma_thr": 0.5}


def box_rhs(oracle, fid, perturb=None):
    op = params(oracle, fid)
    s = B.box_supersaturation(BOX_N[fid])
    f = lambda u: oracle.rhs_coal_batch(op, u) + oracle.rhs_condensation_batch(op, BOX_XI[fid], s, u)  # noqa: E731
    return f if perturb is None else (lambda u: f(u) * perturb(u.shape))


def box_restatement(oracle, fid, perturb=None):
    u0, dt = batch(fid, n=BOX_N[fid])
    return adaptive_tsit5(box_rhs(oracle, fid, perturb), u0, FAMILIES[fid]["t_span"], opts_of(fid, dt))


@functools.lru_cache(maxsize=None)
def box_reference(fid):
    from oracle import cloudy_oracle

    return box_restatement(cloudy_oracle, fid)


@pytest.mark.parametrize("fid", tuple(BOX_N))
def test_box_batches(oracle, fid):
    """COAL | COND with a supersaturation per parcel (test_box_adaptive_host.box_supersaturation, BOX_XI) on the family's batch at
    the box kernel's BS + 1: every status 0, no parcel ends on a clamp, the slowest takes >= 5 attempts beside one-step parcels, a
    step is rejected, condensation moves the state; under last-bit noise at most 1 % change (accepted, rejected) and the others move
    by at most B.TOL_EVAL x evaluations (the bounds of test_box_adaptive_host)."""
    u0, _ = batch(fid, n=BOX_N[fid])
    base, pert = box_reference(fid), box_restatement(oracle, fid, perturb=last_bit_noise(1))
    att = base["accepted"] + base["rejected"]
    diff = changed(base, pert)
    scale = np.maximum(np.abs(u0) + np.abs(base["u"]), 1e-300)
    moved = float((np.abs(pert["u"] - base["u"]) / scale / base["evals"])[:, ~diff].max())
    tendency = oracle.rhs_condensation_batch(params(oracle, fid), BOX_XI[fid], B.box_supersaturation(BOX_N[fid]), u0)
    cond = float((np.abs(tendency) * FAMILIES[fid]["t_span"] / scale).max())
    print(f"box {fid} n={BOX_N[fid]}: attempts {att.min()} .. {att.max()}, {base['rejected'].sum()} rejected; condensation alone would move "
          f"the state by up to {cond:.1e}; under last-bit noise {int(diff.sum())} parcels change counts, the others move by {moved:.1e} x evaluations")
    assert np.all(base["status"] == DONE) and not on_a_clamp(oracle, fid, base["u"]).any()
    assert att.min() == 1 and att.max() >= 5 and base["rejected"].sum() >= 1 and cond > 1e-4
    assert diff.sum() <= 0.01 * diff.size and moved <= B.TOL_EVAL
