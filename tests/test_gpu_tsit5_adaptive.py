"""GPU tests of cloudy_tsit5_adaptive (csrc/adaptive.hpp): per-parcel adaptive Tsit5 to t_span.  The reference is the NumPy
restatement of tests/test_tsit5_adaptive_host.py driven by the unchanged oracle's right-hand side, the closed form of the
single-mode Golovin box, and the fixed-step tableau (_tsit5_host) at a fine step.

Run with `-m gpu`.  Batch sizes: a single parcel, a partial wave beyond one wave, a partial workgroup beyond one workgroup
(1, 65, 257).  The batches and t_span are picked on the oracle alone (test_tsit5_adaptive_host.py)."""
import functools

import numpy as np
import pytest

import bench
import test_tsit5_adaptive_host as H
from gpu_support import SENTINEL, SIZES, _tsit5_host, adaptive, dev, golovin_plan, same_counts, two_gamma_plan

pytestmark = pytest.mark.gpu


# ---- 1. closed form
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("reltol", H.TOLS)
@pytest.mark.parametrize("dist", ["gamma", "exponential"])
def test_golovin_closed_form(gpu_cloudy, oracle, dist, reltol, n):
    """Single-mode Golovin boxes, n over three decades, against M0 e^(-b M1 t), M1, M2 e^(2 b M1 t): per plane the device's
    maximum of |got - exact| / (|u0| + |exact|) is at most twice the restatement's on the same batch + 1e-12 (one flipped
    decision moves a step size by a bounded factor while the error stays O(tol)); all statuses 0, t_reached == t_span bit for
    bit; the padding columns of the out-of-place buffers are untouched."""
    cloudy = gpu_cloudy
    par, op, plan = golovin_plan(cloudy, oracle, dist)
    u0, exact, ref, ref_err = H.golovin_case(oracle, dist, n, reltol)
    got = adaptive(cloudy, plan, u0, H.GOLOVIN_T, reltol=reltol, ld=n + 15)
    err = H.plane_errors(got["u"], exact, u0)
    print(f"{dist} reltol={reltol:g} n={n}: restatement's max error per plane {ref_err}, device's {err}; "
          f"{(~same_counts(got, ref)).sum()} parcels differ in (accepted, rejected)")
    assert np.all(got["status"] == 0) and np.all(got["t"] == H.GOLOVIN_T)
    assert np.all(err <= 2 * ref_err + 1e-12), (err, ref_err)
    assert np.all(got["pad"].view(np.uint64) == SENTINEL) and np.array_equal(got["u_in"], got["buf"])


# ---- 2. / 3. decision parity
@functools.lru_cache(maxsize=None)
def fine_reference(oracle, kind, n):
    """every parcel of the (kind, n) batch by the fixed-step tableau at a step well below the adaptive one's, computed once per
    session: 50 steps where the restatement takes up to 10 (all-Inf), 25 where it takes up to 6 (thresholded plans, whose oracle
    is slow) -- a 5th-order error (6/25)^5 = 8e-4 of the restatement's own"""
    op, _, _, _ = H.two_gamma_case(oracle, kind)
    u0 = H.two_gamma_batch(n, kind=kind)
    n_fine = 50 if kind == "allinf" else 25
    with np.errstate(all="ignore"):
        return _tsit5_host(lambda v: oracle.rhs_coal_batch(op, v), u0, H.TWO_GAMMA_T[kind] / n_fine, n_fine)


def decision_parity(cloudy, oracle, kind, n):
    par, op, plan = two_gamma_plan(cloudy, oracle, kind)
    u0, ref = H.two_gamma_reference_cached(kind, n)
    t_span = H.TWO_GAMMA_T[kind]
    got = adaptive(cloudy, plan, u0, t_span)
    attempts = ref["accepted"] + ref["rejected"]
    assert np.all(ref["status"] == 0) and attempts.max() >= 5
    if n > 1:   # a parcel for which t_span is a single step sits next to one that takes several
        assert np.any((attempts[:-1] == 1) & (attempts[1:] >= 3) | (attempts[:-1] >= 3) & (attempts[1:] == 1))
    assert np.all(got["status"] == 0) and np.all(got["t"] == t_span)
    same = same_counts(got, ref)
    scale = np.abs(u0) + np.abs(ref["u"])
    dev_rel = np.abs(got["u"] - ref["u"]) / np.maximum(scale, 1e-300)
    worst = (dev_rel / ref["evals"])[:, same].max()
    print(f"{kind} n={n}: {(~same).sum()} of {n} parcels differ in (accepted, rejected); the others agree to {worst:.2e} x evaluations")
    # every parcel, flipped or not, against a fine fixed-step run
    fine = fine_reference(oracle, kind, n)
    assert np.isfinite(fine).all(), np.flatnonzero(~np.isfinite(fine).all(axis=0))
    ref_err = H.plane_errors(ref["u"], fine, u0)
    err = H.plane_errors(got["u"], fine, u0)
    print(f"{kind} n={n}: against all {n} parcels of a fine fixed-step run: restatement {ref_err}, device {err}")
    assert (~same).sum() <= 0.05 * n, (~same).sum()
    assert np.all(err <= 2 * ref_err + 1e-12), (err, ref_err)
    assert worst <= 1e-13, worst
    return got


def test_decision_parity_all_inf(gpu_cloudy, oracle):
    """The two-Gamma order-2 plan (the bench's cfg3a matrix), 257 parcels, n over three decades: at most 5 % of the parcels differ
    from the restatement in (accepted, rejected); the others agree to 1e-13 (the asserted per-evaluation tolerance of the tensor
    paths) x the evaluations the parcel took, of |u0| + |want| per plane; every parcel agrees with a fine fixed-step run as in
    test_golovin_closed_form."""
    decision_parity(gpu_cloudy, oracle, "allinf", 257)


@pytest.mark.parametrize("n", [65, 257])
@pytest.mark.parametrize("kind", ["fixed", "moving"])
def test_decision_parity_thresholded(gpu_cloudy, oracle, kind, n):
    """The same with thresholds (5e-9, Inf) and with a MovingThreshold plan: lanes without a parcel and lanes whose parcel has
    finished sit through the barriers of the ranking.
    The batch has a populated rain mode (test_tsit5_adaptive_host.two_gamma_batch says why: with a nearly empty one the
    restatement itself does not resolve 1e-13 x evaluations)."""
    decision_parity(gpu_cloudy, oracle, kind, n)


# ---- 4. batch independence
def test_batch_independence_all_inf(gpu_cloudy, oracle):
    """All-Inf plans: a parcel's result does not depend on its neighbours -- every parcel of the n = 257 run is bit-equal to the
    same parcel in batches of 65 and alone (257 launches of one parcel)."""
    cloudy = gpu_cloudy
    par, op, plan = two_gamma_plan(cloudy, oracle, "allinf")
    u0 = H.two_gamma_batch(257)
    t_span = H.TWO_GAMMA_T["allinf"]
    whole = adaptive(cloudy, plan, u0, t_span)
    keys = ("u", "t", "dt", "accepted", "rejected", "status")

    def check(lo, hi):
        part = adaptive(cloudy, plan, np.ascontiguousarray(u0[:, lo:hi]), t_span)
        for k in keys:
            a, b = np.ascontiguousarray(whole[k][..., lo:hi]), np.ascontiguousarray(part[k])
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (k, lo, hi)

    for lo in range(0, 257, 65):
        check(lo, min(lo + 65, 257))
    for i in range(257):
        check(i, i + 1)


# ---- 5. the budget
def test_max_steps_budget(gpu_cloudy, oracle):
    """max_steps = 3: the slow parcels stop with status 1, accepted + rejected == 3 and t_reached < t_span, in the state the
    restatement stopped the same way reaches; parcels that finish within 3 attempts have status 0.

    A parcel stopped by the budget does not land on t_span: its t_reached is a sum of controller proposals, and the error
    estimate behind a proposal is a difference of stage derivatives that cancels to reltol x EEst of the state, so its rounding
    noise is eps / (reltol EEst) relative and a proposal carries 0.14 of it (beta1).  The restatement alone, its right-hand side
    multiplied by 1 +- 1e-15 per entry, moves its own t_reached by 2.2e-7 relative and its state by 8.1e-10 x evaluations -- all of
    it |f| |dt|: 2.8e-16 x evaluations remain.  So the states are compared where each stopped, |got - want| <= |f(want)| |t_got -
    t_want| + 1e-13 x evaluations of |u0| + |want|, and t_reached to 1e-5 relative: two orders above the restatement's own response
    to that noise (the device's right-hand side differs from the oracle's by more than one last bit), far below any error of a
    step size that is not rounding.  Measured on MI355X without the drift term: 8.2e-10 x evaluations."""
    cloudy = gpu_cloudy
    par, op, plan = two_gamma_plan(cloudy, oracle, "allinf")
    u0, ref = H.two_gamma_reference_cached("allinf", 257, 3)
    t_span = H.TWO_GAMMA_T["allinf"]
    got = adaptive(cloudy, plan, u0, t_span, max_steps=3)
    slow = ref["status"] == 1
    assert 5 <= slow.sum() < 257
    assert np.array_equal(got["status"], ref["status"])
    assert np.all((got["accepted"] + got["rejected"])[slow] == 3) and np.all(got["t"][slow] < t_span)
    assert np.all(got["t"][~slow] == t_span) and np.all((got["accepted"] + got["rejected"])[~slow] <= 3)
    same = same_counts(got, ref)
    assert (~same).sum() <= 0.05 * 257
    dt_rel = np.abs(got["t"] - ref["t"]) / ref["t"]
    drift = np.abs(oracle.rhs_coal_batch(op, ref["u"])) * np.abs(got["t"] - ref["t"])
    excess = np.maximum(np.abs(got["u"] - ref["u"]) - 1.001 * drift, 0.0)
    rel = excess / np.maximum(np.abs(u0) + np.abs(ref["u"]), 1e-300) / ref["evals"]
    print(f"max_steps = 3: {slow.sum()} parcels stopped early; t_reached within {dt_rel[same].max():.2e} of the restatement's, the "
          f"state beyond |f| |dt| within {rel[:, same].max():.2e} x evaluations")
    assert dt_rel[same].max() <= 1e-5, dt_rel[same].max()
    assert rel[:, same].max() <= 1e-13, rel[:, same].max()


# ---- 6. warm start, automatic first step, in place
def test_warm_start_and_in_place(gpu_cloudy, oracle):
    cloudy = gpu_cloudy
    par, op, plan = golovin_plan(cloudy, oracle, "gamma")
    u0 = H.golovin_batch("gamma", 257)
    first = adaptive(cloudy, plan, u0, H.GOLOVIN_T)
    assert np.all(first["status"] == 0) and np.all(first["dt"] > 0) and np.all(np.isfinite(first["dt"]))
    # the next model step from the returned dt: no parcel's first step is rejected (one attempt each: accepted, or status 0)
    second = adaptive(cloudy, plan, first["u"], H.GOLOVIN_T, dt_in=first["dt"], max_steps=1)
    assert np.all(second["rejected"] == 0) and np.all(second["accepted"] == 1)
    # ... and the whole second step takes no more attempts than from a cold start
    warm = adaptive(cloudy, plan, first["u"], H.GOLOVIN_T, dt_in=first["dt"])
    cold = adaptive(cloudy, plan, first["u"], H.GOLOVIN_T)
    print(f"second model step: {warm['accepted'].sum() + warm['rejected'].sum()} attempts warm, "
          f"{cold['accepted'].sum() + cold['rejected'].sum()} cold; rejected {warm['rejected'].sum()} / {cold['rejected'].sum()}")
    assert np.all(warm["status"] == 0)
    assert (warm["accepted"] + warm["rejected"]).sum() <= (cold["accepted"] + cold["rejected"]).sum()
    # without dt_dev the automatic guess is used: the same bits as with a dt_dev of zeros
    auto = adaptive(cloudy, plan, u0, H.GOLOVIN_T, dt_in=None)
    assert auto["dt"] is None
    for k in ("u", "t", "accepted", "rejected", "status"):
        assert np.array_equal(auto[k].view(np.uint8), first[k].view(np.uint8)), k
    # opts.dt_init reaches the kernel: a first step of t_span / 1000 costs more attempts than the automatic one
    small = adaptive(cloudy, plan, u0, H.GOLOVIN_T, dt_init=H.GOLOVIN_T / 1000, dt_in=None)
    assert np.all(small["status"] == 0) and small["accepted"].min() >= 3
    # in place equals out of place bit for bit
    inplace = adaptive(cloudy, plan, u0, H.GOLOVIN_T, in_place=True)
    for k in ("u", "t", "dt", "accepted", "rejected", "status"):
        assert np.array_equal(inplace[k].view(np.uint8), first[k].view(np.uint8)), k
    # t_span = 0: the input copied, zero counts
    zero = adaptive(cloudy, plan, u0, 0.0)
    assert np.array_equal(zero["u"], u0) and np.all(zero["t"] == 0) and not zero["accepted"].any() and not zero["status"].any()
    # the Python wrapper
    u = dev(cloudy, u0)
    acc, rej, status, t = cloudy.solve_tsit5_adaptive(par, u, H.GOLOVIN_T, info=True)
    assert np.array_equal(acc, first["accepted"]) and np.array_equal(rej, first["rejected"]) and np.all(t == H.GOLOVIN_T)
    assert np.array_equal(u.to_numpy(), first["u"])
    with pytest.raises(RuntimeError, match=r"of 257 parcels did not reach t_span; the first is parcel \d+"):
        cloudy.solve_tsit5_adaptive(par, dev(cloudy, u0), H.GOLOVIN_T, max_steps=2, info=True)


# ---- 7. float planes
@pytest.mark.parametrize("kind", ["allinf", "fixed"])
def test_float_planes(gpu_cloudy, oracle, kind):
    """A CLOUDY_F32 plan from float-rounded input against the fp64 plan from the same rounded input: state and control are in
    fp64 registers either way, so the float result is the fp64 result rounded once (to float rounding of the output: half an
    ulp, 2^-24 relative)."""
    cloudy = gpu_cloudy
    _, _, plan64 = two_gamma_plan(cloudy, oracle, kind)
    _, _, plan32 = two_gamma_plan(cloudy, oracle, kind, dtype=1)
    u32 = H.two_gamma_batch(257, kind=kind).astype(np.float32)
    t_span = H.TWO_GAMMA_T[kind]
    want = adaptive(cloudy, plan64, u32.astype(np.float64), t_span)
    got = adaptive(cloudy, plan32, u32, t_span)
    assert got["u"].dtype == np.float32 and np.all(got["status"] == 0)
    assert np.array_equal(got["accepted"], want["accepted"]) and np.array_equal(got["rejected"], want["rejected"])
    fin = np.isfinite(want["u"].astype(np.float32))
    err = np.abs(got["u"].astype(np.float64) - want["u"])[fin] / np.abs(want["u"])[fin]
    print(f"float planes, {kind}: max relative difference {err.max():.2e}")
    assert err.max() <= 2.0 ** -24, err.max()


# ---- 8. refusals
def test_refusals_name_the_alternative_and_leave_the_output_alone(gpu_cloudy, oracle):
    cloudy = gpu_cloudy
    L, E = cloudy.lib(), cloudy._lib
    u0 = H.two_gamma_batch(65)
    _, _, fast = two_gamma_plan(cloudy, oracle, "fixed", dtype=2)          # CLOUDY_F32_FAST
    _, _, aot = two_gamma_plan(cloudy, oracle, "allinf", specialize=-1)    # no plan-time compilation
    numerical = cloudy.numerical_plan([1, 1], cloudy.LinearKernelFunction(5e-3), bench.NORMS, 10, quad_mode=cloudy.QUAD_FIXED)
    for what, plan, batch in (("CLOUDY_F32_FAST", fast, u0.astype(np.float32)), ("specialize = -1", aot, u0), ("numerical", numerical, u0)):
        got = adaptive(cloudy, plan, batch, 1e-3, expect=E.EUNSUPPORTED)
        msg = L.cloudy_last_error().decode()
        assert "cloudy_tsit5_steps" in msg, (what, msg)
        if batch.dtype == np.float64:
            assert np.all(got["u"].view(np.uint64) == SENTINEL), what
        else:
            assert np.all(np.isnan(got["u"])), what
        assert not got["accepted"].any() and np.all(got["t"].view(np.uint64) == SENTINEL)
