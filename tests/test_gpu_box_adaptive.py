"""GPU tests of cloudy_box_tsit5_adaptive (csrc/adaptive_box.hpp): per-parcel adaptive Tsit5 of du/dt = [coal](u) + [cond](u; s, xi).
The reference is the NumPy restatement tsit5_restated.adaptive_tsit5 (without and with t_save) driven by the unchanged oracle's
rhs_coal_batch + rhs_condensation_batch (tests/test_box_adaptive_host.py holds the batches and measures the restatement on them), the closed form of
a Monodisperse mode under condensation, the fixed-step tableau (_tsit5_host) at a fine step, and cloudy_tsit5_adaptive itself.

Run with `-m gpu`.  Batch sizes 1, 65 and 257: a single parcel, a partial wave past one wave, a partial workgroup past one
workgroup of 256 threads -- the 512-thread kernel of COAL | COND on the `fixed` plan still runs a single, partly filled workgroup at
257 (tests/test_gpu_ranked_adaptive.py runs it at 513 and 1025)."""
import functools

import numpy as np
import pytest

import bench
import test_box_adaptive_host as B
import test_tsit5_adaptive_host as H
from gpu_support import INF, SENTINEL, SIZES, _tsit5_host, adaptive, bits_equal, box_adaptive, dev, is_blank, make_case, same_counts, two_gamma_plan
from tsit5_restated import adaptive_tsit5, plane_norms, save_times

pytestmark = pytest.mark.gpu

KEYS = ("u", "t", "dt", "accepted", "rejected", "status")
COAL, COND = 1, 2


@functools.lru_cache(maxsize=None)
def cond_plan(cloudy, oracle):
    par, op, _ = make_case(cloudy, oracle, [2], [[1.0]], (INF,), bench.NORMS)
    return par, op, par.coal_data.plan([2])


@functools.lru_cache(maxsize=None)
def box_runs(cloudy, oracle, kind, n):
    """(without snapshots, with the twelve save times) on a two-Gamma batch with both sources, once per session"""
    _, _, plan = two_gamma_plan(cloudy, oracle, kind)
    u0 = H.two_gamma_batch(n, kind=kind)
    t_span, s = H.TWO_GAMMA_T[kind], B.box_supersaturation(n)
    return (u0, box_adaptive(cloudy, plan, u0, t_span, s, B.XI_BOX, ld=n + 15),
            box_adaptive(cloudy, plan, u0, t_span, s, B.XI_BOX, times=save_times(t_span), ld=n + 15))


# ---- 1. closed form
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("reltol", H.TOLS)
def test_condensation_closed_form(gpu_cloudy, oracle, reltol, n):
    """One Monodisperse mode, condensation only, a supersaturation per parcel through s_dev, ld = n + 15, out of place, against
    M1(t) = n (x0^(2/3) + 2 c xi s t)^(3/2): per plane the device's maximum of |got - exact| / (|u0| + |exact|) is at most twice the
    restatement's on the same batch + 1e-12 (the rule of test_golovin_closed_form); M0 has the bits of the input; every status 0,
    t_reached == t_span bit for bit; padding columns and input untouched."""
    cloudy = gpu_cloudy
    _, _, plan = cond_plan(cloudy, oracle)
    u0, s, exact, ref, ref_err = B.cond_case(n, reltol)
    got = box_adaptive(cloudy, plan, u0, B.COND_T, s, B.XI_COND, sources=COND, reltol=reltol, ld=n + 15)
    err = H.plane_errors(got["u"], exact, u0)
    print(f"reltol={reltol:g} n={n}: restatement's max error per plane {ref_err}, device's {err}; "
          f"{(~same_counts(got, ref)).sum()} parcels differ in (accepted, rejected)")
    assert np.all(got["status"] == 0) and np.all(got["t"] == B.COND_T)
    assert np.all(err <= 2 * ref_err + 1e-12), (err, ref_err)
    assert bits_equal(got["u"][0], u0[0])
    assert np.all(is_blank(got["pad"])) and np.array_equal(got["u_in"], got["buf"])


# ---- 2. decision parity
@functools.lru_cache(maxsize=None)
def fine_reference(kind, n):
    """every parcel by the fixed-step tableau on the combined oracle right-hand side, step counts as
    test_gpu_tsit5_adaptive.fine_reference (50 all-Inf, 25 thresholded), once per session"""
    from oracle import cloudy_oracle as oracle

    n_fine = 50 if kind == "allinf" else 25
    with np.errstate(all="ignore"):
        return _tsit5_host(B.box_rhs(oracle, kind, n), H.two_gamma_batch(n, kind=kind), H.TWO_GAMMA_T[kind] / n_fine, n_fine)


@pytest.mark.parametrize("kind,n", [("allinf", 257), ("fixed", 65), ("fixed", 257), ("moving", 65), ("moving", 257)])
def test_decision_parity(gpu_cloudy, oracle, kind, n):
    """COAL | COND on the two-Gamma batches of test_box_adaptive_host: at most 5 % of the parcels differ from the restatement in
    (accepted, rejected); the others agree per plane to 1e-11 x evaluations of |u0| + |want| -- the per-evaluation bound the project
    asserts for the condensation right-hand side (tests/test_gpu_box_sources.py); the measured value is printed; every parcel,
    flipped or not, agrees with a fine fixed-step run to 2 x the restatement's error + 1e-12."""
    u0, got, _ = box_runs(gpu_cloudy, oracle, kind, n)
    _, ref = B.box_reference_cached(kind, n)
    assert np.all(ref["status"] == 0) and np.all(got["status"] == 0) and np.all(got["t"] == H.TWO_GAMMA_T[kind])
    same = same_counts(got, ref)
    rel = np.abs(got["u"] - ref["u"]) / np.maximum(np.abs(u0) + np.abs(ref["u"]), 1e-300) / ref["evals"]
    worst = rel[:, same].max()
    fine = fine_reference(kind, n)
    assert np.isfinite(fine).all()
    ref_err, err = H.plane_errors(ref["u"], fine, u0), H.plane_errors(got["u"], fine, u0)
    print(f"{kind} n={n}: {(~same).sum()} of {n} parcels differ in (accepted, rejected); the others agree to {worst:.2e} x evaluations; "
          f"against a fine fixed-step run: restatement {ref_err}, device {err}")
    assert (~same).sum() <= 0.05 * n, (~same).sum()
    assert worst <= B.TOL_EVAL, worst
    assert np.all(err <= 2 * ref_err + 1e-12), (err, ref_err)
    assert np.all(is_blank(got["pad"])) and np.array_equal(got["u_in"], got["buf"])


# ---- 3. sources
@pytest.mark.parametrize("kind", ["allinf", "fixed"])
def test_sources(gpu_cloudy, oracle, kind):
    """sources = COAL has the bits of cloudy_tsit5_adaptive in u, dt, t and info; a scalar s those of an s_dev filled with it; in
    place equals out of place; t_span = 0 copies the input with zero counts."""
    cloudy = gpu_cloudy
    _, _, plan = two_gamma_plan(cloudy, oracle, kind)
    n = 65
    u0 = H.two_gamma_batch(n, kind=kind)
    t_span = H.TWO_GAMMA_T[kind]
    base = adaptive(cloudy, plan, u0, t_span, ld=n + 15)
    coal = box_adaptive(cloudy, plan, u0, t_span, 0.05, B.XI_BOX, sources=COAL, ld=n + 15)
    for k in KEYS:
        assert bits_equal(coal[k], base[k]), k
    scalar = box_adaptive(cloudy, plan, u0, t_span, 0.03, B.XI_BOX, ld=n + 15)
    filled = box_adaptive(cloudy, plan, u0, t_span, np.full(n, 0.03), B.XI_BOX, ld=n + 15)
    inplace = box_adaptive(cloudy, plan, u0, t_span, 0.03, B.XI_BOX, ld=n + 15, in_place=True)
    assert np.all(scalar["status"] == 0) and not bits_equal(scalar["u"], base["u"])
    for k in KEYS:
        assert bits_equal(filled[k], scalar[k]), k
        assert bits_equal(inplace[k], scalar[k]), k
    zero = box_adaptive(cloudy, plan, u0, 0.0, 0.03, B.XI_BOX, times=(0.0,), ld=n + 15)
    assert bits_equal(zero["u"], u0) and np.all(zero["t"] == 0) and not zero["accepted"].any() and not zero["rejected"].any()
    assert not zero["status"].any() and bits_equal(zero["saved"][0], u0)


# ---- 4. batch independence of the barrier-free instances
@pytest.mark.parametrize("which", ["cond", "coalcond_allinf"])
def test_batch_independence(gpu_cloudy, oracle, which):
    """COND and COAL | COND all-Inf: the 257-parcel run is bit-equal to its 65-parcel chunks and to 8 parcels run alone, the
    slowest parcel and a one-step parcel among them."""
    cloudy = gpu_cloudy
    if which == "cond":
        _, _, plan = cond_plan(cloudy, oracle)
        u0, s, _, _, _ = B.cond_case(257, 1e-9)
        args = dict(t_span=B.COND_T, xi=B.XI_COND, sources=COND, reltol=1e-9)
    else:
        _, _, plan = two_gamma_plan(cloudy, oracle, "allinf")
        u0, s = H.two_gamma_batch(257), B.box_supersaturation(257)
        args = dict(t_span=H.TWO_GAMMA_T["allinf"], xi=B.XI_BOX)
    whole = box_adaptive(cloudy, plan, u0, s=s, **args)
    attempts = whole["accepted"] + whole["rejected"]
    assert attempts.min() == 1 and attempts.max() >= 5

    def check(idx):
        part = box_adaptive(cloudy, plan, np.ascontiguousarray(u0[:, idx]), s=s[idx], **args)
        for k in KEYS:
            assert bits_equal(whole[k][..., idx], part[k]), (k, idx)

    for lo in range(0, 257, 65):
        check(slice(lo, min(lo + 65, 257)))
    alone = [int(np.argmax(attempts)), int(np.argmin(attempts)), 0, 63, 64, 128, 255, 256]
    for i in alone:
        check(slice(i, i + 1))


# ---- 5. dense output
@pytest.mark.parametrize("case", ["cond", "allinf", "fixed"])
def test_dense_output(gpu_cloudy, oracle, case):
    """The twelve save times: u_out, dt, t, info have the bits of the n_save = 0 call; the snapshot at 0 has the input's bits, the
    one at t_span u_out's; for the parcels with the restatement's counts (at least 95 %) every snapshot agrees with
    adaptive_tsit5 with t_save to 1e-11 x evaluations of |u0| + |want| (the bound of test_gpu_tsit5_saveat with this file's tolerance);
    padding untouched."""
    cloudy = gpu_cloudy
    if case == "cond":
        _, _, plan = cond_plan(cloudy, oracle)
        n = 257
        u0, s, _, ref, _ = B.cond_case(n, 1e-6, True)
        base = box_adaptive(cloudy, plan, u0, B.COND_T, s, B.XI_COND, sources=COND, ld=n + 15)
        got = box_adaptive(cloudy, plan, u0, B.COND_T, s, B.XI_COND, sources=COND, times=save_times(B.COND_T), ld=n + 15)
    else:
        n = 257 if case == "allinf" else 65
        u0, base, got = box_runs(cloudy, oracle, case, n)
        _, ref = B.box_reference_cached(case, n, saveat=True)
    for k in KEYS:
        assert bits_equal(got[k], base[k]), k
    assert np.all(got["status"] == 0) and np.isfinite(got["saved"]).all()
    assert bits_equal(got["saved"][0], u0) and bits_equal(got["saved"][-1], got["u"])
    assert np.all(is_blank(got["saved_pad"])) and np.all(is_blank(got["pad"]))
    same = same_counts(got, ref)
    assert (~same).sum() <= 0.05 * n, (~same).sum()
    rel = np.abs(got["saved"] - ref["saved"]) / np.maximum(np.abs(u0)[None] + np.abs(ref["saved"]), 1e-300) / ref["evals"][None, None, :]
    worst = rel[:, :, same].max(axis=(1, 2))
    print(f"{case} n={n}: {(~same).sum()} parcels differ in (accepted, rejected); the snapshots of the others agree to "
          f"{worst.max():.2e} x evaluations")
    assert worst.max() <= B.TOL_EVAL, worst


def test_budget_leaves_nan_beyond_the_time_reached(gpu_cloudy, oracle):
    """max_steps = 3 on the all-Inf batch with both sources: stopped parcels have status 1 and a quiet NaN in every snapshot beyond
    t_reached and finite values before it."""
    cloudy = gpu_cloudy
    _, _, plan = two_gamma_plan(cloudy, oracle, "allinf")
    u0, s = H.two_gamma_batch(257), B.box_supersaturation(257)
    t_span = H.TWO_GAMMA_T["allinf"]
    ts = save_times(t_span)
    got = box_adaptive(cloudy, plan, u0, t_span, s, B.XI_BOX, times=ts, max_steps=3, ld=257 + 15)
    slow = got["status"] == 1
    assert 5 <= slow.sum() < 257 and np.all(got["status"][~slow] == 0) and np.all(got["t"][slow] < t_span)
    beyond = ts[:, None] > got["t"][None, :]
    assert beyond[:, slow].any() and (~beyond[:, slow]).any() and not beyond[:, ~slow].any()
    nan, fin = np.isnan(got["saved"]), np.isfinite(got["saved"])
    assert np.all(nan.all(axis=1) == beyond) and np.all(fin.all(axis=1) == ~beyond)
    assert np.all(is_blank(got["saved_pad"]))


# ---- 6. warm start
def test_warm_start(gpu_cloudy, oracle):
    cloudy = gpu_cloudy
    _, _, plan = cond_plan(cloudy, oracle)
    u0, s, _, _, _ = B.cond_case(257, 1e-6)
    args = dict(s=s, xi=B.XI_COND, sources=COND)
    first = box_adaptive(cloudy, plan, u0, B.COND_T, **args)
    assert np.all(first["status"] == 0) and np.all(first["dt"] > 0) and np.all(np.isfinite(first["dt"]))
    # the next model step from the returned dt: no parcel's first step is rejected (one attempt each: accepted, or status 0)
    second = box_adaptive(cloudy, plan, first["u"], B.COND_T, dt_in=first["dt"], max_steps=1, **args)
    assert np.all(second["rejected"] == 0) and np.all(second["accepted"] == 1)
    warm = box_adaptive(cloudy, plan, first["u"], B.COND_T, dt_in=first["dt"], **args)
    cold = box_adaptive(cloudy, plan, first["u"], B.COND_T, **args)
    print(f"second model step: {warm['accepted'].sum() + warm['rejected'].sum()} attempts warm, "
          f"{cold['accepted'].sum() + cold['rejected'].sum()} cold; rejected {warm['rejected'].sum()} / {cold['rejected'].sum()}")
    assert np.all(warm["status"] == 0)
    assert (warm["accepted"] + warm["rejected"]).sum() <= (cold["accepted"] + cold["rejected"]).sum()


# ---- 7. float planes
@pytest.mark.parametrize("kind", ["allinf", "fixed"])
def test_float_planes(gpu_cloudy, oracle, kind):
    """A CLOUDY_F32 plan against the fp64 plan from the same float-rounded input: the same counts, the state within 2^-24 relative."""
    cloudy = gpu_cloudy
    _, _, plan64 = two_gamma_plan(cloudy, oracle, kind)
    _, _, plan32 = two_gamma_plan(cloudy, oracle, kind, dtype=1)
    n = 257 if kind == "allinf" else 65
    u32 = H.two_gamma_batch(n, kind=kind).astype(np.float32)
    t_span, s = H.TWO_GAMMA_T[kind], B.box_supersaturation(n)
    want = box_adaptive(cloudy, plan64, u32.astype(np.float64), t_span, s, B.XI_BOX, ld=n + 15)
    got = box_adaptive(cloudy, plan32, u32, t_span, s, B.XI_BOX, ld=n + 15)
    assert got["u"].dtype == np.float32 and np.all(got["status"] == 0)
    assert np.array_equal(got["accepted"], want["accepted"]) and np.array_equal(got["rejected"], want["rejected"])
    fin = np.isfinite(want["u"].astype(np.float32))
    err = np.abs(got["u"].astype(np.float64) - want["u"])[fin] / np.abs(want["u"])[fin]
    print(f"float planes, {kind}: max relative difference {err.max():.2e}")
    assert err.max() <= 2.0 ** -24, err.max()
    assert np.all(is_blank(got["pad"]))


# ---- 8. served and refused
def test_served_and_refused(gpu_cloudy, oracle):
    """A NumericalCoalStyle plan with COND alone runs and agrees with the restatement.  (The closed-form batch is a Monodisperse mode,
    which no NumericalCoalStyle plan can hold -- plan creation refuses it, as the reference has no density for it -- so the batch is
    the all-Inf two-Gamma one with the condensation right-hand side alone, 65 parcels, t_span = 200, xi = 1e-8.)  With COAL | COND the
    plan answers CLOUDY_EUNSUPPORTED, as a CLOUDY_F32_FAST plan and a plan without plan-time compilation do, each naming the
    stage-by-stage alternative and leaving the sentinel-filled outputs alone."""
    cloudy = gpu_cloudy
    L, E = cloudy.lib(), cloudy._lib
    numerical = cloudy.numerical_plan([1, 1], cloudy.LinearKernelFunction(5e-3), bench.NORMS, 10, quad_mode=cloudy.QUAD_FIXED)
    op, _, _, _ = H.two_gamma_case(oracle, "allinf")
    u0, s = H.two_gamma_batch(65), B.box_supersaturation(65)
    ref = adaptive_tsit5(lambda u: oracle.rhs_condensation_batch(op, B.XI_COND, s, u), u0, B.COND_T,
                         dict(reltol=1e-6, abstol=1e-9, max_steps=10000, plane_norms=plane_norms((3, 3))))
    got = box_adaptive(cloudy, numerical, u0, B.COND_T, s, B.XI_COND, sources=COND, ld=80)
    assert np.all(ref["status"] == 0) and np.all(got["status"] == 0) and np.all(got["t"] == B.COND_T)
    same = same_counts(got, ref)
    rel = np.abs(got["u"] - ref["u"]) / np.maximum(np.abs(u0) + np.abs(ref["u"]), 1e-300) / ref["evals"]
    print(f"numerical plan, COND: {(~same).sum()} of 65 parcels differ in (accepted, rejected); the others agree to "
          f"{rel[:, same].max():.2e} x evaluations; the state moved by {(np.abs(ref['u'] - u0) / np.abs(u0)).max():.2e}")
    assert (~same).sum() <= 0.05 * 65 and rel[:, same].max() <= B.TOL_EVAL
    assert bits_equal(got["u"][[0, 3]], u0[[0, 3]]) and np.all(is_blank(got["pad"]))
    g0 = H.two_gamma_batch(65)
    _, _, fast = two_gamma_plan(cloudy, oracle, "fixed", dtype=2)          # CLOUDY_F32_FAST
    _, _, aot = two_gamma_plan(cloudy, oracle, "allinf", specialize=-1)    # no plan-time compilation
    for what, plan, batch in (("numerical", numerical, g0), ("CLOUDY_F32_FAST", fast, g0.astype(np.float32)), ("specialize = -1", aot, g0)):
        ts = save_times(1e-3)
        got = box_adaptive(cloudy, plan, batch, 1e-3, 0.05, B.XI_BOX, times=ts, expect=E.EUNSUPPORTED)
        msg = L.cloudy_last_error().decode()
        assert "cloudy_cond_evap" in msg and "stage by stage" in msg, (what, msg)
        assert np.all(is_blank(got["saved_bits"])) and np.all(is_blank(got["u"])), what
        assert not got["accepted"].any() and np.all(got["t"].view(np.uint64) == SENTINEL)


# ---- 9. the Python wrapper
def test_python_wrapper(gpu_cloudy, oracle):
    cloudy = gpu_cloudy
    par, _, plan = two_gamma_plan(cloudy, oracle, "allinf")
    n = 257
    u0, s = H.two_gamma_batch(n), B.box_supersaturation(n)
    t_span = H.TWO_GAMMA_T["allinf"]
    ts = save_times(t_span)
    want = box_adaptive(cloudy, plan, u0, t_span, s, B.XI_BOX, times=ts)
    s_d = dev(cloudy, s[None, :])
    u = dev(cloudy, u0)
    acc, rej, status, t = cloudy.solve_box_tsit5_adaptive(par, u, t_span, B.XI_BOX, s_d, info=True)
    assert bits_equal(u.to_numpy(), want["u"]) and not status.any() and np.all(t == t_span)
    assert np.array_equal(acc, want["accepted"]) and np.array_equal(rej, want["rejected"])
    u = dev(cloudy, u0)
    saved, acc, rej, status, t = cloudy.solve_box_tsit5_adaptive(par, u, t_span, B.XI_BOX, s_d, saveat=ts, info=True)
    assert bits_equal(saved.to_numpy().reshape(len(ts), 6, n), want["saved"]) and bits_equal(u.to_numpy(), want["u"])
    out = cloudy.DeviceArray.zeros(6, n)
    assert cloudy.solve_box_tsit5_adaptive(par, dev(cloudy, u0), t_span, B.XI_BOX, s_d, out=out) is out
    assert bits_equal(out.to_numpy(), want["u"])
    with pytest.raises(RuntimeError, match=r"of 257 parcels did not reach t_span; the first is parcel \d+"):
        cloudy.solve_box_tsit5_adaptive(par, dev(cloudy, u0), t_span, B.XI_BOX, s_d, max_steps=2, info=True)
