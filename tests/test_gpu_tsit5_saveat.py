"""GPU tests of cloudy_tsit5_adaptive_saveat (csrc/adaptive.hpp, SAVE = true): the per-parcel adaptive Tsit5 with snapshots at the
caller's save times.  The reference is the NumPy restatement of tests/test_tsit5_saveat_host.py driven by the unchanged oracle's
right-hand side, the closed form of the single-mode Golovin box at the save times, and cloudy_tsit5_adaptive itself: saving may not
move a bit of the integration.

Run with `-m gpu`.  Batches, plans and t_span are those of tests/test_gpu_tsit5_adaptive.py (1, 65 and 257 parcels in buffers of
leading dimension n + 15; thresholded plans at 65 parcels: their oracle is slow); the save times are the twelve of
tsit5_restated.SAVE_FRACS."""
import functools

import numpy as np
import pytest

import test_tsit5_adaptive_host as H
import test_tsit5_saveat_host as S
from gpu_support import SENTINEL, SIZES, adaptive, bits_equal, dev, golovin_plan, is_blank, same_counts, saveat, two_gamma_plan
from tsit5_restated import SAVE_FRACS, save_times

pytestmark = pytest.mark.gpu

KEYS = ("u", "t", "dt", "accepted", "rejected", "status")
CASES = (("allinf", 257), ("fixed", 65), ("moving", 65))


@functools.lru_cache(maxsize=None)
def golovin_reference(dist, n, reltol):
    from oracle import cloudy_oracle

    return S.golovin_saveat_case(cloudy_oracle, dist, n, reltol)


@functools.lru_cache(maxsize=None)
def device_runs(cloudy, oracle, kind, n):
    """(cloudy_tsit5_adaptive, cloudy_tsit5_adaptive_saveat at the twelve save times) on a two-Gamma batch, once per session"""
    _, _, plan = two_gamma_plan(cloudy, oracle, kind)
    u0 = H.two_gamma_batch(n, kind=kind)
    t_span = H.TWO_GAMMA_T[kind]
    return u0, adaptive(cloudy, plan, u0, t_span, ld=n + 15), saveat(cloudy, plan, u0, t_span, save_times(t_span), ld=n + 15)


# ---- 1. closed form
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("reltol", H.TOLS)
@pytest.mark.parametrize("dist", ["gamma", "exponential"])
def test_golovin_closed_form_at_the_save_times(gpu_cloudy, oracle, dist, reltol, n):
    """Single-mode Golovin boxes against the closed form at every save time: per plane the device's maximum over all snapshots
    of |got - exact| / (|u0| + |exact|) is at most twice the restatement's + 1e-12 (the rule of test_golovin_closed_form); every
    status is 0."""
    cloudy = gpu_cloudy
    _, _, plan = golovin_plan(cloudy, oracle, dist)
    u0, ts, ref = golovin_reference(dist, n, reltol)
    got = saveat(cloudy, plan, u0, H.GOLOVIN_T, ts, reltol=reltol, ld=n + 15)
    ref_err = S.golovin_snapshot_errors(ref["saved"], u0, ts)
    err = S.golovin_snapshot_errors(got["saved"], u0, ts)
    print(f"{dist} reltol={reltol:g} n={n}: largest error over the snapshots per plane: restatement {ref_err}, device {err}")
    assert np.all(got["status"] == 0) and np.all(got["t"] == H.GOLOVIN_T)
    assert np.isfinite(got["saved"]).all()
    assert np.all(err <= 2 * ref_err + 1e-12), (err, ref_err)
    assert bits_equal(got["saved"][0], u0) and bits_equal(got["saved"][-1], got["u"])
    assert np.all(is_blank(got["saved_pad"]))


# ---- 2. saving does not disturb the integration
@pytest.mark.parametrize("kind,n", CASES)
def test_saving_does_not_disturb_the_integration(gpu_cloudy, oracle, kind, n):
    """u, t, dt, accepted, rejected and status of the new entry point are those of cloudy_tsit5_adaptive on the same batch, bit for
    bit: with the twelve save times, with n_save = 0 (NULL pointers), and in place."""
    cloudy = gpu_cloudy
    _, _, plan = two_gamma_plan(cloudy, oracle, kind)
    u0, base, got = device_runs(cloudy, oracle, kind, n)
    t_span = H.TWO_GAMMA_T[kind]
    assert np.all(base["status"] == 0) and (base["accepted"] + base["rejected"]).max() >= 3
    for k in KEYS:
        assert bits_equal(got[k], base[k]), k
    none = saveat(cloudy, plan, u0, t_span, (), ld=n + 15)
    inplace = saveat(cloudy, plan, u0, t_span, save_times(t_span), ld=n + 15, in_place=True)
    for k in KEYS:
        assert bits_equal(none[k], base[k]), k
        assert bits_equal(inplace[k], base[k]), k
    assert np.all(is_blank(none["saved_bits"]))          # (nothing to save: the buffer is not touched)
    assert bits_equal(inplace["saved"], got["saved"])


# ---- 3. end points
@pytest.mark.parametrize("kind,n", CASES)
def test_end_points_padding_and_input(gpu_cloudy, oracle, kind, n):
    """The snapshot at t_span has the bits of u_out, the one at 0 those of u_in; the columns n .. ld of every snapshot plane and
    of u_out keep the sentinel; u_in is untouched out of place."""
    u0, base, got = device_runs(gpu_cloudy, oracle, kind, n)
    assert got["saved"].shape == (len(SAVE_FRACS), 6, n) and np.isfinite(got["saved"]).all()
    assert bits_equal(got["saved"][-1], got["u"])
    assert bits_equal(got["saved"][0], u0)
    assert got["saved_pad"].shape[2] == 15 and np.all(is_blank(got["saved_pad"])) and np.all(is_blank(got["pad"]))
    assert bits_equal(got["u_in"], got["buf"])


# ---- 4. parity with the restatement
@pytest.mark.parametrize("kind,n", CASES)
def test_snapshot_parity_with_the_restatement(gpu_cloudy, oracle, kind, n):
    """At most 5 % of the parcels differ from the restatement in (accepted, rejected) (as decision_parity; the restatement
    integrates as the one without does -- test_tsit5_saveat_host -- whose own sensitivity on these batches the existing tests
    bound); for the others EVERY snapshot agrees to 1e-13 x the evaluations the parcel took, of |u0| + |want| per plane: the bound
    already asserted for the final state -- the interpolant adds a few dozen FMAs with coefficients <= 48, a rounding contribution
    of order 1e-14 of |h k|."""
    u0, base, got = device_runs(gpu_cloudy, oracle, kind, n)
    _, ts, ref = S.two_gamma_saveat_cached(kind, n)
    assert np.all(ref["status"] == 0) and np.all(got["status"] == 0)
    same = same_counts(got, ref)
    assert (~same).sum() <= 0.05 * n, (~same).sum()
    rel = np.abs(got["saved"] - ref["saved"]) / np.maximum(np.abs(u0)[None] + np.abs(ref["saved"]), 1e-300) / ref["evals"][None, None, :]
    worst = rel[:, :, same].max(axis=(1, 2))
    print(f"{kind} n={n}: {(~same).sum()} of {n} parcels differ in (accepted, rejected); the snapshots of the others agree to "
          f"{worst.max():.2e} x evaluations (per save time: {worst})")
    assert worst.max() <= 1e-13, worst


# ---- 5. the budget
def test_budget_leaves_nan_beyond_the_time_reached(gpu_cloudy, oracle):
    """max_steps = 3 on the all-Inf batch: a parcel stopped with status 1 has NaN in all planes of every snapshot beyond the time
    it reached and finite values in the others; the parcels that finished have finite snapshots throughout."""
    cloudy = gpu_cloudy
    _, _, plan = two_gamma_plan(cloudy, oracle, "allinf")
    u0 = H.two_gamma_batch(257)
    t_span = H.TWO_GAMMA_T["allinf"]
    ts = save_times(t_span)
    got = saveat(cloudy, plan, u0, t_span, ts, max_steps=3, ld=257 + 15)
    base = adaptive(cloudy, plan, u0, t_span, max_steps=3, ld=257 + 15)
    for k in KEYS:
        assert bits_equal(got[k], base[k]), k
    slow = got["status"] == 1
    assert 5 <= slow.sum() < 257 and np.all(got["status"][~slow] == 0) and np.all(got["t"][slow] < t_span)
    beyond = ts[:, None] > got["t"][None, :]                    # (n_save, n)
    assert beyond[:, slow].any() and (~beyond[:, slow]).any() and not beyond[:, ~slow].any()
    nan, fin = np.isnan(got["saved"]), np.isfinite(got["saved"])
    assert np.all(nan.all(axis=1) == beyond) and np.all(fin.all(axis=1) == ~beyond)
    assert np.all(is_blank(got["saved_pad"]))


# ---- 6. batch independence
def test_batch_independence_all_inf(gpu_cloudy, oracle):
    """All-Inf plans: the snapshots of a parcel do not depend on its neighbours -- those of the n = 257 run are bit-equal to the same
    parcels in batches of 65, and to the first, the 65th and the last parcel alone."""
    cloudy = gpu_cloudy
    _, _, plan = two_gamma_plan(cloudy, oracle, "allinf")
    u0, _, whole = device_runs(cloudy, oracle, "allinf", 257)
    t_span = H.TWO_GAMMA_T["allinf"]

    def check(lo, hi):
        part = saveat(cloudy, plan, np.ascontiguousarray(u0[:, lo:hi]), t_span, save_times(t_span))
        assert bits_equal(whole["saved"][:, :, lo:hi], part["saved"]), (lo, hi)
        for k in KEYS:
            assert bits_equal(whole[k][..., lo:hi], part[k]), (k, lo, hi)

    for lo in range(0, 257, 65):
        check(lo, min(lo + 65, 257))
    for i in (0, 64, 256):
        check(i, i + 1)


# ---- 7. float planes
@pytest.mark.parametrize("kind", ["allinf", "fixed"])
def test_float_planes(gpu_cloudy, oracle, kind):
    """A CLOUDY_F32 plan from float-rounded input against the fp64 plan from the same rounded input: state, control and interpolant
    are in fp64 registers either way, so every float snapshot is the fp64 one rounded once (2^-24 relative); equal counts."""
    cloudy = gpu_cloudy
    _, _, plan64 = two_gamma_plan(cloudy, oracle, kind)
    _, _, plan32 = two_gamma_plan(cloudy, oracle, kind, dtype=1)
    n = 257 if kind == "allinf" else 65
    u32 = H.two_gamma_batch(n, kind=kind).astype(np.float32)
    t_span = H.TWO_GAMMA_T[kind]
    ts = save_times(t_span)
    want = saveat(cloudy, plan64, u32.astype(np.float64), t_span, ts, ld=n + 15)
    got = saveat(cloudy, plan32, u32, t_span, ts, ld=n + 15)
    assert got["saved"].dtype == np.float32 and np.all(got["status"] == 0)
    assert np.array_equal(got["accepted"], want["accepted"]) and np.array_equal(got["rejected"], want["rejected"])
    fin = np.isfinite(want["saved"].astype(np.float32))
    assert np.array_equal(np.isfinite(got["saved"]), fin)
    err = np.abs(got["saved"].astype(np.float64) - want["saved"])[fin] / np.abs(want["saved"])[fin]
    print(f"float planes, {kind}: max relative difference over the snapshots {err.max():.2e}")
    assert err.max() <= 2.0 ** -24, err.max()
    assert bits_equal(got["saved"][0], u32) and bits_equal(got["saved"][-1], got["u"])
    assert np.all(is_blank(got["saved_pad"]))


# ---- 8. refusals
def test_refusals_name_the_alternative_and_leave_every_output_alone(gpu_cloudy, oracle):
    cloudy = gpu_cloudy
    import bench

    L, E = cloudy.lib(), cloudy._lib
    u0 = H.two_gamma_batch(65)
    _, _, fast = two_gamma_plan(cloudy, oracle, "fixed", dtype=2)          # CLOUDY_F32_FAST
    _, _, aot = two_gamma_plan(cloudy, oracle, "allinf", specialize=-1)    # no plan-time compilation
    numerical = cloudy.numerical_plan([1, 1], cloudy.LinearKernelFunction(5e-3), bench.NORMS, 10, quad_mode=cloudy.QUAD_FIXED)
    for what, plan, batch in (("CLOUDY_F32_FAST", fast, u0.astype(np.float32)), ("specialize = -1", aot, u0), ("numerical", numerical, u0)):
        got = saveat(cloudy, plan, batch, 1e-3, save_times(1e-3), expect=E.EUNSUPPORTED)
        msg = L.cloudy_last_error().decode()
        assert "cloudy_tsit5_steps" in msg, (what, msg)
        assert np.all(is_blank(got["saved_bits"])), what
        assert np.all(is_blank(got["u"])), what
        assert not got["accepted"].any() and np.all(got["t"].view(np.uint64) == SENTINEL)


# ---- 9. the Python wrapper
def test_python_wrapper_returns_the_bits_of_the_c_call(gpu_cloudy, oracle):
    cloudy = gpu_cloudy
    par, _, plan = golovin_plan(cloudy, oracle, "gamma")
    u0 = H.golovin_batch("gamma", 257)
    ts = save_times(H.GOLOVIN_T)
    want = saveat(cloudy, plan, u0, H.GOLOVIN_T, ts)
    u = dev(cloudy, u0)
    saved, acc, rej, status, t = cloudy.solve_tsit5_adaptive_saveat(par, u, H.GOLOVIN_T, ts, info=True)
    assert saved.shape == (len(ts) * 3, 257) and saved.dtype == np.float64
    assert bits_equal(saved.to_numpy().reshape(len(ts), 3, 257), want["saved"])
    assert bits_equal(u.to_numpy(), want["u"])
    assert np.array_equal(acc, want["accepted"]) and np.array_equal(rej, want["rejected"]) and not status.any() and np.all(t == H.GOLOVIN_T)
    only = cloudy.solve_tsit5_adaptive_saveat(par, dev(cloudy, u0), H.GOLOVIN_T, ts)
    assert bits_equal(only.to_numpy(), saved.to_numpy())
    with pytest.raises(RuntimeError, match=r"of 257 parcels did not reach t_span; the first is parcel \d+"):
        cloudy.solve_tsit5_adaptive_saveat(par, dev(cloudy, u0), H.GOLOVIN_T, ts, max_steps=2, info=True)
