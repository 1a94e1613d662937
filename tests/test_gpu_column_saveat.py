"""GPU tests of the dense output of the per-column adaptive Tsit5 (cloudy_rainshaft_tsit5_adaptive_saveat, csrc/adaptive_column.hpp
with SAVE = true).

The reference is the NumPy restatement of tests/test_column_saveat_host.py (tsit5_restated.adaptive_tsit5 with clamp=True and t_save)
on the oracle's column right-hand side, on the batch of tests/test_column_adaptive_host.py -- 27 columns of 20 cells, two workgroups
at 512 threads, COAL | COND with the supersaturation profile on, from the caller's first step DT0 -- at the twelve save times of
tsit5_restated.SAVE_FRACS.  Run with `-m gpu`."""
import numpy as np
import pytest

from gpu_support import NCOL, NZ, VEL, XI, bits_equal, dev, is_blank, moving_column_case
from gpu_support import column_plan as plan_of
from gpu_support import column_run as run
from test_column_adaptive_host import CASES, DT0, T_SPAN
from test_column_saveat_host import SNAPSHOT_BOUND, column_saveat_reference_cached, snapshot_distance, snapshots_reached
from tsit5_restated import DONE, MAX_STEPS

pytestmark = pytest.mark.gpu
KEYS = ("u", "dt", "t", "accepted", "rejected", "status")


def saveat(cloudy, plan, u0, s, t_span, times, **kw):
    return run(cloudy, plan, u0, s, t_span, times=times, **kw)


_RUNS = {}


def device_run(cloudy, oracle, case):
    """cloudy_rainshaft_tsit5_adaptive_saveat on the batch at the twelve save times, ld = n + 7, once per session"""
    if case not in _RUNS:
        u0, s, ts, _ = column_saveat_reference_cached(case, "dt0")
        _, plan = plan_of(cloudy, oracle, case)
        _RUNS[case] = saveat(cloudy, plan, u0, s, T_SPAN[case], ts, ld=u0.shape[1] + 7, dt_init=DT0)
    return _RUNS[case]


# ---- 1. saving does not disturb the integration
@pytest.mark.parametrize("block", [None, "256"])
@pytest.mark.parametrize("case", CASES)
def test_saving_does_not_disturb_the_integration(gpu_cloudy, oracle, case, block, monkeypatch):
    """u_out, dt_dev, t_dev and info_dev of a call with the twelve save times, and of one with n_save = 0, have the bits of
    cloudy_rainshaft_tsit5_adaptive on the same input -- at the default pick of the workgroup size (512 threads) and with
    CLOUDY_HIP_RS_BLOCK=256, which both entry points honour alike."""
    if block:
        monkeypatch.setenv("CLOUDY_HIP_RS_BLOCK", block)
    u0, s, ts, _ = column_saveat_reference_cached(case, "dt0")
    _, plan = plan_of(gpu_cloudy, oracle, case)
    plain = run(gpu_cloudy, plan, u0, s, T_SPAN[case], dt_init=DT0)
    with_times = saveat(gpu_cloudy, plan, u0, s, T_SPAN[case], ts, dt_init=DT0)
    without = saveat(gpu_cloudy, plan, u0, s, T_SPAN[case], (), dt_init=DT0)
    assert plain["rejected"].sum() > 0 and np.all(plain["status"] == DONE)
    for key in KEYS:
        assert bits_equal(with_times[key], plain[key]), key
        assert bits_equal(without[key], plain[key]), key
    assert is_blank(without["guard"]).all()
    if block:   # the snapshots do not depend on the workgroup size either
        assert bits_equal(with_times["saved"], device_run(gpu_cloudy, oracle, case)["saved"])


# ---- 2. snapshot parity with the restatement
@pytest.mark.parametrize("case", CASES)
def test_snapshot_parity_with_the_restatement(gpu_cloudy, oracle, case):
    """The counts are the restatement's column by column and every snapshot is within 1e-9 of its plane's maximum -- the bound of
    the column parity test, which the restatement resolves: its own response to the last bit of its right-hand side is 1.1e-14
    (test_snapshots_are_insensitive_to_the_last_bit_of_the_rhs asserts a tenth of the bound).  No snapshot the integrator forms
    is negative; the one at 0 is the input, its -1e-30 cell included (test 3)."""
    _, _, ts, want = column_saveat_reference_cached(case, "dt0")
    got = device_run(gpu_cloudy, oracle, case)
    assert np.array_equal(got["accepted"], want["accepted"]) and np.array_equal(got["rejected"], want["rejected"])
    assert np.all(got["status"] == DONE) and np.isfinite(got["saved"]).all()
    err = snapshot_distance(got["saved"], want["saved"])
    print(f"{case}: max over the snapshots of |hip - restatement| / max|plane| = {err:.2e}")
    assert err < SNAPSHOT_BOUND
    assert ts[0] == 0.0 and got["saved"][1:].min() >= 0.0


# ---- 3. end points and padding
@pytest.mark.parametrize("case", CASES)
def test_end_points_and_padding(gpu_cloudy, oracle, case):
    """The snapshot at 0 has the bits of u_in and the one at t_span those of u_out; with ld = n + 7 the columns n .. ld of every
    snapshot plane and everything behind the last snapshot keep their sentinel; u_in is unchanged; u_out_dev == u_in_dev gives
    the same snapshots."""
    u0, s, ts, _ = column_saveat_reference_cached(case, "dt0")
    got = device_run(gpu_cloudy, oracle, case)
    n = u0.shape[1]
    assert ts[0] == 0.0 and ts[-1] == T_SPAN[case]
    assert bits_equal(got["saved"][0], u0) and bits_equal(got["saved"][-1], got["u"])
    assert got["saved_pad"].shape[2] == 7 and is_blank(got["saved_pad"]).all() and is_blank(got["guard"]).all()
    assert is_blank(got["pad"]).all()
    assert bits_equal(got["u_in"], got["buf"])
    _, plan = plan_of(gpu_cloudy, oracle, case)
    same = saveat(gpu_cloudy, plan, u0, s, T_SPAN[case], ts, ld=n + 7, dt_init=DT0, in_place=True)
    assert bits_equal(same["saved"], got["saved"]) and bits_equal(same["u"], got["u"])
    assert is_blank(same["saved_pad"]).all() and is_blank(same["guard"]).all()
    still = saveat(gpu_cloudy, plan, u0, s, 0.0, (0.0,), dt_init=DT0)          # t_span = 0: every snapshot is the input
    assert bits_equal(still["saved"][0], u0) and bits_equal(still["u"], u0) and is_blank(still["guard"]).all()


# ---- 4. budget
@pytest.mark.parametrize("case", CASES)
def test_budget(gpu_cloudy, oracle, case):
    """max_steps = 3: every cell of a stopped column has NaN in every plane of each snapshot beyond t_dev[col] and finite values,
    the restatement's, in each snapshot it passed; the columns that reached t_span are complete."""
    u0, s, ts, want = column_saveat_reference_cached(case, "dt0", 1e-6, 3)
    _, plan = plan_of(gpu_cloudy, oracle, case)
    got = saveat(gpu_cloudy, plan, u0, s, T_SPAN[case], ts, dt_init=DT0, max_steps=3)
    assert np.array_equal(got["status"], want["status"]) and np.array_equal(got["accepted"], want["accepted"])
    stopped = got["status"] == MAX_STEPS
    assert stopped.any() and (got["status"] == DONE).any() and np.all(got["t"][stopped] < T_SPAN[case])
    reached, none = snapshots_reached(got["saved"])
    for c in range(NCOL):
        assert np.array_equal(reached[:, c], ts <= got["t"][c]), c
        assert np.array_equal(none[:, c], ts > got["t"][c]), c
    assert reached[:, ~stopped].all() and (reached[:, stopped].sum(axis=0) < len(ts)).all()
    assert np.array_equal(np.isnan(got["saved"]), np.isnan(want["saved"]))
    passed = ~np.isnan(want["saved"])
    err = snapshot_distance(np.where(passed, got["saved"], 0.0), np.where(passed, want["saved"], 0.0))
    print(f"{case}, max_steps = 3: the snapshots the columns passed differ from the restatement's by {err:.2e} of the plane maxima")
    assert err < SNAPSHOT_BOUND
    assert is_blank(got["guard"]).all()


# ---- 5. independence
@pytest.mark.parametrize("case", CASES)
def test_a_columns_snapshots_do_not_depend_on_its_neighbours(gpu_cloudy, oracle, case):
    """fp64 planes, bitwise: column 19 run alone (one 256-thread workgroup), as the last of 27 and in the whole batch."""
    u0, s, ts, _ = column_saveat_reference_cached(case, "dt0")
    _, plan = plan_of(gpu_cloudy, oracle, case)
    k = 19
    sl, end = slice(k * NZ, (k + 1) * NZ), slice((NCOL - 1) * NZ, NCOL * NZ)
    moved, s_moved = u0.copy(), s.copy()
    moved[:, end], s_moved[end] = u0[:, sl], s[sl]
    whole = device_run(gpu_cloudy, oracle, case)
    last = saveat(gpu_cloudy, plan, moved, s_moved, T_SPAN[case], ts, dt_init=DT0)
    alone = saveat(gpu_cloudy, plan, np.ascontiguousarray(u0[:, sl]), s[sl], T_SPAN[case], ts, dt_init=DT0)
    assert whole["rejected"][k] > 0
    assert bits_equal(last["saved"][:, :, end], whole["saved"][:, :, sl]) and bits_equal(alone["saved"], whole["saved"][:, :, sl])


# ---- 6. float planes
@pytest.mark.parametrize("case", CASES)
def test_float_planes(gpu_cloudy, oracle, case):
    """CLOUDY_F32 planes: the snapshots are float, and -- state, control and interpolant in fp64 registers -- each is the float
    rounding of the fp64 run's on the float-rounded input: the bound of test_float_planes of test_gpu_column_adaptive.py, equality;
    the snapshot at t_span has the bits of u_out."""
    u0, s, ts, _ = column_saveat_reference_cached(case, "dt0")
    u32 = u0.astype(np.float32)
    _, p64 = plan_of(gpu_cloudy, oracle, case)
    _, p32 = plan_of(gpu_cloudy, oracle, case, dtype=1)
    a = saveat(gpu_cloudy, p64, u32.astype(np.float64), s, T_SPAN[case], ts, dt_init=DT0)
    b = saveat(gpu_cloudy, p32, u32, s, T_SPAN[case], ts, dt_init=DT0, ld=u0.shape[1] + 7)
    assert b["saved"].dtype == np.float32 and a["rejected"].sum() > 0
    assert np.array_equal(b["saved"], a["saved"].astype(np.float32))
    assert bits_equal(b["saved"][-1], b["u"]) and bits_equal(b["saved"][0], u32)
    assert is_blank(b["saved_pad"]).all() and is_blank(b["guard"]).all()
    for key in ("accepted", "rejected", "status", "t", "dt"):
        assert np.array_equal(a[key], b[key]), key


# ---- 7. refusals
def test_refusals(gpu_cloudy, oracle):
    """MovingThreshold, NumericalCoalStyle, CLOUDY_F32_FAST and nz = 1025: each CLOUDY_EUNSUPPORTED with a message that names the
    fixed-step integrator; u_out and u_save keep their sentinel."""
    import bench
    from cloudy_jl_amd.box_model import _numerical_plan_for

    cloudy = gpu_cloudy
    E = cloudy._lib
    par, plan = plan_of(cloudy, oracle, "gamma_mixture")
    mpar, _, mtypes, _ = moving_column_case(cloudy, oracle)
    plans = {"moving": (mpar.coal_data.plan(mtypes, vel=VEL), 6, "MovingThreshold"),
             "numerical": (_numerical_plan_for(bench.cfg4q_par(cloudy), 0), 9, "NumericalCoalStyle"),
             "f32_fast": (par.coal_data.plan([1, 1], vel=VEL, dtype=2), 6, "CLOUDY_F32_FAST"),
             "tall": (plan, 6, "1024")}
    for name, (p, nm, word) in plans.items():
        nz = 1025 if name == "tall" else 20
        dtype = np.float32 if name == "f32_fast" else np.float64
        got = saveat(cloudy, p, np.ones((nm, 2 * nz), dtype), None, 1.0, (0.0, 0.5, 1.0), nz=nz, expect=E.EUNSUPPORTED)
        assert word in got["message"] and "cloudy_rainshaft_cond_ssprk33_steps" in got["message"], (name, got["message"])
        assert is_blank(got["u"]).all() and is_blank(got["saved"]).all() and is_blank(got["guard"]).all(), name


# ---- 8. the Python wrapper
def test_python_wrapper(gpu_cloudy, oracle):
    """solve_rainshaft_tsit5_adaptive_saveat returns the bits of the C call."""
    cloudy = gpu_cloudy
    case = "single_gamma"
    u0, s, ts, want = column_saveat_reference_cached(case, "dt0")
    par, plan = plan_of(cloudy, oracle, case)
    ref = saveat(cloudy, plan, u0, s, T_SPAN[case], ts, dt_init=DT0)
    ud, sd = dev(cloudy, u0), dev(cloudy, s[None, :])
    out = cloudy.DeviceArray.zeros(*u0.shape)
    res = cloudy.solve_rainshaft_tsit5_adaptive_saveat(par, ud, T_SPAN[case], ts, XI, sd, dt=DT0, out=out)
    assert isinstance(res, tuple) and len(res) == 2 and res[0] is out
    planes, n = u0.shape
    assert res[1].to_numpy().shape == (len(ts) * planes, n)
    assert bits_equal(res[1].to_numpy().reshape(len(ts), planes, n), ref["saved"]) and bits_equal(out.to_numpy(), ref["u"])
    assert np.array_equal(ud.to_numpy(), u0)
    mine = cloudy.DeviceArray.zeros(len(ts) * planes, n)
    full = cloudy.solve_rainshaft_tsit5_adaptive_saveat(par, ud, T_SPAN[case], ts, XI, sd, dt=DT0, out=out, save_out=mine, info=True)
    assert len(full) == 6 and full[1] is mine and bits_equal(mine.to_numpy().reshape(len(ts), planes, n), ref["saved"])
    assert np.array_equal(full[2], want["accepted"]) and np.array_equal(full[3], want["rejected"]) and not full[4].any()
    assert np.all(full[5] == T_SPAN[case])
    with pytest.raises(RuntimeError, match=r"columns did not reach t_span; the first is column \d+ \(status 1"):
        cloudy.solve_rainshaft_tsit5_adaptive_saveat(par, dev(cloudy, u0), T_SPAN[case], ts, XI, sd, dt=DT0, max_steps=3, info=True)
    with pytest.raises(ValueError):
        cloudy.solve_rainshaft_tsit5_adaptive_saveat(par, ud, T_SPAN[case], ts, save_out=cloudy.DeviceArray.zeros(planes, n))
