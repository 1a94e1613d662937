"""GPU tests of the per-column adaptive Tsit5 for rainshaft columns (cloudy_rainshaft_tsit5_adaptive, csrc/adaptive_column.hpp).

The reference is the NumPy restatement of tests/test_column_adaptive_host.py (tsit5_restated.adaptive_tsit5 with clamp=True) on the
oracle's column right-hand side, on the batch that module picks: 27 columns of 20 cells -- two workgroups at 512 threads, three at 256 --
amplitudes over a decade, the supersaturation profile of test_gpu_column_sources.  Run with `-m gpu`."""
import ctypes as C

import numpy as np
import pytest

from gpu_support import DZ, NCOL, NZ, VEL, XI, blank, dev, is_blank, moving_column_case
from gpu_support import column_plan as plan_of
from gpu_support import column_run as run
from test_column_adaptive_host import CASES, DT0, FIRST, T_SPAN, column_reference_cached
from tsit5_restated import DONE, DT_MIN, MAX_STEPS, default_opts

pytestmark = pytest.mark.gpu
COAL, COALCOND = 1, 3


# ---- 1. decision parity
@pytest.mark.parametrize("first", sorted(FIRST, reverse=True))
@pytest.mark.parametrize("case", CASES)
def test_decision_parity_with_the_restatement(gpu_cloudy, oracle, case, first):
    """COAL | COND on both plans, from a caller's first step DT0 that the denser columns reject ("dt0": the batch of the issue's
    check): every column ends with status 0 and t == t_span exactly, its accepted and rejected counts are the restatement's, the
    state is within 1e-9 of each plane's maximum (the bound of the column parity test), dt_dev within 1e-6 relative, and the step
    counts differ between columns of one workgroup.  "auto": the same batch from the automatic first step (Hairer's guess from the
    two column means; no rejections) with the same assertions but for dt_dev, which the reference itself resolves to 7e-3 only
    there (test_the_batch_of_the_gpu_tests says why and asserts it): held to 5e-2."""
    u0, s, want = column_reference_cached(case, first)
    _, plan = plan_of(gpu_cloudy, oracle, case)
    got = run(gpu_cloudy, plan, u0, s, T_SPAN[case], dt_init=0.0 if FIRST[first] is None else FIRST[first])
    print(f"{case} {first}: accepted {got['accepted'].tolist()} rejected {got['rejected'].tolist()}")
    assert np.all(got["status"] == DONE) and np.all(got["t"] == T_SPAN[case])
    assert np.array_equal(got["accepted"], want["accepted"]) and np.array_equal(got["rejected"], want["rejected"])
    err = np.abs(got["u"] - want["u"]).max(axis=1) / (np.abs(want["u"]).max(axis=1) + 1e-300)
    dt_err = np.abs(got["dt"] - want["dt"]) / want["dt"]
    print(f"{case} {first}: max |hip - restatement| / max|plane| = {err.max():.2e}, dt_dev relative {dt_err.max():.2e}")
    assert err.max() < 1e-9 and got["u"].min() >= 0.0
    assert dt_err.max() < (1e-6 if first == "dt0" else 5e-2)
    att = got["accepted"] + got["rejected"]
    assert len(set(att[:25].tolist())) > 1 and (first == "auto" or got["rejected"].sum() > 0)


# ---- 2. per-column independence
@pytest.mark.parametrize("case", CASES)
def test_a_column_does_not_depend_on_its_neighbours_or_the_workgroup_size(gpu_cloudy, oracle, case, monkeypatch):
    """fp64 planes, bitwise: a column run alone, run as the last of 27 and run in the whole batch gives the same u, dt, t and
    counts -- at the default pick (512 threads; the column alone: 256), with CLOUDY_HIP_RS_BLOCK=256 (twelve columns per
    workgroup, the last column in a third one) and =512."""
    u0, s, _ = column_reference_cached(case, "dt0")
    _, plan = plan_of(gpu_cloudy, oracle, case)
    k = 19
    sl, end = slice(k * NZ, (k + 1) * NZ), slice((NCOL - 1) * NZ, NCOL * NZ)
    moved, s_moved = u0.copy(), s.copy()
    moved[:, end], s_moved[end] = u0[:, sl], s[sl]
    seen = []
    for block in (None, "256", "512"):
        if block:
            monkeypatch.setenv("CLOUDY_HIP_RS_BLOCK", block)
        whole = run(gpu_cloudy, plan, u0, s, T_SPAN[case], dt_init=DT0)
        last = run(gpu_cloudy, plan, moved, s_moved, T_SPAN[case], dt_init=DT0)
        alone = run(gpu_cloudy, plan, np.ascontiguousarray(u0[:, sl]), s[sl], T_SPAN[case], dt_init=DT0)
        seen += [(whole["u"][:, sl], whole["dt"][k], whole["t"][k], whole["accepted"][k], whole["rejected"][k]),
                 (last["u"][:, end], last["dt"][-1], last["t"][-1], last["accepted"][-1], last["rejected"][-1]),
                 (alone["u"], alone["dt"][0], alone["t"][0], alone["accepted"][0], alone["rejected"][0])]
        if block:   # the other columns of the batch have the bits of the default pick as well
            assert np.array_equal(whole["u"], first_whole["u"]) and np.array_equal(whole["dt"], first_whole["dt"])
        else:
            first_whole = whole
    assert seen[0][4] > 0                                # (a column with a rejected step)
    for other in seen[1:]:
        assert np.array_equal(other[0], seen[0][0]) and other[1:] == seen[0][1:]


# ---- 3. error control
@pytest.mark.parametrize("case", CASES)
def test_error_control(gpu_cloudy, oracle, case):
    """Against the restatement at reltol = 1e-10: the error at reltol = 1e-8 is smaller than at 1e-5 in every plane that carries
    mass.  Attempts and tolerance: the column the controller works hardest on takes strictly more attempts at every tighter
    reltol (1e-5 < 1e-8 < 1e-10: 20 < 30 < 42 and 15 < 18 < 22 in the restatement).  Column by column this does not hold in the
    rules themselves -- the sparsest columns of the batch are governed by the automatic first step, and the restatement gives them
    10, 7 and 6 attempts -- so the maximum over the batch is what is asserted."""
    u0, s, ref = column_reference_cached(case, "auto", 1e-10)
    _, plan = plan_of(gpu_cloudy, oracle, case)
    res = {rt: run(gpu_cloudy, plan, u0, s, T_SPAN[case], reltol=rt) for rt in (1e-5, 1e-8, 1e-10)}
    mass = np.abs(ref["u"]).max(axis=1) > 0.0
    err = {rt: np.abs(res[rt]["u"] - ref["u"]).max(axis=1) / (np.abs(ref["u"]).max(axis=1) + 1e-300) for rt in res}
    att = {rt: int((res[rt]["accepted"] + res[rt]["rejected"]).max()) for rt in res}
    print(f"{case}: error per plane at 1e-5 {err[1e-5]}, at 1e-8 {err[1e-8]}, at 1e-10 {err[1e-10]}; most attempts {att}")
    assert all(np.all(r["status"] == DONE) for r in res.values())
    assert mass.any() and np.all(err[1e-8][mass] < err[1e-5][mass])
    assert att[1e-5] < att[1e-8] < att[1e-10]


# ---- 4. sources
@pytest.mark.parametrize("case", CASES)
def test_sources(gpu_cloudy, oracle, case):
    """COAL | COND with xi = 0 has the bits of COAL; with the profile on every plane that carries mass moves."""
    u0, s, _ = column_reference_cached(case, "auto")
    _, plan = plan_of(gpu_cloudy, oracle, case)
    coal = run(gpu_cloudy, plan, u0, None, T_SPAN[case], sources=COAL)
    zero = run(gpu_cloudy, plan, u0, s, T_SPAN[case], sources=COALCOND, xi=0.0)
    both = run(gpu_cloudy, plan, u0, s, T_SPAN[case], sources=COALCOND)
    for key in ("u", "dt", "t", "accepted", "rejected", "status"):
        assert np.array_equal(coal[key], zero[key]), key
    assert np.all(coal["status"] == DONE)
    moved = np.abs(both["u"] - coal["u"]).max(axis=1) / (np.abs(coal["u"]).max(axis=1) + 1e-300)
    mass = np.abs(coal["u"]).max(axis=1) > 0.0
    print(f"{case}: the condensation source moves the planes by {moved} of their maxima")
    assert mass.any() and np.all(moved[mass] > 1e-4)


# ---- 5. budget and degenerate columns
@pytest.mark.parametrize("case", CASES)
def test_budget_and_degenerate_columns(gpu_cloudy, oracle, case):
    """max_steps = 3: status 1 with t < t_span where the restatement says so (every column), at its t.  An all-zero column in
    the same workgroup takes one accepted step and stays zero.  A column with one NaN moment ends with status 1 or 2 within
    max_steps = 50, and its workgroup neighbours keep the bits they have without it."""
    u0, s, want = column_reference_cached(case, "auto", 1e-6, 3)
    _, plan = plan_of(gpu_cloudy, oracle, case)
    got = run(gpu_cloudy, plan, u0, s, T_SPAN[case], max_steps=3)
    assert np.array_equal(got["status"], want["status"]) and np.all(got["status"] == MAX_STEPS)
    assert np.array_equal(got["accepted"], want["accepted"]) and np.array_equal(got["rejected"], want["rejected"])
    assert np.all(got["t"] < T_SPAN[case]) and np.allclose(got["t"], want["t"], rtol=1e-6, atol=0)
    zero = u0.copy()
    zero[:, 3 * NZ:4 * NZ] = 0.0
    base = run(gpu_cloudy, plan, zero, s, T_SPAN[case], max_steps=50)
    assert (base["accepted"][3], base["rejected"][3], base["status"][3], base["t"][3]) == (1, 0, DONE, T_SPAN[case])
    assert not base["u"][:, 3 * NZ:4 * NZ].any()
    bad = zero.copy()
    bad[1, 5 * NZ + 11] = np.nan
    res = run(gpu_cloudy, plan, bad, s, T_SPAN[case], max_steps=50)
    assert res["status"][5] in (MAX_STEPS, DT_MIN) and res["accepted"][5] + res["rejected"][5] <= 50
    keep = np.ones(u0.shape[1], bool)
    keep[5 * NZ:6 * NZ] = False
    cols = np.arange(NCOL) != 5
    assert np.array_equal(res["u"][:, keep], base["u"][:, keep])
    for key in ("dt", "t", "accepted", "rejected", "status"):
        assert np.array_equal(res[key][cols], base[key][cols]), key


# ---- 6. warm start and edge cases
@pytest.mark.parametrize("case", CASES)
def test_warm_start_and_edge_cases(gpu_cloudy, oracle, case):
    """The second call, with the returned dt_dev, takes no more attempts than the first call took without it; t_span = 0 copies with
    status 0 and zero counts; n_columns = 0 is CLOUDY_OK; u_out == u_in gives the bits of the out-of-place call; with
    ld > nz * n_columns the sentinel columns are untouched."""
    cloudy = gpu_cloudy
    L = cloudy.lib()
    u0, s, _ = column_reference_cached(case, "auto")
    _, plan = plan_of(cloudy, oracle, case)
    n = u0.shape[1]
    cold = run(cloudy, plan, u0, s, T_SPAN[case], ld=n + 37)
    assert cold["pad"].shape[1] == 37 and np.all(is_blank(cold["pad"]))
    assert np.array_equal(cold["u"], run(cloudy, plan, u0, s, T_SPAN[case])["u"])
    warm = run(cloudy, plan, cold["u"], s, T_SPAN[case], dt_in=cold["dt"])
    a_w, a_c = warm["accepted"] + warm["rejected"], cold["accepted"] + cold["rejected"]
    print(f"{case}: attempts of the second call, warm {a_w.tolist()}, of the first, cold {a_c.tolist()}")
    assert np.all(warm["status"] == DONE) and np.all(a_w <= a_c) and a_w.sum() < a_c.sum()
    still = run(cloudy, plan, u0, s, 0.0)
    assert np.array_equal(still["u"].view(np.uint64), u0.view(np.uint64))
    assert not still["accepted"].any() and not still["rejected"].any() and not still["status"].any() and not still["t"].any()
    o = default_opts(cloudy)   # (a direct call: no column, no leading dimension and no buffer is not a batch the driver can build)
    assert L.cloudy_rainshaft_tsit5_adaptive(plan.handle, NZ, 0, 0, None, None, COALCOND, None, 0.0, XI, DZ, 1.0, C.byref(o), None, None,
                                             None, None) == 0
    assert np.array_equal(run(cloudy, plan, u0, s, T_SPAN[case], in_place=True, no_outputs=True)["u"], cold["u"])


# ---- 7. float planes
@pytest.mark.parametrize("case", CASES)
def test_float_planes(gpu_cloudy, oracle, case):
    """CLOUDY_F32 planes: state and control stay in fp64 registers, so the output equals the float rounding of the fp64 run on
    the float-rounded input, and the counts are equal."""
    u0, s, _ = column_reference_cached(case, "dt0")
    u32 = u0.astype(np.float32)
    _, p64 = plan_of(gpu_cloudy, oracle, case)
    _, p32 = plan_of(gpu_cloudy, oracle, case, dtype=1)
    a = run(gpu_cloudy, p64, u32.astype(np.float64), s, T_SPAN[case], dt_init=DT0)
    b = run(gpu_cloudy, p32, u32, s, T_SPAN[case], dt_init=DT0)
    assert np.array_equal(b["u"], a["u"].astype(np.float32))
    for key in ("accepted", "rejected", "status", "t", "dt"):
        assert np.array_equal(a[key], b[key]), key
    assert a["rejected"].sum() > 0


# ---- 8. refusals
def test_refusals(gpu_cloudy, oracle):
    """MovingThreshold, NumericalCoalStyle, CLOUDY_F32_FAST, nz = 1025 and a plan created with specialize = -1: each
    CLOUDY_EUNSUPPORTED with a message that names the fixed-step integrator, and the output sentinels stay intact.  A plan without
    velocity terms: CLOUDY_EINVAL."""
    import bench
    from cloudy_jl_amd.box_model import _numerical_plan_for

    cloudy = gpu_cloudy
    E = cloudy._lib
    par, plan = plan_of(cloudy, oracle, "gamma_mixture")
    mpar, _, mtypes, _ = moving_column_case(cloudy, oracle)
    plans = {"moving": (mpar.coal_data.plan(mtypes, vel=VEL), 6, "MovingThreshold"),
             "numerical": (_numerical_plan_for(bench.cfg4q_par(cloudy), 0), 9, "NumericalCoalStyle"),
             "f32_fast": (par.coal_data.plan([1, 1], vel=VEL, dtype=2), 6, "CLOUDY_F32_FAST"),
             "tall": (plan, 6, "1024"),
             "aot": (par.coal_data.plan([1, 1], vel=VEL, specialize=-1), 6, "compiled for the plan"),
             "no_velocity": (par.coal_data.plan([1, 1]), 6, "n_vel")}
    for name, (p, nm, word) in plans.items():
        nz = 1025 if name == "tall" else 20
        got = run(cloudy, p, blank(nm, 2 * nz, np.float32 if name == "f32_fast" else np.float64), 0.01, 1.0, nz=nz, no_outputs=True,
                  expect=E.EINVAL if name == "no_velocity" else E.EUNSUPPORTED)
        msg = got["message"]
        assert word in msg and (name == "no_velocity" or "cloudy_rainshaft_cond_ssprk33_steps" in msg), (name, msg)
        assert np.all(is_blank(got["u"])), name


# ---- 9. the Python wrapper
def test_python_wrapper(gpu_cloudy, oracle):
    cloudy = gpu_cloudy
    case = "single_gamma"
    u0, s, want = column_reference_cached(case, "auto")
    par, _ = plan_of(cloudy, oracle, case)
    ud, sd = dev(cloudy, u0), dev(cloudy, s[None, :])
    out = cloudy.DeviceArray.zeros(*u0.shape)
    dt_dev = cloudy.DeviceArray.zeros(1, NCOL)
    assert cloudy.solve_rainshaft_tsit5_adaptive(par, ud, T_SPAN[case], XI, sd, out=out, dt_dev=dt_dev) is out
    assert np.array_equal(ud.to_numpy(), u0) and np.all(dt_dev.to_numpy() > 0.0)
    res = cloudy.solve_rainshaft_tsit5_adaptive(par, ud, T_SPAN[case], XI, sd, out=out, info=True)
    assert isinstance(res, tuple) and len(res) == 4 and all(r.shape == (NCOL,) for r in res)
    assert np.array_equal(res[0], want["accepted"]) and np.array_equal(res[1], want["rejected"]) and not res[2].any()
    assert np.all(res[3] == T_SPAN[case])
    assert cloudy.solve_rainshaft_tsit5_adaptive(par, ud, T_SPAN[case]) is ud          # in place, coalescence + sedimentation
    with pytest.raises(RuntimeError, match=r"27 of 27 columns did not reach t_span; the first is column 0 \(status 1"):
        cloudy.solve_rainshaft_tsit5_adaptive(par, dev(cloudy, u0), T_SPAN[case], XI, sd, max_steps=3, info=True)
    with pytest.raises(ValueError):
        cloudy.solve_rainshaft_tsit5_adaptive(par, ud, T_SPAN[case], dt_dev=cloudy.DeviceArray.zeros(1, NCOL + 1))
