#!/usr/bin/env python3
"""ONE timing driver for the GPU box (round 6: replaces fourteen one-off tools/time_*.py; what they measured is recorded in
profiles/ and in the commit log).  HIP events on the launch stream after >= 150 ms of back-to-back launches (bench._sustained_ms);
every experiment switch of the library is an environment variable, so an A/B run is two calls of the same line:

  python tools/timeit.py kernels cfg3b cfg4 moving4 [--reps R] [--parcels P] [--error] [--dtype 0|1|2|3]
        cloudy_coal_rhs of named bench workloads (tensor plans); --error: max |hip - oracle| / scale on 20000 parcels
  python tools/timeit.py conv <constant|linear|hydrodynamic|long> <dist,dist,...> [n] [--fused] [--fixed NQ] [--lognorm-example]
        a NumericalCoalStyle plan on the synthetic batch (1 Gamma, 0 Exponential, 3 Lognormal); --fused: cloudy_ssprk33_steps beside
        three launches; --fixed NQ: the fixed Gauss rule instead of converged mode
  python tools/timeit.py columns [--nz NZ] [--cells N] [--workload cfg3b] [--steps S]
        cloudy_rainshaft_ssprk33_steps and cloudy_rainshaft_rhs (ms per 1e7 cells)
  python tools/timeit.py colcond [--nz NZ] [--cells N] [--workload cfg3b] [--steps S]
        cloudy_rainshaft_cond_ssprk33_steps on the bench's column batch: (a) cloudy_rainshaft_ssprk33_steps, (b) the three sources
        fused, (c) the sequence (b) replaces -- cloudy_rainshaft_rhs + cloudy_cond_evap + torch updates per stage
  python tools/timeit.py coladaptive [--nz NZ] [--cells N] [--workload cfg3b] [--t-span T] [--reltol R] [--max-steps M] [--n-save K]
        cloudy_rainshaft_tsit5_adaptive (COAL | COND) on the batch of `colcond` to t = T (2 s), against
        cloudy_rainshaft_cond_ssprk33_steps with the driver's 2 steps of T / 2 in the same run; statuses, attempts and the
        active-lane fraction from the info planes, sum(attempts) / sum over workgroups of (columns x max(attempts)); --n-save K:
        cloudy_rainshaft_tsit5_adaptive_saveat with 0, 1 and K equidistant save times in the same run, ms per call beside the
        algorithmic snapshot traffic per cell
  python tools/timeit.py integrators [--parcels P]
        cloudy_ssprk33_steps / cloudy_tsit5_steps of the tensor plans cfg3a, cfg3b, cfg2
  python tools/timeit.py box [--parcels P] [--steps S]
        cloudy_box_ssprk33_steps on cfg3a and cfg3b: (a) cloudy_ssprk33_steps, (b) coalescence + condensation fused, (c) condensation
        alone, (d) the unfused sequence (b) replaces -- cloudy_coal_rhs + cloudy_cond_evap + torch updates per stage
  python tools/timeit.py parcel [--parcels P] [--steps S]
        cloudy_parcel_ssprk33_steps on a batch of the driver's mixture case (Exponential + Gamma): (a) the fused call, (b) the
        sequence it replaces -- cloudy_cond_evap per stage plus torch thermodynamics and updates, (c) cloudy_box_ssprk33_steps with
        CLOUDY_SRC_COND on the same moments (constant supersaturation: the floor)
  python tools/timeit.py adaptive [--parcels P] [--t-span T] [--reltol R]
        cloudy_tsit5_adaptive on the cfg3a plan, n log-uniform over three decades: (a) the adaptive call, (b) cloudy_tsit5_steps at
        the fixed dt the densest parcels need for the same measured end-state error -- the caller's only alternative without (a);
        and the active-lane fraction of (a) from the info planes, sum(attempts) / sum over waves of 64 max(attempts)
  python tools/timeit.py boxadaptive [--parcels P] [--t-span T] [--reltol R] [--xi X]
        cloudy_box_tsit5_adaptive on the batch of `adaptive` against cloudy_tsit5_adaptive in the same run: COAL | COND, COND alone,
        COAL | COND with 16 save times; ms per call, ratios and active-lane fractions
  python tools/timeit.py parceladaptive [--parcels P] [--t-span T] [--reltol R]
        cloudy_parcel_tsit5_adaptive on one Monodisperse mode: the decade batch (N = 2e8 10^U(-1, 1), w = U(0.5, 10), default_rng(5))
        and the driver's uniform batch (N = 2e8, w = 10); for each the new entry point with 0 and 41 save times and
        cloudy_parcel_ssprk33_steps with the driver's 40 steps of t_span / 40; ms per call and active-lane fractions.  The two
        integrators do different amounts of work for different accuracy
  python tools/timeit.py saveat [--parcels P] [--t-span T] [--reltol R]
        cloudy_tsit5_adaptive_saveat on the batch of `adaptive`: cloudy_tsit5_adaptive itself, then the new entry point with n_save =
        0, 1 and 16 equidistant save times (the last at t_span), and the algorithmic snapshot traffic per parcel
  python tools/timeit.py spectra [--parcels P]
        cloudy_moments on the cfg3a batch with 1 and 8 orders, full and up to a cutoff of 1e-9 kg, and cloudy_density at 16 and 100
        grid points (on as many parcels as keep its output within the bytes of the 8-order call), each beside a fill
        (cloudy_memset) of as many output planes in the same run: the store floor of the call (the library exports no
        device-to-device copy; the reads of a call are the plan's 6 moment planes)
  python tools/timeit.py host [--parcels P]
        cloudy_coal_rhs_host on cfg3a: the PCIe-inclusive rate (host arrays staged through the device)

switches read by the library: CLOUDY_HIP_LIB, CLOUDY_HIP_JIT, CLOUDY_HIP_JIT_DEFS, CLOUDY_HIP_CONV_HINTS, CLOUDY_HIP_CONV_BLOCK,
CLOUDY_HIP_CONV_ROUNDS, CLOUDY_HIP_LONG_SPLIT, CLOUDY_HIP_JIT_QUAD_WAVES, CLOUDY_HIP_RS_BLOCK, CLOUDY_HIP_RS_FUSED_RHS, ..."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bench  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402


def kernel_functions(pkg):
    return {"constant": pkg.ConstantKernelFunction(1e-4), "linear": pkg.LinearKernelFunction(5.0),
            "hydrodynamic": pkg.HydrodynamicKernelFunction(1e2 * np.pi), "long": pkg.LongKernelFunction(5.236e-10, 9.44e9, 5.78)}


def cmd_kernels(a, pkg, L):
    out = []
    for name in a.names:
        n = a.parcels or bench.workload_spec(name)["default_parcels"]
        wl = bench.make_workload(name, n)
        plan = wl["coal_data"].plan(wl["dist_types"], dtype=a.dtype)
        dt = pkg.plane_dtype(plan) if hasattr(pkg, "plane_dtype") else np.float64
        m, dm = pkg.DeviceArray.from_numpy(wl["mom"].astype(dt)), pkg.DeviceArray.zeros(plan.nmom, n, dt)
        ms = bench._event_ms(pkg, plan, m, dm, a.reps)
        err = ""
        if a.error:
            from oracle import cloudy_oracle as O

            ns = min(n, 20000)
            want, scale = O.rhs_coal_batch(bench.oracle_params(name), np.ascontiguousarray(wl["mom"][:, :ns]), with_scale=True)
            got = dm.columns_to_numpy(ns)
            ok = np.isfinite(want) & (scale > 0)
            err = f", err {float((np.abs(got - want)[ok] / scale[ok]).max()):.1e}, nan {int(np.isnan(got[ok]).sum())}"
        out.append(f"{name} {ms:.3f} ms ({n / ms * 1e3:.3e}/s, jit={int(plan.specialized)}{err})")
        del m, dm
    print(os.environ.get("CLOUDY_HIP_JIT_DEFS", "") or "default", "|", " | ".join(out), flush=True)


def cmd_conv(a, pkg, L):
    dists = [int(x) for x in a.dists.split(",")]
    N = len(dists)
    n = a.n
    if a.lognorm_example:
        mom = bench.lognorm_example_moments(n)
    elif N <= 4:
        mom = bench.synth_moments(N, n, bench.SEED)
    else:   # N size classes between 1e-12 and 1e-4 kg, number densities falling with size (as tests/test_gpu_parity.py::many_mode_moments)
        rng = np.random.Generator(np.random.Philox(key=bench.SEED))
        edges = np.logspace(-12, -4, N + 1)
        mom = np.ascontiguousarray(np.concatenate([bench._gamma_mode(rng, n, 1e6 * 10.0 ** (-1.5 * i * 8 / N), 1e9 * 10.0 ** (-1.5 * i * 8 / N),
                                                                      0.5 if i == 0 else 1.0, 7.0, edges[i], edges[i + 1]) for i in range(N)]))
    m, dm = pkg.DeviceArray.from_numpy(mom), pkg.DeviceArray.zeros(3 * N, n)
    kfn = pkg.get_normalized_kernel_func(kernel_functions(pkg)[a.kernel], bench.NORMS)
    plan = pkg.NumericalPlan(dists, kfn, bench.NORMS, a.fixed or 8, specialize=1,
                             quad_mode=pkg.QUAD_FIXED if a.fixed else pkg.QUAD_CONVERGED)
    ms = bench._sustained_ms(pkg, lambda: pkg._lib.check(L.cloudy_coal_rhs(plan.handle, n, n, m.ptr, dm.ptr, None)), min_reps=a.reps,
                             max_reps=max(a.reps, 20))
    line = f"{'fixed ' + str(a.fixed) if a.fixed else 'converged'} {a.kernel} {dists}: {ms:.3f} ms per {n} parcels = {n / ms * 1e3:.3e} parcel-RHS/s"
    if a.fused:
        mi = bench._sustained_ms(pkg, lambda: pkg._lib.check(
            L.cloudy_ssprk33_steps(plan.handle, n, n, m.ptr, dm.ptr, C.c_double(1e-3), 1, None)), min_reps=3, max_reps=10)
        line += f"; cloudy_ssprk33_steps (3 evaluations) {mi:.3f} ms = {mi / (3 * ms):.2f} x three launches"
    print(line, flush=True)


def cmd_columns(a, pkg, L):
    nz, ncol = a.nz, max(a.cells // a.nz, 1)
    n = nz * ncol
    wl = bench.make_workload(a.workload, n, seed=7)
    plan = wl["coal_data"].plan(wl["dist_types"], vel=((50.0, 1.0 / 6),))
    u, out = pkg.DeviceArray.from_numpy(wl["mom"]), pkg.DeviceArray.zeros(*wl["mom"].shape)
    flux = pkg.DeviceArray.zeros(*wl["mom"].shape)
    ms_i = bench._sustained_ms(pkg, lambda: pkg._lib.check(
        L.cloudy_rainshaft_ssprk33_steps(plan.handle, nz, ncol, n, u.ptr, out.ptr, 150.0, 1e-3, a.steps, None)), min_reps=3)
    ms_r = bench._sustained_ms(pkg, lambda: pkg._lib.check(
        L.cloudy_rainshaft_rhs(plan.handle, nz, ncol, n, u.ptr, 150.0, flux.ptr, out.ptr, None)), min_reps=3)
    print(f"{a.workload} columns nz={nz} x {ncol}: integrator {ms_i:.3f} ms per call of {a.steps} step(s) = {ms_i / (3 * a.steps) * 1e7 / n:.3f} ms "
          f"per evaluation of 1e7 cells; cloudy_rainshaft_rhs {ms_r * 1e7 / n:.3f} ms per 1e7 cells  (CLOUDY_HIP_RS_BLOCK="
          f"{os.environ.get('CLOUDY_HIP_RS_BLOCK', 'auto')})", flush=True)


def cmd_colcond(a, pkg, L):
    """ms per call of S steps on nz-cell columns with a supersaturation per cell: (a) the existing column integrator (no third
    source), (b) cloudy_rainshaft_cond_ssprk33_steps, (c) the same steps stage by stage: the clamp, two right-hand-side launches and
    the update on the planes (torch, on the same stream) per stage"""
    here = os.path.dirname(os.path.abspath(__file__))   # torch imports the standard library's timeit: this file must not shadow it
    sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") != here]
    import torch

    nz, ncol = a.nz, max(a.cells // a.nz, 1)
    n, steps, xi, dz, h = nz * ncol, a.steps, 1e-8, 150.0, 1e-3
    wl = bench.make_workload(a.workload, n, seed=7)
    plan = wl["coal_data"].plan(wl["dist_types"], vel=((50.0, 1.0 / 6),))
    u0, out = pkg.DeviceArray.from_numpy(wl["mom"]), pkg.DeviceArray.zeros(*wl["mom"].shape)
    z = (np.arange(nz) + 0.5) * dz
    s = pkg.DeviceArray.from_numpy(np.tile(np.where(z >= 0.45 * z.max(), 0.03, -0.2), ncol)[None, :])
    ms_a = bench._sustained_ms(pkg, lambda: pkg._lib.check(
        L.cloudy_rainshaft_ssprk33_steps(plan.handle, nz, ncol, n, u0.ptr, out.ptr, dz, h, steps, None)), min_reps=3)
    ms_b = bench._sustained_ms(pkg, lambda: pkg._lib.check(
        L.cloudy_rainshaft_cond_ssprk33_steps(plan.handle, nz, ncol, n, u0.ptr, out.ptr, s.ptr, 0.0, xi, dz, h, steps, None)), min_reps=3)
    t0 = torch.from_numpy(wl["mom"]).cuda()
    u, up, f, g, w = (torch.empty_like(t0) for _ in range(5))

    def staged():
        u.copy_(t0)
        for _ in range(steps):
            for stage in range(3):
                u.clamp_(min=0.0)
                if stage == 0:
                    up.copy_(u)
                pkg._lib.check(L.cloudy_rainshaft_rhs(plan.handle, nz, ncol, n, u.data_ptr(), dz, w.data_ptr(), f.data_ptr(), None))
                pkg._lib.check(L.cloudy_cond_evap(plan.handle, n, n, u.data_ptr(), s.ptr, 0.0, xi, g.data_ptr(), None))
                f.add_(g)
                if stage == 0:
                    torch.add(up, f, alpha=h, out=u)
                elif stage == 1:
                    u.add_(f, alpha=h).add_(up, alpha=3.0).mul_(0.25)
                else:
                    u.mul_(2.0).add_(f, alpha=2.0 * h).add_(up).div_(3.0)
        u.clamp_(min=0.0)

    ms_c = bench._sustained_ms(pkg, staged, min_reps=3)
    # What the timed calls computed.  The stepped states of this synthetic batch are not compared: random parcels stacked as
    # columns hold zero-variance cells whose closure flips under one ulp, and the existing integrator and the oracle themselves
    # move by many orders of magnitude there under a 1e-15 perturbation.  One evaluation is well conditioned: the
    # fused right-hand side with the source against cloudy_rainshaft_rhs + cloudy_cond_evap, entry by entry, and with s = 0
    # the new integrator against the existing one, bit for bit.
    x = pkg.DeviceArray.from_numpy(np.maximum(wl["mom"], 0.0))
    fr, base, cond = (pkg.DeviceArray.zeros(*wl["mom"].shape) for _ in range(3))
    pkg._lib.check(L.cloudy_rainshaft_cond_rhs(plan.handle, nz, ncol, n, x.ptr, s.ptr, 0.0, xi, dz, w.data_ptr(), fr.ptr, None))
    pkg._lib.check(L.cloudy_rainshaft_rhs(plan.handle, nz, ncol, n, x.ptr, dz, w.data_ptr(), base.ptr, None))
    pkg._lib.check(L.cloudy_cond_evap(plan.handle, n, n, x.ptr, s.ptr, 0.0, xi, cond.ptr, None))
    fr, base, cond = fr.to_numpy(), base.to_numpy(), cond.to_numpy()
    same_nan = bool(np.array_equal(np.isfinite(fr), np.isfinite(base + cond)))
    fin = np.isfinite(fr) & np.isfinite(base + cond)
    dev = float((np.abs(fr - (base + cond))[fin] / np.maximum((np.abs(base) + np.abs(cond))[fin], 1e-300)).max())
    o0 = pkg.DeviceArray.zeros(*wl["mom"].shape)
    pkg._lib.check(L.cloudy_rainshaft_ssprk33_steps(plan.handle, nz, ncol, n, u0.ptr, out.ptr, dz, h, steps, None))
    pkg._lib.check(L.cloudy_rainshaft_cond_ssprk33_steps(plan.handle, nz, ncol, n, u0.ptr, o0.ptr, None, 0.0, xi, dz, h, steps, None))
    bits = bool(np.array_equal(out.to_numpy(), o0.to_numpy(), equal_nan=True))
    print(f"{a.workload} columns nz={nz} x {ncol}, {steps} steps per call: (a) cloudy_rainshaft_ssprk33_steps {ms_a:.3f} ms | (b) with "
          f"condensation, fused {ms_b:.3f} ms | (c) rainshaft_rhs + cond_evap + torch updates per stage {ms_c:.3f} ms | b/a "
          f"{ms_b / ms_a:.3f} | c/b {ms_c / ms_b:.2f} | one evaluation, fused vs rhs + cond_evap: same finite pattern {same_nan}, max "
          f"{dev:.1e} of |rhs| + |cond| per entry | s = 0 steps equal the existing integrator's: {bits}", flush=True)


def cmd_host(a, pkg, L):
    """the PCIe-inclusive rate: cloudy_coal_rhs_host stages host arrays through the device (never the bench's `value`)"""
    import time

    n = a.parcels or 10_000_000
    wl = bench.make_workload("cfg3a", n)
    plan = wl["coal_data"].plan(wl["dist_types"])
    mom, out = np.ascontiguousarray(wl["mom"]), np.zeros_like(wl["mom"])
    pin, pout = mom.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    best = 1e9
    for _ in range(4):
        t0 = time.perf_counter()
        pkg._lib.check(L.cloudy_coal_rhs_host(plan.handle, n, n, pin, pout))
        best = min(best, time.perf_counter() - t0)
    gb = 2 * plan.nmom * 8 * n / 1e9
    print(f"cloudy_coal_rhs_host, cfg3a, {n} parcels (pageable host arrays, {gb:.2f} GB over PCIe): {best * 1e3:.1f} ms = {n / best:.3e} parcel-RHS/s "
          f"= {gb / best:.1f} GB/s of host traffic", flush=True)


def cmd_coladaptive(a, pkg, L):
    """ms per call on the batch of colcond: the per-column adaptive integrator to t_span, and the fixed-step integrator with the
    driver's two steps over the same span (different amounts of work for different accuracy: the second has no error control)"""
    nz, ncol = a.nz, max(a.cells // a.nz, 1)
    n, xi, dz = nz * ncol, 1e-8, 150.0
    wl = bench.make_workload(a.workload, n, seed=7)
    plan = wl["coal_data"].plan(wl["dist_types"], vel=((50.0, 1.0 / 6),))
    u0, out = pkg.DeviceArray.from_numpy(wl["mom"]), pkg.DeviceArray.zeros(*wl["mom"].shape)
    z = (np.arange(nz) + 0.5) * dz
    s = pkg.DeviceArray.from_numpy(np.tile(np.where(z >= 0.45 * z.max(), 0.03, -0.2), ncol)[None, :])
    o = pkg._lib.AdaptiveOptsC()
    L.cloudy_adaptive_opts_init(C.byref(o))
    o.reltol, o.max_steps = a.reltol, a.max_steps
    info, t_dev = pkg.DeviceArray.zeros(3, ncol, dtype=np.int32), pkg.DeviceArray.zeros(1, ncol)
    ms_a = bench._sustained_ms(pkg, lambda: pkg._lib.check(L.cloudy_rainshaft_tsit5_adaptive(
        plan.handle, nz, ncol, n, u0.ptr, out.ptr, 3, s.ptr, 0.0, xi, dz, a.t_span, C.byref(o), None, t_dev.ptr, info.ptr, None)), min_reps=3)
    ms_f = bench._sustained_ms(pkg, lambda: pkg._lib.check(L.cloudy_rainshaft_cond_ssprk33_steps(
        plan.handle, nz, ncol, n, u0.ptr, out.ptr, s.ptr, 0.0, xi, dz, a.t_span / 2, 2, None)), min_reps=3)
    acc, rej, status = info.to_numpy()
    att = (acc + rej).astype(np.int64)
    # the workgroup size jit_column_adaptive_part gives this batch: 256 for a batch that fits one workgroup, else the size with the
    # fewest idle lanes among 256 / 512 / 1024 (CLOUDY_HIP_RS_BLOCK: that size)
    env = os.environ.get("CLOUDY_HIP_RS_BLOCK")
    bs = int(env) if env in ("256", "512", "1024") else 256 if ncol <= 256 // nz else min(
        (256, 512, 1024), key=lambda b: (13.7, 13.25, 14.6)[(256, 512, 1024).index(b)] * b / ((b // nz) * nz) if b >= nz else 1e300)
    cpb = bs // nz
    pad = (-ncol) % cpb
    per_wg = np.concatenate([att, np.zeros(pad, np.int64)]).reshape(-1, cpb)
    frac = float(att.sum() * nz) / float(per_wg.max(axis=1).sum() * bs)
    print(f"{a.workload} columns nz={nz} x {ncol}, t_span {a.t_span:g}, reltol {a.reltol:g}, max_steps {a.max_steps}: "
          f"cloudy_rainshaft_tsit5_adaptive {ms_a:.3f} ms per call | cloudy_rainshaft_cond_ssprk33_steps, 2 steps {ms_f:.3f} ms | ratio "
          f"{ms_a / ms_f:.2f} | status 0 / 1 / 2: {int((status == 0).sum())} / {int((status == 1).sum())} / {int((status == 2).sum())} | "
          f"attempts mean {att.mean():.1f}, max {int(att.max())}, rejected {int(rej.sum())} | active-lane fraction {frac:.3f} at {bs} "
          f"threads  (CLOUDY_HIP_RS_BLOCK={env or 'auto'})", flush=True)
    if a.n_save < 1:
        return
    # --n-save K: the same batch through cloudy_rainshaft_tsit5_adaptive_saveat with 0 (the kernel above), 1 and K equidistant save
    # times, the last at t_span, in the same run; beside each the algorithmic snapshot traffic, n_save x planes x sizeof(plane type)
    # per cell
    planes, esz = wl["mom"].shape[0], wl["mom"].dtype.itemsize
    snap = pkg.DeviceArray.zeros(a.n_save * planes, n)
    line = [f"cloudy_rainshaft_tsit5_adaptive {ms_a:.3f} ms"]
    for k in sorted({0, 1, a.n_save}):
        ts = (C.c_double * max(k, 1))(*[a.t_span * (j + 1) / k for j in range(k)])
        ms = bench._sustained_ms(pkg, lambda: pkg._lib.check(L.cloudy_rainshaft_tsit5_adaptive_saveat(
            plan.handle, nz, ncol, n, u0.ptr, out.ptr, 3, s.ptr, 0.0, xi, dz, a.t_span, C.byref(o), None, t_dev.ptr, info.ptr, None, k,
            ts if k else None, snap.ptr if k else None)), min_reps=3)
        line.append(f"n_save = {k}: {ms:.3f} ms ({ms / ms_a:.3f} x, {k * planes * esz} B per cell of snapshots)")
    print(f"{a.workload} columns nz={nz} x {ncol}, cloudy_rainshaft_tsit5_adaptive_saveat in the same run: " + " | ".join(line), flush=True)


def cmd_integrators(a, pkg, L):
    for name in ("cfg3a", "cfg3b", "cfg2"):
        n = a.parcels or 4_000_000
        wl = bench.make_workload(name, n, seed=7)
        plan = wl["coal_data"].plan(wl["dist_types"])
        u, out = pkg.DeviceArray.from_numpy(wl["mom"]), pkg.DeviceArray.zeros(*wl["mom"].shape)
        ms_s = bench._sustained_ms(pkg, lambda: pkg._lib.check(L.cloudy_ssprk33_steps(plan.handle, n, n, u.ptr, out.ptr, C.c_double(1e-3), 4, None)))
        ms_t = bench._sustained_ms(pkg, lambda: pkg._lib.check(L.cloudy_tsit5_steps(plan.handle, n, n, u.ptr, out.ptr, C.c_double(1e-3), 4, None)))
        print(f"{name}, {n} parcels: SSPRK33 {ms_s / 12:.4f} ms per evaluation, Tsit5 {ms_t / 25:.4f} ms per evaluation", flush=True)


def cmd_adaptive(a, pkg, L):
    """ms per call: (a) cloudy_tsit5_adaptive to t_span at reltol, (b) cloudy_tsit5_steps with the number of equal steps at which
    its worst end-state error over a sample of parcels (against 400 fixed steps) is no larger than (a)'s"""
    n, t_span, sample = a.parcels or 10_000_000, a.t_span, 20000
    wl = bench.make_workload("cfg3a", 1)
    plan = wl["coal_data"].plan(wl["dist_types"])
    mom = bench.synth_moments(2, n, 7, degenerate_frac=0.0)   # the cloud mode's n: 1e6 .. 1e9, log-uniform
    u0, out = pkg.DeviceArray.from_numpy(mom), pkg.DeviceArray.zeros(*mom.shape)
    info, t_dev = pkg.DeviceArray.zeros(3, n, np.int32), pkg.DeviceArray.zeros(1, n)
    opts = pkg._lib.AdaptiveOptsC()
    L.cloudy_adaptive_opts_init(C.byref(opts))
    opts.reltol = a.reltol
    call = lambda: pkg._lib.check(L.cloudy_tsit5_adaptive(plan.handle, n, n, u0.ptr, out.ptr, t_span, C.byref(opts), None, t_dev.ptr,   # noqa: E731
                                                          info.ptr, None))
    ms_a = bench._sustained_ms(pkg, call, min_reps=3)
    counts = info.to_numpy()
    attempts = (counts[0] + counts[1]).astype(np.int64)
    waves = np.pad(attempts, (0, -n % 64)).reshape(-1, 64)
    lane_fraction = attempts.sum() / (64 * waves.max(axis=1)).sum()
    got = out.columns_to_numpy(sample)
    us, truth = pkg.DeviceArray.from_numpy(np.ascontiguousarray(mom[:, :sample])), pkg.DeviceArray.zeros(6, sample)
    pkg._lib.check(L.cloudy_tsit5_steps(plan.handle, sample, sample, us.ptr, truth.ptr, t_span / 400, 400, None))
    want = truth.to_numpy()
    # the error is measured on the regular parcels of the sample (as the stepping tests: finite and within a factor 10 of their
    # initial state after 400 steps) that the adaptive call brought to t_span: the order-2 kernel blows up in finite time on the
    # densest tail of 1e7 parcels, where no step size has an error to compare
    with np.errstate(all="ignore"):
        ok = np.isfinite(want).all(axis=0) & (np.abs(want) <= 10 * np.abs(mom[:, :sample]) + 1e-300).all(axis=0) & (counts[2, :sample] == 0)
    err = lambda x: float(np.max((np.abs(x - want) / np.maximum(np.abs(mom[:, :sample]) + np.abs(want), 1e-300))[:, ok]))   # noqa: E731
    e_a = err(got)
    steps, fs = 1, pkg.DeviceArray.zeros(6, sample)
    while steps < 400:
        pkg._lib.check(L.cloudy_tsit5_steps(plan.handle, sample, sample, us.ptr, fs.ptr, t_span / steps, steps, None))
        e_b = err(fs.to_numpy())
        if e_b <= e_a:   # (NaN: not yet)
            break
        steps += max(1, steps // 4)
    ms_b = bench._sustained_ms(pkg, lambda: pkg._lib.check(L.cloudy_tsit5_steps(plan.handle, n, n, u0.ptr, out.ptr, t_span / steps, steps, None)),
                               min_reps=3)
    print(f"cfg3a, {n} parcels to t = {t_span:g}, reltol {a.reltol:g}: (a) cloudy_tsit5_adaptive {ms_a:.3f} ms, attempts 1 .. {attempts.max()} "
          f"(mean {attempts.mean():.2f}, rejected {int(counts[1].sum())}, status != 0: {int((counts[2] != 0).sum())}), end-state error "
          f"{e_a:.1e} on {int(ok.sum())} regular parcels of {sample} | (b) cloudy_tsit5_steps, {steps} steps of {t_span / steps:.3g} for error {e_b:.1e}: {ms_b:.3f} ms | "
          f"b/a {ms_b / ms_a:.2f} | active-lane fraction of (a) {lane_fraction:.3f}", flush=True)


def cmd_saveat(a, pkg, L):
    """ms per call on the batch of cmd_adaptive: cloudy_tsit5_adaptive, and cloudy_tsit5_adaptive_saveat with 0, 1 and 16 save times"""
    n, t_span = a.parcels or 10_000_000, a.t_span
    wl = bench.make_workload("cfg3a", 1)
    plan = wl["coal_data"].plan(wl["dist_types"])
    mom = bench.synth_moments(2, n, 7, degenerate_frac=0.0)
    u0, out = pkg.DeviceArray.from_numpy(mom), pkg.DeviceArray.zeros(*mom.shape)
    info, t_dev = pkg.DeviceArray.zeros(3, n, np.int32), pkg.DeviceArray.zeros(1, n)
    opts = pkg._lib.AdaptiveOptsC()
    L.cloudy_adaptive_opts_init(C.byref(opts))
    opts.reltol = a.reltol
    plain = lambda: pkg._lib.check(L.cloudy_tsit5_adaptive(plan.handle, n, n, u0.ptr, out.ptr, t_span, C.byref(opts), None, t_dev.ptr,   # noqa: E731
                                                           info.ptr, None))
    ms = {"cloudy_tsit5_adaptive": bench._sustained_ms(pkg, plain, min_reps=3)}
    for n_save in (0, 1, 16):
        times = (C.c_double * max(n_save, 1))(*[t_span * (j + 1) / n_save for j in range(n_save)])
        saved = pkg.DeviceArray(max(n_save, 1) * plan.nmom, n)
        call = lambda: pkg._lib.check(L.cloudy_tsit5_adaptive_saveat(plan.handle, n, n, u0.ptr, out.ptr, t_span, C.byref(opts), None,   # noqa: E731
                                                                     t_dev.ptr, info.ptr, None, n_save, times, saved.ptr))
        ms[f"saveat n_save = {n_save}"] = bench._sustained_ms(pkg, call, min_reps=3)
        saved.free()
    base = ms["cloudy_tsit5_adaptive"]
    print(f"cfg3a, {n} parcels to t = {t_span:g}, reltol {a.reltol:g}: " + " | ".join(f"{k} {v:.3f} ms ({v / base:.3f} x)" for k, v in ms.items()) +
          f" | snapshot traffic n_save x {plan.nmom} planes x 8 B = {plan.nmom * 8} B per parcel and save time (state in + out: "
          f"{2 * plan.nmom * 8} B)", flush=True)


def cmd_spectra(a, pkg, L):
    """ms per call of cloudy_moments (1 and 8 orders, full and partial) and cloudy_density (16 and 100 grid points), per mode, on the
    cfg3a batch, each beside a fill of as many output planes"""
    n = a.parcels or 10_000_000
    wl = bench.make_workload("cfg3a", 1)
    plan = wl["coal_data"].plan(wl["dist_types"])
    mom = bench.synth_moments(2, n, 7)
    u0 = pkg.DeviceArray.from_numpy(mom)
    all_orders = (0.0, 0.25, 2.0 / 3.0, 1.0, 7.0 / 6.0, 2.0, 3.5, 6.0)
    budget = plan.N * len(all_orders) * n   # output elements of the largest moments call: the density calls stay within them

    def report(what, planes, m, call):
        out = pkg.DeviceArray(planes, m)
        ms = bench._sustained_ms(pkg, lambda: pkg._lib.check(call(out)), min_reps=3)
        fill = bench._sustained_ms(pkg, lambda: pkg._lib.check(L.cloudy_memset(out.ptr, 0, out.nbytes, None)), min_reps=3)
        out.free()
        print(f"cfg3a, {m} parcels: {what}: {ms:.3f} ms, fill of {planes} planes {fill:.3f} ms ({ms / fill:.2f} x), "
              f"{planes * 8} B stored + {plan.nmom * 8} B read per parcel", flush=True)

    for n_orders in (1, 8):
        arr = (C.c_double * n_orders)(*all_orders[-n_orders:])
        for x_t in (float("inf"), 1e-9):
            report(f"cloudy_moments, {n_orders} order(s), {'full' if np.isinf(x_t) else 'up to 1e-9 kg'}", plan.N * n_orders, n,
                   lambda out: L.cloudy_moments(plan.handle, n, n, u0.ptr, n_orders, arr, x_t, 1, out.ptr, None))
    for n_x in (16, 100):
        m = min(n, budget // (n_x * plan.N))
        grid = pkg.DeviceArray.from_numpy(np.logspace(-14, -5, n_x).reshape(1, -1))
        um = pkg.DeviceArray.from_numpy(mom[:, :m])   # (one leading dimension for the moments and the densities: m)
        report(f"cloudy_density, {n_x} grid points", n_x * plan.N, m,
               lambda out: L.cloudy_density(plan.handle, m, m, um.ptr, 0, n_x, grid.ptr, 1, out.ptr, None))
        um.free()


def cmd_boxadaptive(a, pkg, L):
    """ms per call on the batch of cmd_adaptive: cloudy_tsit5_adaptive, and cloudy_box_tsit5_adaptive with COAL | COND, COND alone and
    COAL | COND with 16 save times (a supersaturation per parcel, U(-0.02, 0.05)); the active-lane fraction of each from its info planes"""
    n, t_span = a.parcels or 10_000_000, a.t_span
    wl = bench.make_workload("cfg3a", 1)
    plan = wl["coal_data"].plan(wl["dist_types"])
    mom = bench.synth_moments(2, n, 7, degenerate_frac=0.0)
    u0, out = pkg.DeviceArray.from_numpy(mom), pkg.DeviceArray.zeros(*mom.shape)
    s_dev = pkg.DeviceArray.from_numpy(np.random.default_rng(0).uniform(-0.02, 0.05, n)[None, :])
    info, t_dev = pkg.DeviceArray.zeros(3, n, np.int32), pkg.DeviceArray.zeros(1, n)
    opts = pkg._lib.AdaptiveOptsC()
    L.cloudy_adaptive_opts_init(C.byref(opts))
    opts.reltol = a.reltol

    def lane_fraction():
        counts = info.to_numpy()
        attempts = (counts[0] + counts[1]).astype(np.int64)
        waves = np.pad(attempts, (0, -n % 64)).reshape(-1, 64)
        return attempts.sum() / (64 * waves.max(axis=1)).sum(), int((counts[2] != 0).sum())

    plain = lambda: pkg._lib.check(L.cloudy_tsit5_adaptive(plan.handle, n, n, u0.ptr, out.ptr, t_span, C.byref(opts), None, t_dev.ptr,   # noqa: E731
                                                           info.ptr, None))
    ms = {"cloudy_tsit5_adaptive": (bench._sustained_ms(pkg, plain, min_reps=3),) + lane_fraction()}
    for name, sources, n_save in (("COAL | COND", 3, 0), ("COND", 2, 0), ("COAL | COND, n_save = 16", 3, 16)):
        times = (C.c_double * max(n_save, 1))(*[t_span * (j + 1) / n_save for j in range(n_save)])
        saved = pkg.DeviceArray(max(n_save, 1) * plan.nmom, n)
        call = lambda: pkg._lib.check(L.cloudy_box_tsit5_adaptive(plan.handle, n, n, u0.ptr, out.ptr, sources, s_dev.ptr, 0.0, a.xi, t_span,   # noqa: E731
                                                                  C.byref(opts), None, t_dev.ptr, info.ptr, None, n_save,
                                                                  times if n_save else None, saved.ptr if n_save else None))
        ms[name] = (bench._sustained_ms(pkg, call, min_reps=3),) + lane_fraction()
        saved.free()
    base = ms["cloudy_tsit5_adaptive"][0]
    print(f"cfg3a, {n} parcels to t = {t_span:g}, reltol {a.reltol:g}, xi {a.xi:g}: " +
          " | ".join(f"{k} {v[0]:.3f} ms ({v[0] / base:.3f} x), active lanes {v[1]:.3f}, status != 0: {v[2]}" for k, v in ms.items()), flush=True)


def cmd_parceladaptive(a, pkg, L):
    """ms per call of cloudy_parcel_tsit5_adaptive (n_save = 0 and 41) beside cloudy_parcel_ssprk33_steps (40 fixed steps) on the
    decade batch and on the driver's uniform batch; the active-lane fraction of the adaptive calls from their info planes"""
    n, t_span = a.parcels or 10_000_000, a.t_span
    c = pkg.ParcelParams()
    d, keep = pkg.Plan.make_desc([2], np.array([[1.0]]), (float("inf"),), (1e8, 1e-12), 0)
    handle = C.c_void_p()
    pkg._lib.check(L.cloudy_plan_create(C.byref(d), C.byref(handle)))
    m0_drop = 4 / 3 * np.pi * 8e-6**3 * 1000.0
    dcp = c.cp_v - c.cp_l
    T0, p0 = 280.15, 8e4
    e = c.press_triple * (T0 / c.T_triple) ** (dcp / c.R_v) * np.exp((c.LH_v0 - dcp * c.T_0) / c.R_v * (1 / c.T_triple - 1 / T0))
    m_d, m_v = (p0 - e) / c.R_d / T0, e / c.R_v / T0

    def batch(N, w):   # parcel_example.jl:174-179, 218 per parcel
        M1 = N * m0_drop
        return np.ascontiguousarray(np.stack([np.ones(n), np.full(n, p0), np.full(n, T0), m_v / (m_d + m_v + M1), N, M1])), w

    rng = np.random.default_rng(5)
    batches = {"decade batch": batch(2e8 * 10.0 ** rng.uniform(-1.0, 1.0, n), rng.uniform(0.5, 10.0, n)),
               "uniform batch (N = 2e8, w = 10)": batch(np.full(n, 2e8), np.full(n, 10.0))}
    opts = pkg._lib.AdaptiveOptsC()
    L.cloudy_adaptive_opts_init(C.byref(opts))
    opts.reltol = a.reltol
    cc = c.to_c()
    info, t_dev, out = pkg.DeviceArray.zeros(3, n, np.int32), pkg.DeviceArray.zeros(1, n), pkg.DeviceArray.zeros(6, n)
    n_save = 41
    times = (C.c_double * n_save)(*[t_span * j / (n_save - 1) for j in range(n_save)])
    saved = pkg.DeviceArray(n_save * 6, n)
    for name, (y, w) in batches.items():
        y0, w_dev = pkg.DeviceArray.from_numpy(y), pkg.DeviceArray.from_numpy(w[None, :])
        res = []
        for k in (0, n_save):
            call = lambda: pkg._lib.check(L.cloudy_parcel_tsit5_adaptive(handle, n, n, y0.ptr, out.ptr, pkg.SRC_COND, w_dev.ptr, 0.0,   # noqa: E731
                                                                         C.byref(cc), t_span, C.byref(opts), None, t_dev.ptr, info.ptr,
                                                                         None, k, times if k else None, saved.ptr if k else None))
            ms = bench._sustained_ms(pkg, call, min_reps=3)
            counts = info.to_numpy()
            attempts = (counts[0] + counts[1]).astype(np.int64)
            waves = np.pad(attempts, (0, -n % 64)).reshape(-1, 64)
            res.append(f"adaptive, n_save = {k}: {ms:.3f} ms, attempts {attempts.min()} .. {attempts.max()} (mean {attempts.mean():.1f}), "
                       f"active lanes {attempts.sum() / (64 * waves.max(axis=1)).sum():.3f}, status != 0: {int((counts[2] != 0).sum())}")
        fixed = lambda: pkg._lib.check(L.cloudy_parcel_ssprk33_steps(handle, n, n, y0.ptr, out.ptr, pkg.SRC_COND, w_dev.ptr, 0.0,   # noqa: E731
                                                                     C.byref(cc), t_span / 40, 40, None))
        res.append(f"cloudy_parcel_ssprk33_steps, 40 steps of {t_span / 40:g}: {bench._sustained_ms(pkg, fixed, min_reps=3):.3f} ms")
        print(f"{name}, {n} parcels to t = {t_span:g}, reltol {a.reltol:g}: " + " | ".join(res), flush=True)
        y0.free()
        w_dev.free()
    L.cloudy_plan_destroy(handle)


def cmd_box(a, pkg, L):
    """ms per call of S steps: (a) cloudy_ssprk33_steps, (b) / (c) cloudy_box_ssprk33_steps with COAL | COND / COND, (d) the same
    steps stage by stage: two right-hand-side launches and the update on the planes (torch, on the same stream) per stage"""
    here = os.path.dirname(os.path.abspath(__file__))   # torch imports the standard library's timeit: this file must not shadow it
    sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") != here]
    import torch

    n, steps, xi, dt = a.parcels or 10_000_000, a.steps, 1e-8, C.c_double(1e-3)
    s_host = np.random.default_rng(0).uniform(-0.02, 0.05, n)
    for name in ("cfg3a", "cfg3b"):
        wl = bench.make_workload(name, n, seed=7)
        plan = wl["coal_data"].plan(wl["dist_types"])
        u0, out = pkg.DeviceArray.from_numpy(wl["mom"]), pkg.DeviceArray.zeros(*wl["mom"].shape)
        s = pkg.DeviceArray.from_numpy(s_host[None, :])
        both = pkg.SRC_COAL | pkg.SRC_COND
        ms_a = bench._sustained_ms(pkg, lambda: pkg._lib.check(L.cloudy_ssprk33_steps(plan.handle, n, n, u0.ptr, out.ptr, dt, steps, None)))
        ms_b = bench._sustained_ms(pkg, lambda: pkg._lib.check(
            L.cloudy_box_ssprk33_steps(plan.handle, n, n, u0.ptr, out.ptr, both, s.ptr, 0.0, xi, dt, steps, None)))
        ms_c = bench._sustained_ms(pkg, lambda: pkg._lib.check(
            L.cloudy_box_ssprk33_steps(plan.handle, n, n, u0.ptr, out.ptr, pkg.SRC_COND, s.ptr, 0.0, xi, dt, steps, None)))
        t0 = torch.from_numpy(wl["mom"]).cuda()
        u, up, f, g = (torch.empty_like(t0) for _ in range(4))
        h = dt.value

        def unfused():
            u.copy_(t0)
            for _ in range(steps):
                up.copy_(u)
                for stage in range(3):
                    pkg._lib.check(L.cloudy_coal_rhs(plan.handle, n, n, u.data_ptr(), f.data_ptr(), None))
                    pkg._lib.check(L.cloudy_cond_evap(plan.handle, n, n, u.data_ptr(), s.ptr, 0.0, xi, g.data_ptr(), None))
                    f.add_(g)
                    if stage == 0:
                        torch.add(up, f, alpha=h, out=u)
                    elif stage == 1:
                        u.add_(f, alpha=h).add_(up, alpha=3.0).mul_(0.25)
                    else:
                        u.mul_(2.0).add_(f, alpha=2.0 * h).add_(up).div_(3.0)

        ms_d = bench._sustained_ms(pkg, unfused, min_reps=3)
        # the two paths compute the same steps (to the roundings of the update formulas)
        pkg._lib.check(L.cloudy_box_ssprk33_steps(plan.handle, n, n, u0.ptr, out.ptr, both, s.ptr, 0.0, xi, dt, steps, None))
        unfused()
        got, want = out.columns_to_numpy(20000), u[:, :20000].cpu().numpy()
        fin = np.isfinite(want) & np.isfinite(got)
        dev = float(np.max(np.abs(got - want)[fin] / np.maximum((np.abs(wl["mom"][:, :20000]) + np.abs(want))[fin], 1e-300)))
        print(f"{name}, {n} parcels, {steps} steps per call: (a) cloudy_ssprk33_steps {ms_a:.3f} ms | (b) box COAL|COND {ms_b:.3f} ms | "
              f"(c) box COND {ms_c:.3f} ms | (d) unfused coal_rhs + cond_evap + torch updates {ms_d:.3f} ms | b/a {ms_b / ms_a:.2f} | "
              f"d/b {ms_d / ms_b:.2f} | (b) = {3 * steps * n / ms_b * 1e3:.3e} parcel-RHS/s | fused vs unfused state, first 20000 "
              f"parcels: {dev:.1e} of |u0| + |u|", flush=True)
        del u, up, f, g, t0, u0, out


def cmd_parcel(a, pkg, L):
    """ms per call of S steps of the adiabatic parcel (parcel_example.jl's mixture case, N and m0 scaled per parcel)"""
    here = os.path.dirname(os.path.abspath(__file__))   # (as cmd_box)
    sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") != here]
    import torch

    n, steps, dt, w = a.parcels or 10_000_000, a.steps, 0.5, 10.0
    norms, types = (1e8, 1e-12), [0, 1]
    cd = pkg.CoalescenceData(pkg.CoalescenceTensor([[1.0]]), (2, 3), (float("inf"),) * 2, norms)
    plan = cd.plan(types)
    c = pkg.ParcelParams()
    rng = np.random.default_rng(0)
    N, m0 = 2e8 * rng.uniform(0.5, 2, n), 4 / 3 * np.pi * 8e-6**3 * 1000.0 * rng.uniform(0.5, 2, n)
    T, p, S = rng.uniform(270, 290, n), rng.uniform(6e4, 9e4, n), rng.uniform(0.99, 1.01, n)
    dcp = c.cp_v - c.cp_l

    def p_vs(T, exp=np.exp):
        return c.press_triple * (T / c.T_triple) ** (dcp / c.R_v) * exp((c.LH_v0 - dcp * c.T_0) / c.R_v * (1 / c.T_triple - 1 / T))

    th = (N * m0 / 2) / (N / 10) / 2
    y_host = np.stack([S, p, T, 0.622 * S * p_vs(T) / p, 0.9 * N, N * m0 / 2, 0.1 * N, N * m0 / 2, 0.1 * N * th * th * 6])
    y0, out = pkg.DeviceArray.from_numpy(y_host), pkg.DeviceArray.zeros(*y_host.shape)
    cc = c.to_c()
    fused = lambda: pkg._lib.check(L.cloudy_parcel_ssprk33_steps(plan.handle, n, n, y0.ptr, out.ptr, pkg.SRC_COND, None, w, C.byref(cc),   # noqa: E731
                                                                 dt, steps, None))
    ms_a = bench._sustained_ms(pkg, fused)
    u0, uo = pkg.DeviceArray.from_numpy(y_host[4:]), pkg.DeviceArray.zeros(5, n)
    ms_c = bench._sustained_ms(pkg, lambda: pkg._lib.check(
        L.cloudy_box_ssprk33_steps(plan.handle, n, n, u0.ptr, uo.ptr, pkg.SRC_COND, None, 0.01, 8e-8, dt, steps, None)))
    t0 = torch.from_numpy(y_host).cuda()
    y, yp, f = (torch.empty_like(t0) for _ in range(3))
    s_eff = torch.empty(n, dtype=torch.float64, device="cuda")
    rvd, g = c.R_v / c.R_d, c.grav

    def rhs():   # f = dY(y): torch thermodynamics, cloudy_cond_evap with xi = 1 and s = xi(T) (S - 1) (1000 / rho_l)^(1/3) per parcel
        S_, p_, T_, q_ = y[0], y[1], y[2], y[3]
        m_liq = y[5] + y[7]
        q_l = m_liq * (c.R_d * (1 + (rvd - 1) * q_) * T_) / p_
        q_t = q_ + q_l
        R = c.R_d * (1 + (rvd - 1) * q_t - rvd * q_l)
        cp = c.cp_d + (c.cp_v - c.cp_d) * q_t + (c.cp_l - c.cp_v) * q_l
        Lv = c.LH_v0 + dcp * (T_ - c.T_0)
        xi = 1 / (Lv / (c.K_therm * T_) * (Lv / (c.R_v * T_) - 1) + c.R_v * T_ / (c.D_vapor * p_vs(T_, torch.exp)))
        torch.mul(xi, S_ - 1, out=s_eff)
        s_eff.mul_((1000.0 / c.rho_l) ** (1 / 3))
        pkg._lib.check(L.cloudy_cond_evap(plan.handle, n, n, y[4:].data_ptr(), s_eff.data_ptr(), 0.0, 1.0, f[4:].data_ptr(), None))
        dq = (f[5] + f[7]) * (R * T_) / p_
        f[0] = (Lv * g / (cp * T_ * T_ * c.R_v) - g / (R * T_)) * w * S_ - (1 / q_ + Lv * Lv / (c.R_v * T_ * T_ * cp)) * S_ * dq
        f[1] = -p_ * g * w / (R * T_)
        f[2] = (Lv * dq - g * w) / cp
        f[3] = -dq

    def staged():
        y.copy_(t0)
        for _ in range(steps):
            yp.copy_(y)
            for stage in range(3):
                rhs()
                if stage == 0:
                    torch.add(yp, f, alpha=dt, out=y)
                elif stage == 1:
                    y.add_(f, alpha=dt).add_(yp, alpha=3.0).mul_(0.25)
                else:
                    y.mul_(2.0).add_(f, alpha=2.0 * dt).add_(yp).div_(3.0)

    ms_b = bench._sustained_ms(pkg, staged, min_reps=3)
    fused()
    staged()
    got, want = out.columns_to_numpy(20000), y[:, :20000].cpu().numpy()
    dev = np.abs(got - want) / (np.abs(y_host[:, :20000]) + np.abs(want))
    dev[0] = np.abs(got[0] - want[0]) / np.maximum(np.abs(want[0] - 1), np.abs(y_host[0, :20000] - 1))
    print(f"parcel (Exponential + Gamma), {n} parcels, {steps} steps per call: (a) cloudy_parcel_ssprk33_steps {ms_a:.3f} ms | (b) staged "
          f"cloudy_cond_evap + torch thermodynamics and updates {ms_b:.3f} ms | (c) cloudy_box_ssprk33_steps COND {ms_c:.3f} ms | "
          f"b/a {ms_b / ms_a:.2f} | a/c {ms_a / ms_c:.2f} | (a) = {3 * steps * n / ms_a * 1e3:.3e} parcel-RHS/s | fused vs staged state, "
          f"first 20000 parcels: {float(dev.max()):.1e}", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    k = sub.add_parser("kernels")
    k.add_argument("names", nargs="+")
    k.add_argument("--reps", type=int, default=5)
    k.add_argument("--parcels", type=int, default=0)
    k.add_argument("--error", action="store_true")
    k.add_argument("--dtype", type=int, default=0)
    c = sub.add_parser("conv")
    c.add_argument("kernel")
    c.add_argument("dists")
    c.add_argument("n", nargs="?", type=int, default=4_000_000)
    c.add_argument("--reps", type=int, default=3)
    c.add_argument("--fused", action="store_true")
    c.add_argument("--fixed", type=int, default=0)
    c.add_argument("--lognorm-example", action="store_true")
    r = sub.add_parser("columns")
    r.add_argument("--nz", type=int, default=20)
    r.add_argument("--cells", type=int, default=10_000_000)
    r.add_argument("--workload", default="cfg3b")
    r.add_argument("--steps", type=int, default=2)
    cc = sub.add_parser("colcond")
    cc.add_argument("--nz", type=int, default=20)
    cc.add_argument("--cells", type=int, default=10_000_000)
    cc.add_argument("--workload", default="cfg3b")
    cc.add_argument("--steps", type=int, default=2)
    ca = sub.add_parser("coladaptive")
    ca.add_argument("--nz", type=int, default=20)
    ca.add_argument("--cells", type=int, default=10_000_000)
    ca.add_argument("--workload", default="cfg3b")
    ca.add_argument("--t-span", type=float, default=2.0)
    ca.add_argument("--reltol", type=float, default=1e-6)
    ca.add_argument("--max-steps", type=int, default=200)
    ca.add_argument("--n-save", type=int, default=0, help="K > 0: cloudy_rainshaft_tsit5_adaptive_saveat with 0, 1 and K save times as well")
    i = sub.add_parser("integrators")
    i.add_argument("--parcels", type=int, default=0)
    b = sub.add_parser("box")
    b.add_argument("--parcels", type=int, default=0)
    b.add_argument("--steps", type=int, default=4)
    pc = sub.add_parser("parcel")
    pc.add_argument("--parcels", type=int, default=0)
    pc.add_argument("--steps", type=int, default=2)
    ad = sub.add_parser("adaptive")
    ad.add_argument("--parcels", type=int, default=0)
    ad.add_argument("--t-span", type=float, default=5e-3)
    ad.add_argument("--reltol", type=float, default=1e-6)
    sv = sub.add_parser("saveat")
    sv.add_argument("--parcels", type=int, default=0)
    sv.add_argument("--t-span", type=float, default=5e-3)
    sv.add_argument("--reltol", type=float, default=1e-6)
    ba = sub.add_parser("boxadaptive")
    ba.add_argument("--parcels", type=int, default=0)
    ba.add_argument("--t-span", type=float, default=5e-3)
    ba.add_argument("--reltol", type=float, default=1e-6)
    ba.add_argument("--xi", type=float, default=1e-5)
    pa = sub.add_parser("parceladaptive")
    pa.add_argument("--parcels", type=int, default=0)
    pa.add_argument("--t-span", type=float, default=20.0)
    pa.add_argument("--reltol", type=float, default=1e-6)
    sp = sub.add_parser("spectra")
    sp.add_argument("--parcels", type=int, default=0)
    hh = sub.add_parser("host")
    hh.add_argument("--parcels", type=int, default=0)
    a = ap.parse_args()
    pkg = load_package()
    {"kernels": cmd_kernels, "conv": cmd_conv, "columns": cmd_columns, "colcond": cmd_colcond, "coladaptive": cmd_coladaptive, "integrators": cmd_integrators, "box": cmd_box, "parcel": cmd_parcel, "adaptive": cmd_adaptive,
     "saveat": cmd_saveat, "boxadaptive": cmd_boxadaptive, "parceladaptive": cmd_parceladaptive,
     "spectra": cmd_spectra, "host": cmd_host}[a.cmd](a, pkg, pkg.lib())


if __name__ == "__main__":
    main()
