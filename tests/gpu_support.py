"""What the GPU test modules share (not collected; imported as tsit5_restated is): tolerances, device and case helpers, the host
restatements of the fixed-step schemes, the sentinel NaNs with their bit-level predicates, the plans and batches that more than one
GPU file uses, and adaptive_call -- the one driver of the six C entry points of the adaptive Tsit5 family.

No test_gpu_*.py imports another: the cases and references chosen on the CPU live in the *_host.py modules, the restated loop in
tsit5_restated.py, everything else that is shared here."""
import ctypes as C
import functools

import numpy as np

import bench
from tsit5_restated import A_ROWS, default_opts

EPS = float(np.finfo(np.float64).eps)
INF = float("inf")
TOL_POLY = 1e-13   # all-Inf polynomial path (north_star: 1e-12)
TOL_QUAD = 1e-12   # Simpson / incomplete-gamma path, fp64 (north_star: 1e-8)
TOL_REL = 1e-10    # plain relative error of outputs that are not small differences of large terms


def dev(cloudy, a):
    return cloudy.DeviceArray.from_numpy(a)


def run_rhs(cloudy, par, mom, ts=None):
    rhs = cloudy.make_box_model_rhs(cloudy.AnalyticalCoalStyle(), ts)
    m = dev(cloudy, mom)
    dm = cloudy.DeviceArray.zeros(*mom.shape)
    rhs(dm, m, par, 0.0)
    return dm.to_numpy()


def make_case(cloudy, oracle, dist_types, kc, thr, norms, moving=False, k_range=(EPS, 10.0), vel=()):
    """product-side ODE parameters + oracle params for the same configuration"""
    N = len(dist_types)
    kc = np.asarray(kc, dtype=np.float64)
    if kc.ndim == 2:
        kc = np.broadcast_to(kc, (N, N) + kc.shape).copy()
    kernels = tuple(tuple(cloudy.CoalescenceTensor(kc[j, k]) for k in range(N)) for j in range(N))
    npm = tuple({0: 2, 1: 3, 2: 2, 3: 3}[t] for t in dist_types)
    ts = cloudy.MovingThreshold() if moving else cloudy.FixedThreshold()
    cd = cloudy.CoalescenceData(kernels, npm, thr, norms, ts)
    mk = {0: lambda: cloudy.ExponentialPrimitiveParticleDistribution(1.0, 1.0),
          1: lambda: cloudy.GammaPrimitiveParticleDistribution(1.0, 1.0, 1.0),
          2: lambda: cloudy.MonodispersePrimitiveParticleDistribution(1.0, 1.0),
          3: lambda: cloudy.LognormalPrimitiveParticleDistribution(1.0, 1.0, 1.0)}
    pd = tuple(mk[t]() for t in dist_types)
    extra = {"vel": vel} if len(vel) else {}
    par = cloudy.ODEParameters(pd, cd, npm, norms, k_range=k_range, **extra)
    op = oracle.make_params(list(dist_types), kc, thr, norms=norms, threshold_style=1 if moving else 0,
                            k_range=k_range, vel=vel)
    return par, op, ts


def assert_close_scaled(got, want, scale, tol, what=""):
    assert got.shape == want.shape
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_g, nan_w), f"{what}: NaN pattern differs"
    ok = ~nan_w
    err = np.abs(got[ok] - want[ok])
    bound = tol * scale[ok]
    bad = err > bound
    worst = (err / np.maximum(scale[ok], 1e-300)).max() if err.size else 0.0
    assert not bad.any(), f"{what}: max |diff|/scale = {worst:.3e} > {tol:g} ({bad.sum()} of {err.size})"
    if tol <= TOL_QUAD:   # fp64 comparisons: outputs that are not cancellations must also agree RELATIVELY
        big = np.abs(want[ok]) > 1e-3 * scale[ok]
        rel = err[big] / np.abs(want[ok][big])
        assert not (rel > TOL_REL).any(), f"{what}: max relative error of non-cancelling outputs {rel.max():.3e} > {TOL_REL:g}"
    return worst


def mixed_moments(dist_types, n, seed):
    """physical moments for a mixed Exp/Gamma mode list, (nmom, n)"""
    if len(dist_types) > 4:   # (bench.synth_moments knows the four size classes of the reference's examples)
        return many_mode_moments(dist_types, n, seed)[0]
    full = bench.synth_moments(len(dist_types), n, seed)
    rows = []
    for i, t in enumerate(dist_types):
        rows += [full[3 * i], full[3 * i + 1]] + ([full[3 * i + 2]] if t in (1, 3) else [])
    return np.ascontiguousarray(np.stack(rows))


def many_mode_moments(dist_types, n, seed):
    """physical moments of N size classes between 1e-12 and 1e-4 kg (one decade each for N = 8), number densities falling
    with size as in bench.synth_moments, 1 % degenerate parcels per mode; -> (moments, mask of the parcels without a degenerate mode)"""
    N = len(dist_types)
    regular = np.ones(n, dtype=bool)
    rng = np.random.Generator(np.random.Philox(key=seed))
    edges = np.logspace(-12, -4, N + 1)
    rows = []
    for i, t in enumerate(dist_types):
        hi = 1e9 * 10.0 ** (-1.5 * i * 8 / N)
        m = bench._gamma_mode(rng, n, hi * 1e-3, hi, 0.5 if i == 0 else 1.0, 7.0, edges[i], edges[i + 1])
        z = rng.choice(n, max(n // 100, 1), replace=False)
        m[:, z[: len(z) // 2]] = 0.0
        m[2, z[len(z) // 2:]] = m[1, z[len(z) // 2:]] ** 2 / m[0, z[len(z) // 2:]]
        regular[z] = False
        rows += [m[0], m[1]] + ([m[2]] if t in (1, 3) else [])
    return np.ascontiguousarray(np.stack(rows)), regular


def _ssprk33_host(rhs_fn, u, dt, n_steps):
    """OrdinaryDiffEq's SSPRK33 update formulas with a host-side RHS callable (numpy)."""
    u = u.copy()
    for _ in range(n_steps):
        up = u.copy()
        k = rhs_fn(u)
        u = up + dt * k
        k = rhs_fn(u)
        u = (3.0 * up + u + dt * k) / 4.0
        k = rhs_fn(u)
        u = (up + 2.0 * u + 2.0 * dt * k) / 3.0
    return u


def _tsit5_host(rhs_fn, u, dt, n_steps):
    """the Tsit5 tableau (Tsitouras 2011; OrdinaryDiffEq's Tsit5()) with a fixed step and a host-side RHS callable"""
    u = u.copy()
    for _ in range(n_steps):
        k = [rhs_fn(u)]
        for row in A_ROWS[:-1]:
            k.append(rhs_fn(u + dt * sum(a * ki for a, ki in zip(row, k))))
        u = u + dt * sum(a * ki for a, ki in zip(A_ROWS[-1], k))
    return u


def oracle_reference(oracle, op, mom, dt, n_steps, xi, s, coal, cond):
    """SSPRK33 with the oracle's right-hand sides"""
    def rhs(u):
        f = np.zeros_like(u)
        if coal:
            f = f + oracle.rhs_coal_batch(op, u)
        if cond:
            f = f + oracle.rhs_condensation_batch(op, xi, s, u)
        return f

    with np.errstate(all="ignore"):
        return _ssprk33_host(rhs, mom, dt, n_steps)


def rel_err(got, want, mom, ok):
    ref = np.abs(mom) + np.abs(want)
    return np.abs(got - want)[:, ok] / np.maximum(ref[:, ok], 1e-300)


# ---- sentinels: NaNs no arithmetic produces, and what the tests ask of bits
SENTINEL = np.float64(np.nan).view(np.uint64) | np.uint64(0x5EED)
SENTINEL32 = np.uint32(0x7FC00000 | 0x5EED)


def blank(planes, ld, dtype=np.float64):
    """(planes, ld) of the sentinel NaN of the plane type"""
    f64 = dtype == np.float64
    return np.full((planes, ld), SENTINEL if f64 else SENTINEL32, dtype=np.uint64 if f64 else np.uint32).view(dtype)


def is_blank(x):
    """elementwise: still the sentinel of its width (x: fp64 / float planes, or their bits)"""
    return x.view(np.uint64) == SENTINEL if x.dtype.itemsize == 8 else x.view(np.uint32) == SENTINEL32


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def same_counts(got, ref):
    return (got["accepted"] == ref["accepted"]) & (got["rejected"] == ref["rejected"])


# ---- NumericalCoalStyle cases (tests/test_gpu_numerical.py; the integrators' tests of test_gpu_parity.py)
def kernel_funcs(cloudy, oracle):
    return {
        "constant": (cloudy.ConstantKernelFunction(1e-4), oracle.kernel_func(oracle.KF_CONSTANT, 1e-4)),
        "linear": (cloudy.LinearKernelFunction(5.0), oracle.kernel_func(oracle.KF_LINEAR, 5.0)),
        "hydro": (cloudy.HydrodynamicKernelFunction(1e2 * np.pi), oracle.kernel_func(oracle.KF_HYDRODYNAMIC, 1e2 * np.pi)),
        "long": (cloudy.LongKernelFunction(5.236e-10, 9.44e9, 5.78), oracle.kernel_func(oracle.KF_LONG, 5.236e-10, 9.44e9, 5.78)),
    }


def numerical_case(cloudy, oracle, dist_types, kname, nq=10, k_range=None):
    """product-side ODE parameters (p.kernel_func normalised, as the reference's drivers pass it) + oracle params"""
    kf, okf = kernel_funcs(cloudy, oracle)[kname]
    mk = {0: lambda: cloudy.ExponentialPrimitiveParticleDistribution(1.0, 1.0),
          1: lambda: cloudy.GammaPrimitiveParticleDistribution(1.0, 1.0, 1.0),
          3: lambda: cloudy.LognormalPrimitiveParticleDistribution(1.0, 1.0, 1.0)}
    pd = tuple(mk[t]() for t in dist_types)
    npm = tuple({0: 2, 1: 3, 3: 3}[t] for t in dist_types)
    extra = {"k_range": k_range} if k_range else {}
    par = cloudy.ODEParameters(pd, None, npm, bench.NORMS, kernel_func=cloudy.get_normalized_kernel_func(kf, bench.NORMS),
                               quad_order=nq, quad_mode=cloudy.QUAD_FIXED, **extra)
    op = oracle.make_params(list(dist_types), np.zeros((1, 1)), (INF,) * len(dist_types), norms=bench.NORMS,
                            **({"k_range": k_range} if k_range else {}))
    return par, op, oracle.get_normalized_kernel_func(okf, bench.NORMS)


def converged_case(cloudy, oracle, dist_types, kname, q=8):
    par, op, okf = numerical_case(cloudy, oracle, dist_types, kname, q)
    par.quad_mode = cloudy.QUAD_CONVERGED
    return par, op, okf


# ---- the adiabatic parcel's driver cases (tests/test_gpu_parcel.py, tests/test_gpu_parcel_adaptive.py)
def mass_rows(dist_types):
    rows, off = [], 0
    for t in dist_types:
        rows.append(off + 1)
        off += 3 if t in (1, 3) else 2
    return rows


def driver_case(name):
    """init_conditions of parcel_example.jl:114-146 -> (dist_types, moments)"""
    from test_parcel_host import M0_DROP, N0

    N, m0 = N0, M0_DROP
    if name == "monodisperse":
        return [2], [N, N * m0]
    if name == "gamma":   # k = 2, theta = m0 / 2
        return [1], [N, N * m0, N * (m0 / 2) ** 2 * 6]
    th_g = (N * m0 / 2) / (N / 10) / 2   # mixture: Exponential(0.9 N, .) + Gamma(0.1 N, ., 2), half the mass each
    return [0, 1], [0.9 * N, N * m0 / 2, 0.1 * N, N * m0 / 2, 0.1 * N * th_g**2 * 6]


# ---- the rainshaft column batch (tests/test_gpu_column_*.py and the column *_host.py modules)
XI = 1e-8
VEL = ((50.0, 1.0 / 6),)
GOLOVIN = [[EPS / 1e6, 5.0], [5.0, 0.0]]
NZ, DZ, DT, NCOL = 20, 150.0, 1.0, 27   # 25 columns per 512-thread workgroup at 20 cells: 27 spill into a second one


def supersaturation(nz, dz, ncol):
    """one value per cell in the cell order of the state (cell col * nz + iz): 0.03 in the cloud layer (z >= 1350 m), -0.2 below,
    scaled by a factor that differs from column to column -- a wrong cell-to-s mapping cannot pass"""
    z = (np.arange(nz) + 0.5) * dz
    prof = np.where(z >= 1350.0, 0.03, -0.2)
    return np.concatenate([(0.5 + 0.05 * c) * prof for c in range(ncol)])


def reference_case(cloudy, oracle, case):
    """par, op, dist_types, amp of the two configurations of test_rainshaft_column_integrator_ssprk33"""
    if case == "gamma_mixture":   # rainshaft_gamma_mixture.jl:15-60: the ranked body
        dist_types, thr, amp = [1, 1], (2e-10, INF), np.array([1e7, 1e-3, 2e-13, 0.0, 0.0, 0.0])
    else:                         # rainshaft_single_gamma.jl: the all-Inf body
        dist_types, thr, amp = [1], (INF,), np.array([1e7, 1e-3, 2e-13])
    par, op, _ = make_case(cloudy, oracle, dist_types, GOLOVIN, thr, bench.NORMS, vel=VEL)
    par.dz, par.nz, par.dt = DZ, NZ, DT
    return par, op, dist_types, amp


def column_set(amp):
    """the columns of test_rainshaft_column_integrator_ssprk33 (scaled slabs, the slab touching the top, the cell with -1e-30),
    extended to 27 columns"""
    z = (np.arange(NZ) + 0.5) * DZ
    at = ((z >= 0.5 * z.max() - DZ / 2) & (z < 0.75 * z.max() - DZ / 2)).astype(float)
    cols = [np.outer(amp * s, at) for s in (1.0, 0.3, 3.0)]
    shifted = np.outer(amp, np.roll(at, 3))
    dirty = np.outer(amp, at)
    dirty[:, 2] = -1e-30
    cols += [shifted, dirty] + [np.outer(amp * (0.5 + 0.1 * i), at) for i in range(NCOL - 5)]
    return np.ascontiguousarray(np.concatenate(cols, axis=1))


def moving_column_case(cloudy, oracle):
    """A MovingThreshold two-mode column configuration -> (par, threshold style, dist_types, three columns of column_set)"""
    par, _, ts = make_case(cloudy, oracle, [1, 1], GOLOVIN, (0.9, 1.0), bench.NORMS, moving=True, vel=VEL)
    par.nz, par.dz, par.dt = NZ, DZ, DT
    return par, ts, [1, 1], column_set(np.array([1e7, 1e-3, 2e-13, 1e4, 1e-4, 2e-12]))[:, : 3 * NZ].copy()


@functools.lru_cache(maxsize=None)
def _column_plan(cloudy, oracle, case, dtype, kw):
    par, _, dist_types, _ = reference_case(cloudy, oracle, case)
    return par, par.coal_data.plan(dist_types, vel=VEL, dtype=dtype, **dict(kw))


def column_plan(cloudy, oracle, case, dtype=0, **kw):
    """(par, plan) of a reference_case, one per session"""
    return _column_plan(cloudy, oracle, case, dtype, tuple(sorted(kw.items())))


# ---- the plans of the per-parcel adaptive tests (tests/test_tsit5_adaptive_host.py picks the cases)
SIZES = (1, 65, 257)


@functools.lru_cache(maxsize=None)
def golovin_plan(cloudy, oracle, dist):
    import test_tsit5_adaptive_host as H

    par, op, _ = make_case(cloudy, oracle, [1 if dist == "gamma" else 0], H.GOLOVIN_KC, (INF,), bench.NORMS)
    return par, op, par.coal_data.plan([1 if dist == "gamma" else 0])


@functools.lru_cache(maxsize=None)
def two_gamma_plan(cloudy, oracle, kind, dtype=0, specialize=0):
    import test_tsit5_adaptive_host as H

    _, kc, thr, moving = H.two_gamma_case(oracle, kind)
    par, op, _ = make_case(cloudy, oracle, [1, 1], kc, thr, bench.NORMS, moving=moving)
    return par, op, par.coal_data.plan([1, 1], dtype=dtype, specialize=specialize)


# ---- one driver for the six C entry points of the adaptive Tsit5 family
# entry: (one controller per column of nz cells, the arguments between u_out and t_span, takes save times).  "forcing" stands for
# the pointer / value pair of s (box, columns) or w (parcel).
ENTRIES = {
    "cloudy_tsit5_adaptive": (False, (), False),
    "cloudy_tsit5_adaptive_saveat": (False, (), True),
    "cloudy_box_tsit5_adaptive": (False, ("sources", "forcing", "xi"), True),
    "cloudy_parcel_tsit5_adaptive": (False, ("sources", "forcing", "params"), True),
    "cloudy_rainshaft_tsit5_adaptive": (True, ("sources", "forcing", "xi", "dz"), False),
    "cloudy_rainshaft_tsit5_adaptive_saveat": (True, ("sources", "forcing", "xi", "dz"), True),
}


def adaptive_call(entry, cloudy, plan, u0, t_span, times=(), *, sources=3, forcing=None, xi=0.0, nz=1, ld=None, pad=7.0, in_place=False,
                  dt_in="zeros", no_outputs=False, save_null=True, expect=0, **opts):
    """One call of the C entry point `entry` on a host batch u0 (planes, n), in sentinel-filled buffers of leading dimension ld
    (default n) whose input columns n .. ld hold `pad` (None: the sentinel).  m controllers: m = n parcels, or n / nz columns.

    forcing: s of the box and the columns, w of the parcel -- None or a float by value, an array (n,) through the device pointer.
    dt_in: "zeros" -- dt_dev holds opts.dt_init for the columns (whose first step comes from there) and 0 for parcels; an array
    (m,) -- the caller's steps; None -- dt_dev = NULL.  no_outputs: dt_dev, t_dev and info_dev are all NULL.  times: t_save; with
    none, t_save and u_save are NULL unless save_null is False.  opts: fields of cloudy_adaptive_opts.

    Asserts the return code and, out of place, that the input buffer kept its bits.  -> dict: u, pad (the columns n .. ld of the
    output), u_in (the input buffer after the call), buf (before it), t, dt, accepted, rejected, status (m each; None where the
    pointer was NULL), saved (n_save, planes, n), saved_pad, guard (one snapshot's worth of planes behind the last: never
    written), saved_bits (all of u_save, guard included, as unsigned integers), message."""
    L = cloudy.lib()
    columns, middle, saves = ENTRIES[entry]
    planes, n = u0.shape
    ld = n if ld is None else ld
    m = n // nz
    lt = m if columns else ld                  # the length of dt_dev, t_dev and the rows of info_dev
    dtype = u0.dtype.type
    buf = blank(planes, ld, dtype) if pad is None else np.full((planes, ld), pad, dtype=dtype)
    buf[:, :n] = u0
    u_in = dev(cloudy, buf)
    u_out = u_in if in_place else dev(cloudy, blank(planes, ld, dtype))
    by_pointer = np.ndim(forcing) > 0
    f_dev = dev(cloudy, np.pad(np.asarray(forcing, dtype=np.float64), (0, ld - n))[None, :]) if by_pointer else None
    if dt_in is None or no_outputs:
        dt_dev = None
    elif isinstance(dt_in, str):
        dt_dev = dev(cloudy, np.full((1, lt), float(opts.get("dt_init", 0.0)) if columns else 0.0))
    else:
        dt_dev = dev(cloudy, np.pad(np.asarray(dt_in, dtype=np.float64), (0, lt - m))[None, :])
    t_dev = None if no_outputs else dev(cloudy, blank(1, lt))
    info = None if no_outputs else cloudy.DeviceArray.zeros(3, lt, np.int32)
    n_save = len(times)
    snap = dev(cloudy, blank((n_save + 1) * planes, ld, dtype))
    arr = (C.c_double * max(n_save, 1))(*times)
    o = default_opts(cloudy, **opts)
    params = cloudy.ParcelParams().to_c()
    ptr = lambda d: None if d is None else d.ptr   # noqa: E731
    piece = dict(sources=[sources], forcing=[ptr(f_dev), 0.0 if by_pointer or forcing is None else float(forcing)], xi=[xi], dz=[DZ],
                 params=[C.byref(params)])
    args = [plan.handle] + ([nz, m] if columns else [n]) + [ld, u_in.ptr, u_out.ptr] + [a for p in middle for a in piece[p]]
    args += [t_span, C.byref(o), ptr(dt_dev), ptr(t_dev), ptr(info), None]
    if saves:
        args += [n_save, arr if n_save or not save_null else None, snap.ptr if n_save or not save_null else None]
    rc = getattr(L, entry)(*args)
    message = L.cloudy_last_error().decode()
    assert rc == expect, (rc, message)
    cloudy._lib.check(L.cloudy_stream_synchronize(None))
    out, after, sv = u_out.to_numpy(), u_in.to_numpy(), snap.to_numpy()
    assert in_place or bits_equal(after, buf), "out of place: the input changed"
    counts = [None] * 3 if info is None else info.to_numpy()[:, :m]
    first = lambda d: None if d is None else d.to_numpy()[0, :m]   # noqa: E731
    bits = sv.view(np.uint64 if sv.dtype.itemsize == 8 else np.uint32)
    sv = sv.reshape(n_save + 1, planes, ld)
    return dict(u=out[:, :n], pad=out[:, n:], u_in=after, buf=buf, t=first(t_dev), dt=first(dt_dev), accepted=counts[0],
                rejected=counts[1], status=counts[2], saved=sv[:n_save, :, :n], saved_pad=sv[:n_save, :, n:], guard=sv[n_save],
                saved_bits=bits, message=message)


adaptive = functools.partial(adaptive_call, "cloudy_tsit5_adaptive")
saveat = functools.partial(adaptive_call, "cloudy_tsit5_adaptive_saveat", save_null=False)


def box_adaptive(cloudy, plan, u0, t_span, s, xi, **kw):
    """s: a float, or an array (through s_dev)"""
    return adaptive_call("cloudy_box_tsit5_adaptive", cloudy, plan, u0, t_span, forcing=s, xi=xi, **kw)


def column_run(cloudy, plan, u0, s, t_span, times=None, nz=NZ, xi=XI, **kw):
    """the column entry points on u0 (planes, nz * n_columns), input padding of sentinels; with `times` the one with dense output"""
    entry = "cloudy_rainshaft_tsit5_adaptive" + ("" if times is None else "_saveat")
    return adaptive_call(entry, cloudy, plan, u0, t_span, () if times is None else times, forcing=s, nz=nz, xi=xi, pad=None, **kw)
