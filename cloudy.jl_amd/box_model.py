"""The operator boundary: make_box_model_rhs (test/examples/utils/box_model_helpers.jl:22-53), batched.

    rhs = make_box_model_rhs(AnalyticalCoalStyle())          # same factory signature
    rhs(dm, m, par, t)                                        # same 4-argument in-place ODE function

`m`, `dm` are (nmom, n_parcels) device arrays (DeviceArray or CUDA torch tensors), i.e. Julia's m[parcel, moment].
`par` carries the fields rhs_coal! reads: pdists (types only), coal_data, NProgMoms, norms.
"""
from types import SimpleNamespace

import numpy as np

from . import _lib
from .device import DeviceArray, as_device, dtype_code
from .EquationTypes import AnalyticalCoalStyle, CoalescenceStyle, FixedThreshold, MovingThreshold, NumericalCoalStyle
from .ParticleDistributions import nparams

EPS = float(np.finfo(np.float64).eps)


def ODEParameters(pdists, coal_data, NProgMoms, norms, **extra):
    """The ODE_parameters NamedTuple of the examples (e.g. box_gamma_mixture.jl:29-35; NumericalCoalStyle drivers pass
    coal_data=None and kernel_func=<normalised kernel function>, Numerical/n_particles_gamma.jl:37-38)."""
    return SimpleNamespace(pdists=tuple(pdists), coal_data=coal_data, NProgMoms=tuple(NProgMoms), norms=tuple(norms),
                           **extra)


def _numerical_plan_for(par, dtype=0):
    from .Coalescence import numerical_plan

    if tuple(nparams(d) for d in par.pdists) != tuple(par.NProgMoms):
        raise ValueError("NProgMoms must equal nparams of p.pdists")
    return numerical_plan([d.type_id for d in par.pdists], par.kernel_func, par.norms,
                          quad_order=getattr(par, "quad_order", 0), k_range=getattr(par, "k_range", (EPS, 10.0)),
                          dtype=dtype, quad_mode=getattr(par, "quad_mode", 1))  # default: converged mode


def _plan_for(par, dtype=0):
    if tuple(nparams(d) for d in par.pdists) != tuple(par.NProgMoms):
        raise ValueError("NProgMoms must equal nparams of p.pdists")
    if tuple(par.norms) != tuple(par.coal_data.norms):
        raise ValueError("p.norms differs from the norms the CoalescenceData was built with")
    if dtype == 1 and getattr(par, "fast_f32", False):
        dtype = 2  # CLOUDY_F32_FAST: single-precision arithmetic in the per-node Simpson / incomplete-gamma pass
    return par.coal_data.plan([d.type_id for d in par.pdists], k_range=getattr(par, "k_range", (EPS, 10.0)),
                              vel=getattr(par, "vel", ()), dtype=dtype)


def rhs_coal(coal_type, dmom, mom, p, threshold_style, stream=None):
    """rhs_coal! (box_model_helpers.jl:29-53): normalise, invert closures, get_coal_ints, de-normalise --
    one fused HIP kernel per call."""
    if not isinstance(coal_type, (AnalyticalCoalStyle, NumericalCoalStyle)):
        raise ValueError("Invalid coal style!")
    if dtype_code(mom) != dtype_code(dmom):
        raise TypeError("mom and dmom must have the same element type")
    if isinstance(coal_type, NumericalCoalStyle):
        # get_coal_ints(coal_type, p.pdists, p.kernel_func), box_model_helpers.jl:47-48
        plan = _numerical_plan_for(p, dtype_code(mom))
    else:
        if isinstance(threshold_style, MovingThreshold) != isinstance(p.coal_data.ts, MovingThreshold):
            raise ValueError("threshold style of the RHS does not match the CoalescenceData")
        plan = _plan_for(p, dtype_code(mom))  # float32 arrays select a CLOUDY_F32 plan (fp32 planes, fp64 arithmetic)
    mptr, planes, n, ld = as_device(mom)
    dptr, dplanes, dn, dld = as_device(dmom)
    if planes != plan.nmom or dplanes != plan.nmom or dn != n or dld != ld:
        raise ValueError(f"mom and dmom must both be ({plan.nmom}, n) with equal leading dimension")
    _lib.check(_lib.lib().cloudy_coal_rhs(plan.handle, n, ld, mptr, dptr, stream))
    return dmom


def make_box_model_rhs(coal_type, threshold_style=None):
    """make_box_model_rhs(coal_type::CoalescenceStyle, threshold_style::ThresholdStyle = FixedThreshold())."""
    if not isinstance(coal_type, CoalescenceStyle):
        raise TypeError("coal_type must be a CoalescenceStyle")
    ts = threshold_style if threshold_style is not None else FixedThreshold()

    def rhs(dm, m, par, t):
        return rhs_coal(coal_type, dm, m, par, ts)

    return rhs


def solve_ssprk33(par, u, dt, n_steps, out=None, stream=None, coal_type=None):
    """solve(ODEProblem(rhs, u, tspan, par), SSPRK33(), dt = dt) for n_steps fixed steps, on the device
    (cloudy_ssprk33_steps): the final state only (the examples' `sol.u[end]`).  `u` is advanced in place unless
    `out` is given.  `coal_type`: the style the RHS was made with (make_box_model_rhs(coal_type)); default
    AnalyticalCoalStyle, NumericalCoalStyle() integrates get_coal_ints(::NumericalCoalStyle, p.pdists, p.kernel_func)."""
    if coal_type is not None and not isinstance(coal_type, (AnalyticalCoalStyle, NumericalCoalStyle)):
        raise ValueError("Invalid coal style!")
    plan = _numerical_plan_for(par, dtype_code(u)) if isinstance(coal_type, NumericalCoalStyle) else _plan_for(par, dtype_code(u))
    uptr, planes, n, ld = as_device(u)
    o = out if out is not None else u
    optr, oplanes, on, old = as_device(o)
    if planes != plan.nmom or oplanes != plan.nmom or on != n or old != ld:
        raise ValueError(f"u and out must both be ({plan.nmom}, n) with equal leading dimension")
    _lib.check(_lib.lib().cloudy_ssprk33_steps(plan.handle, n, ld, uptr, optr, float(dt), int(n_steps), stream))
    return o


def solve_tsit5(par, u, dt, n_steps, out=None, stream=None, coal_type=None):
    """solve(ODEProblem(rhs, u, tspan, par), Tsit5(), dt = dt, adaptive = false) for n_steps fixed steps, on the device
    (cloudy_tsit5_steps): BASELINE configs[0] names Tsit5; no reference driver uses it (they call SSPRK33).  Every plan
    solve_ssprk33 serves (thresholds Inf / fixed / moving, NumericalCoalStyle through `coal_type`), fp64 or float planes.
    `u` is advanced in place unless `out` is given."""
    if coal_type is not None and not isinstance(coal_type, (AnalyticalCoalStyle, NumericalCoalStyle)):
        raise ValueError("Invalid coal style!")
    plan = _numerical_plan_for(par, dtype_code(u)) if isinstance(coal_type, NumericalCoalStyle) else _plan_for(par, dtype_code(u))
    uptr, planes, n, ld = as_device(u)
    o = out if out is not None else u
    optr, oplanes, on, old = as_device(o)
    if planes != plan.nmom or oplanes != plan.nmom or on != n or old != ld:
        raise ValueError(f"u and out must both be ({plan.nmom}, n) with equal leading dimension")
    _lib.check(_lib.lib().cloudy_tsit5_steps(plan.handle, n, ld, uptr, optr, float(dt), int(n_steps), stream))
    return o


ADAPTIVE_STATUS = ("reached t_span", "max_steps attempts", "dt below 1e-14 t_span or not finite")


def solve_tsit5_adaptive(par, u, t_span, reltol=1e-6, abstol=1e-9, dt=None, max_steps=10000, out=None, dt_dev=None, info=False,
                         stream=None, coal_type=None):
    """Every parcel of `u` from t = 0 to t = t_span with adaptive Tsit5 under a step-size controller of its own, on the device
    (cloudy_tsit5_adaptive): the PI controller, error norm and statuses of include/cloudy_hip.h.  `reltol` is relative, `abstol` in
    normalised units (mom ./ norms); `dt`: the first step of every parcel (None: Hairer's first guess per parcel); `max_steps`
    bounds accepted + rejected steps per parcel.  `dt_dev`: an (1, n) fp64 device array, in/out -- the first step per parcel where
    positive, the next proposed step on return (a host model calling once per model step starts warm).  `u` is advanced in place
    unless `out` is given.  Returns the state; with info=True returns (accepted, rejected, status, t_reached) as numpy arrays
    (this synchronises) and raises RuntimeError naming the count and the first index if any status is not 0 -- AFTER the call: `u`
    (or `out`) and `dt_dev` already hold what every parcel reached, the stopped ones their state at the time they stopped.
    AnalyticalCoalStyle
    plans, fp64 or float planes; NumericalCoalStyle plans are refused (solve_tsit5 steps them with a fixed dt)."""
    import ctypes as C

    if coal_type is not None and not isinstance(coal_type, (AnalyticalCoalStyle, NumericalCoalStyle)):
        raise ValueError("Invalid coal style!")
    plan = _numerical_plan_for(par, dtype_code(u)) if isinstance(coal_type, NumericalCoalStyle) else _plan_for(par, dtype_code(u))
    uptr, planes, n, ld = as_device(u)
    o = out if out is not None else u
    optr, oplanes, on, old = as_device(o)
    if planes != plan.nmom or oplanes != plan.nmom or on != n or old != ld:
        raise ValueError(f"u and out must both be ({plan.nmom}, n) with equal leading dimension")
    dptr = None
    if dt_dev is not None:
        dptr, dplanes, dn, _ = as_device(dt_dev)
        if dplanes != 1 or dn != n or dtype_code(dt_dev) != 0:
            raise ValueError("dt_dev must be an (1, n) fp64 device array")
    L = _lib.lib()
    opts = _lib.AdaptiveOptsC()
    L.cloudy_adaptive_opts_init(C.byref(opts))
    opts.reltol, opts.abstol, opts.dt_init, opts.max_steps = float(reltol), float(abstol), 0.0 if dt is None else float(dt), int(max_steps)
    t_arr = DeviceArray.zeros(1, n) if info else None
    i_arr = DeviceArray.zeros(3, ld, dtype=np.int32) if info else None
    _lib.check(L.cloudy_tsit5_adaptive(plan.handle, n, ld, uptr, optr, float(t_span), C.byref(opts), dptr,
                                       t_arr.ptr if info else None, i_arr.ptr if info else None, stream))
    if not info:
        return o
    _lib.check(L.cloudy_stream_synchronize(stream))
    counts = i_arr.to_numpy()[:, :n]
    accepted, rejected, status = counts[0].copy(), counts[1].copy(), counts[2].copy()
    bad = np.flatnonzero(status)
    if bad.size:
        raise RuntimeError(f"solve_tsit5_adaptive: {bad.size} of {n} parcels did not reach t_span; the first is parcel {int(bad[0])} "
                           f"(status {int(status[bad[0]])}: {ADAPTIVE_STATUS[int(status[bad[0]])]})")
    return accepted, rejected, status, t_arr.to_numpy()[0]


def solve_tsit5_adaptive_saveat(par, u, t_span, saveat, reltol=1e-6, abstol=1e-9, dt=None, max_steps=10000, out=None, dt_dev=None,
                                info=False, stream=None, coal_type=None):
    """solve_tsit5_adaptive with dense output (cloudy_tsit5_adaptive_saveat): the same integration -- the step sequence of every
    parcel is the one solve_tsit5_adaptive takes, bit for bit -- and the state of every parcel at the batch-wide times `saveat`
    (host floats in [0, t_span], strictly increasing), from the free 4th-order interpolant of Tsit5 inside the accepted step that
    holds the time.  Returns the snapshots as a DeviceArray of shape (n_save * planes, ld) in the plane type of `u`: snapshot j,
    plane p is row j * planes + p; a snapshot at 0 equals the input and one at t_span the final state bit for bit; a parcel that
    stopped early has NaN in the snapshots it did not reach.  With info=True returns (snapshots, accepted, rejected, status,
    t_reached) and raises as solve_tsit5_adaptive does -- keep the snapshots of a run that may stop early with info=False and
    read the status planes through the C call.  Everything else as solve_tsit5_adaptive."""
    import ctypes as C

    if coal_type is not None and not isinstance(coal_type, (AnalyticalCoalStyle, NumericalCoalStyle)):
        raise ValueError("Invalid coal style!")
    plan = _numerical_plan_for(par, dtype_code(u)) if isinstance(coal_type, NumericalCoalStyle) else _plan_for(par, dtype_code(u))
    uptr, planes, n, ld = as_device(u)
    o = out if out is not None else u
    optr, oplanes, on, old = as_device(o)
    if planes != plan.nmom or oplanes != plan.nmom or on != n or old != ld:
        raise ValueError(f"u and out must both be ({plan.nmom}, n) with equal leading dimension")
    dptr = None
    if dt_dev is not None:
        dptr, dplanes, dn, _ = as_device(dt_dev)
        if dplanes != 1 or dn != n or dtype_code(dt_dev) != 0:
            raise ValueError("dt_dev must be an (1, n) fp64 device array")
    times = np.ascontiguousarray(np.atleast_1d(np.asarray(saveat, dtype=np.float64)))
    if times.ndim != 1:
        raise ValueError("saveat must be a sequence of times")
    n_save = int(times.size)
    saved = DeviceArray(n_save * planes, ld, dtype=np.float32 if dtype_code(u) else np.float64)
    L = _lib.lib()
    opts = _lib.AdaptiveOptsC()
    L.cloudy_adaptive_opts_init(C.byref(opts))
    opts.reltol, opts.abstol, opts.dt_init, opts.max_steps = float(reltol), float(abstol), 0.0 if dt is None else float(dt), int(max_steps)
    t_arr = DeviceArray.zeros(1, n) if info else None
    i_arr = DeviceArray.zeros(3, ld, dtype=np.int32) if info else None
    _lib.check(L.cloudy_tsit5_adaptive_saveat(plan.handle, n, ld, uptr, optr, float(t_span), C.byref(opts), dptr,
                                              t_arr.ptr if info else None, i_arr.ptr if info else None, stream, n_save,
                                              times.ctypes.data_as(C.POINTER(C.c_double)), saved.ptr if n_save else None))
    if not info:
        return saved
    _lib.check(L.cloudy_stream_synchronize(stream))
    counts = i_arr.to_numpy()[:, :n]
    accepted, rejected, status = counts[0].copy(), counts[1].copy(), counts[2].copy()
    bad = np.flatnonzero(status)
    if bad.size:
        raise RuntimeError(f"solve_tsit5_adaptive_saveat: {bad.size} of {n} parcels did not reach t_span; the first is parcel "
                           f"{int(bad[0])} (status {int(status[bad[0]])}: {ADAPTIVE_STATUS[int(status[bad[0]])]})")
    return saved, accepted, rejected, status, t_arr.to_numpy()[0]


def solve_box_ssprk33(par, u, dt, n_steps, xi, s, coal=True, cond=True, out=None, stream=None, coal_type=None):
    """solve(ODEProblem(rhs!, u, tspan, par), SSPRK33(), dt = dt) for n_steps fixed steps on the device, with rhs! the sum of
    the selected sources: rhs_coal! (`coal`) and rhs_condensation!(dm, m, par, s) (`cond`; condensation_single_gamma.jl:24-28,
    condensation_exp_gamma.jl:23-31) -- one launch, state in registers, one closure inversion per stage for both sources
    (cloudy_box_ssprk33_steps).  `xi` = p.xi; `s`: the supersaturation, a float or an (1, n) fp64 device array (one value per
    parcel), as rhs_condensation takes it.  `u` is advanced in place unless `out` is given.  `coal_type`: as solve_ssprk33; a
    NumericalCoalStyle plan serves cond alone."""
    if coal_type is not None and not isinstance(coal_type, (AnalyticalCoalStyle, NumericalCoalStyle)):
        raise ValueError("Invalid coal style!")
    sources = (_lib.SRC_COAL if coal else 0) | (_lib.SRC_COND if cond else 0)
    plan = _numerical_plan_for(par, dtype_code(u)) if isinstance(coal_type, NumericalCoalStyle) else _plan_for(par, dtype_code(u))
    uptr, planes, n, ld = as_device(u)
    o = out if out is not None else u
    optr, oplanes, on, old = as_device(o)
    if planes != plan.nmom or oplanes != plan.nmom or on != n or old != ld:
        raise ValueError(f"u and out must both be ({plan.nmom}, n) with equal leading dimension")
    if hasattr(s, "data_ptr") or isinstance(s, DeviceArray):
        sptr, splanes, sn, _ = as_device(s)
        if splanes != 1 or sn != n or dtype_code(s) != 0:   # (the kernel reads n doubles, whatever the plan's plane type)
            raise ValueError("s must be a float or an (1, n) fp64 device array")
        sval = 0.0
    else:
        sptr, sval = None, float(s)
    _lib.check(_lib.lib().cloudy_box_ssprk33_steps(plan.handle, n, ld, uptr, optr, sources, sptr, sval, float(xi), float(dt),
                                                  int(n_steps), stream))
    return o


def solve_box_tsit5_adaptive(par, u, t_span, xi, s, coal=True, cond=True, saveat=None, reltol=1e-6, abstol=1e-9, dt=None,
                             max_steps=10000, out=None, dt_dev=None, info=False, stream=None, coal_type=None):
    """Every parcel of `u` from t = 0 to t = t_span with adaptive Tsit5 under a step-size controller of its own, the right-hand
    side the sum of the selected sources (cloudy_box_tsit5_adaptive): rhs_coal! (`coal`) and rhs_condensation!(dm, m, par, s)
    (`cond`) -- the error-controlled counterpart of solve_box_ssprk33.  `xi` and `s` as solve_box_ssprk33 takes them (`s`: a float
    or an (1, n) fp64 device array, one supersaturation per parcel); the controller, `reltol`, `abstol`, `dt`, `max_steps`,
    `dt_dev`, `out` and `info` as solve_tsit5_adaptive.  `saveat` (None: no snapshots): host times as solve_tsit5_adaptive_saveat
    takes them; the snapshots come back as it returns them.  Returns what solve_tsit5_adaptive returns -- the state, or with
    info=True (accepted, rejected, status, t_reached) -- and with `saveat` what solve_tsit5_adaptive_saveat returns: the snapshots,
    or (snapshots, accepted, rejected, status, t_reached).  With info=True a parcel that did not reach t_span raises the
    RuntimeError of solve_tsit5_adaptive, after the call.  `coal_type`: as solve_ssprk33; a NumericalCoalStyle plan serves cond
    alone."""
    import ctypes as C

    if coal_type is not None and not isinstance(coal_type, (AnalyticalCoalStyle, NumericalCoalStyle)):
        raise ValueError("Invalid coal style!")
    sources = (_lib.SRC_COAL if coal else 0) | (_lib.SRC_COND if cond else 0)
    plan = _numerical_plan_for(par, dtype_code(u)) if isinstance(coal_type, NumericalCoalStyle) else _plan_for(par, dtype_code(u))
    uptr, planes, n, ld = as_device(u)
    o = out if out is not None else u
    optr, oplanes, on, old = as_device(o)
    if planes != plan.nmom or oplanes != plan.nmom or on != n or old != ld:
        raise ValueError(f"u and out must both be ({plan.nmom}, n) with equal leading dimension")
    if hasattr(s, "data_ptr") or isinstance(s, DeviceArray):
        sptr, splanes, sn, _ = as_device(s)
        if splanes != 1 or sn != n or dtype_code(s) != 0:   # (the kernel reads n doubles, whatever the plan's plane type)
            raise ValueError("s must be a float or an (1, n) fp64 device array")
        sval = 0.0
    else:
        sptr, sval = None, float(s)
    dptr = None
    if dt_dev is not None:
        dptr, dplanes, dn, _ = as_device(dt_dev)
        if dplanes != 1 or dn != n or dtype_code(dt_dev) != 0:
            raise ValueError("dt_dev must be an (1, n) fp64 device array")
    n_save, times, saved = 0, None, None
    if saveat is not None:
        times = np.ascontiguousarray(np.atleast_1d(np.asarray(saveat, dtype=np.float64)))
        if times.ndim != 1:
            raise ValueError("saveat must be a sequence of times")
        n_save = int(times.size)
        saved = DeviceArray(n_save * planes, ld, dtype=np.float32 if dtype_code(u) else np.float64)
    L = _lib.lib()
    opts = _lib.AdaptiveOptsC()
    L.cloudy_adaptive_opts_init(C.byref(opts))
    opts.reltol, opts.abstol, opts.dt_init, opts.max_steps = float(reltol), float(abstol), 0.0 if dt is None else float(dt), int(max_steps)
    t_arr = DeviceArray.zeros(1, n) if info else None
    i_arr = DeviceArray.zeros(3, ld, dtype=np.int32) if info else None
    _lib.check(L.cloudy_box_tsit5_adaptive(plan.handle, n, ld, uptr, optr, sources, sptr, sval, float(xi), float(t_span), C.byref(opts),
                                           dptr, t_arr.ptr if info else None, i_arr.ptr if info else None, stream, n_save,
                                           times.ctypes.data_as(C.POINTER(C.c_double)) if n_save else None,
                                           saved.ptr if n_save else None))
    if not info:
        return o if saveat is None else saved
    _lib.check(L.cloudy_stream_synchronize(stream))
    counts = i_arr.to_numpy()[:, :n]
    accepted, rejected, status = counts[0].copy(), counts[1].copy(), counts[2].copy()
    bad = np.flatnonzero(status)
    if bad.size:
        raise RuntimeError(f"solve_box_tsit5_adaptive: {bad.size} of {n} parcels did not reach t_span; the first is parcel "
                           f"{int(bad[0])} (status {int(status[bad[0]])}: {ADAPTIVE_STATUS[int(status[bad[0]])]})")
    res = (accepted, rejected, status, t_arr.to_numpy()[0])
    return res if saveat is None else (saved,) + res
