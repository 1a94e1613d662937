"""The operator boundary: make_box_model_rhs (test/examples/utils/box_model_helpers.jl:22-53), batched.

    rhs = make_box_model_rhs(AnalyticalCoalStyle())          # same factory signature
    rhs(dm, m, par, t)                                        # same 4-argument in-place ODE function

`m`, `dm` are (nmom, n_parcels) device arrays (DeviceArray or CUDA torch tensors), i.e. Julia's m[parcel, moment].
`par` carries the fields rhs_coal! reads: pdists (types only), coal_data, NProgMoms, norms.
"""
from types import SimpleNamespace

import numpy as np

from . import _lib
from ._adaptive import Controller, save_args, save_times, scalar_or_plane, snapshot_planes, state_pair
from .device import as_device, dtype_code
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


def _solver_plan(par, u, coal_type):
    """the plan of a solve_* call: `coal_type` None or AnalyticalCoalStyle: the tensor plan of `par`, NumericalCoalStyle: its quadrature plan"""
    if coal_type is not None and not isinstance(coal_type, (AnalyticalCoalStyle, NumericalCoalStyle)):
        raise ValueError("Invalid coal style!")
    return _numerical_plan_for(par, dtype_code(u)) if isinstance(coal_type, NumericalCoalStyle) else _plan_for(par, dtype_code(u))


def solve_ssprk33(par, u, dt, n_steps, out=None, stream=None, coal_type=None):
    """solve(ODEProblem(rhs, u, tspan, par), SSPRK33(), dt = dt) for n_steps fixed steps, on the device
    (cloudy_ssprk33_steps): the final state only (the examples' `sol.u[end]`).  `u` is advanced in place unless
    `out` is given.  `coal_type`: the style the RHS was made with (make_box_model_rhs(coal_type)); default
    AnalyticalCoalStyle, NumericalCoalStyle() integrates get_coal_ints(::NumericalCoalStyle, p.pdists, p.kernel_func)."""
    plan = _solver_plan(par, u, coal_type)
    o, uptr, optr, n, ld = state_pair(u, out, plan.nmom)
    _lib.check(_lib.lib().cloudy_ssprk33_steps(plan.handle, n, ld, uptr, optr, float(dt), int(n_steps), stream))
    return o


def solve_tsit5(par, u, dt, n_steps, out=None, stream=None, coal_type=None):
    """solve(ODEProblem(rhs, u, tspan, par), Tsit5(), dt = dt, adaptive = false) for n_steps fixed steps, on the device
    (cloudy_tsit5_steps): BASELINE configs[0] names Tsit5; no reference driver uses it (they call SSPRK33).  Every plan
    solve_ssprk33 serves (thresholds Inf / fixed / moving, NumericalCoalStyle through `coal_type`), fp64 or float planes.
    `u` is advanced in place unless `out` is given."""
    plan = _solver_plan(par, u, coal_type)
    o, uptr, optr, n, ld = state_pair(u, out, plan.nmom)
    _lib.check(_lib.lib().cloudy_tsit5_steps(plan.handle, n, ld, uptr, optr, float(dt), int(n_steps), stream))
    return o


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
    plan = _solver_plan(par, u, coal_type)
    o, uptr, optr, n, ld = state_pair(u, out, plan.nmom)
    ctl = Controller(reltol, abstol, dt, max_steps, dt_dev, info, n, ld)
    _lib.check(_lib.lib().cloudy_tsit5_adaptive(plan.handle, n, ld, uptr, optr, float(t_span), *ctl.args, stream))
    return ctl.result("solve_tsit5_adaptive", stream) if info else o


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
    plan = _solver_plan(par, u, coal_type)
    o, uptr, optr, n, ld = state_pair(u, out, plan.nmom)
    ctl = Controller(reltol, abstol, dt, max_steps, dt_dev, info, n, ld)
    times = save_times(saveat, "saveat")
    saved = snapshot_planes(u, times.size, plan.nmom, ld)
    _lib.check(_lib.lib().cloudy_tsit5_adaptive_saveat(plan.handle, n, ld, uptr, optr, float(t_span), *ctl.args, stream,
                                                      *save_args(times, saved.ptr)))
    return (saved,) + ctl.result("solve_tsit5_adaptive_saveat", stream) if info else saved


def solve_box_ssprk33(par, u, dt, n_steps, xi, s, coal=True, cond=True, out=None, stream=None, coal_type=None):
    """solve(ODEProblem(rhs!, u, tspan, par), SSPRK33(), dt = dt) for n_steps fixed steps on the device, with rhs! the sum of
    the selected sources: rhs_coal! (`coal`) and rhs_condensation!(dm, m, par, s) (`cond`; condensation_single_gamma.jl:24-28,
    condensation_exp_gamma.jl:23-31) -- one launch, state in registers, one closure inversion per stage for both sources
    (cloudy_box_ssprk33_steps).  `xi` = p.xi; `s`: the supersaturation, a float or an (1, n) fp64 device array (one value per
    parcel), as rhs_condensation takes it.  `u` is advanced in place unless `out` is given.  `coal_type`: as solve_ssprk33; a
    NumericalCoalStyle plan serves cond alone."""
    plan = _solver_plan(par, u, coal_type)
    sources = (_lib.SRC_COAL if coal else 0) | (_lib.SRC_COND if cond else 0)
    o, uptr, optr, n, ld = state_pair(u, out, plan.nmom)
    sptr, sval = scalar_or_plane(s, n, "s")
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
    plan = _solver_plan(par, u, coal_type)
    sources = (_lib.SRC_COAL if coal else 0) | (_lib.SRC_COND if cond else 0)
    o, uptr, optr, n, ld = state_pair(u, out, plan.nmom)
    sptr, sval = scalar_or_plane(s, n, "s")
    ctl = Controller(reltol, abstol, dt, max_steps, dt_dev, info, n, ld)
    times = save_times(() if saveat is None else saveat, "saveat")
    saved = None if saveat is None else snapshot_planes(u, times.size, plan.nmom, ld)
    _lib.check(_lib.lib().cloudy_box_tsit5_adaptive(plan.handle, n, ld, uptr, optr, sources, sptr, sval, float(xi), float(t_span),
                                                   *ctl.args, stream, *save_args(times, saved.ptr if times.size else None)))
    if not info:
        return o if saveat is None else saved
    res = ctl.result("solve_box_tsit5_adaptive", stream)
    return res if saveat is None else (saved,) + res
