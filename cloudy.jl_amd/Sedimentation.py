"""Batched sedimentation flux (src/Sources/Sedimentation.jl:22-37) and the rainshaft per-cell sources
(test/examples/utils/rainshaft_helpers.jl:52-78, without the inter-cell flux divergence)."""
from . import _lib
from ._adaptive import Controller, save_args, save_times, scalar_or_plane, snapshot_planes, state_pair
from .device import DeviceArray, as_device, plane_dtype


def get_sedimentation_flux(plan, mom, out=None, stream=None):
    """mom (nmom, n) device, physical units -> flux (nmom, n) device, physical units."""
    ptr, planes, n, ld = as_device(mom)
    o = out if out is not None else DeviceArray(plan.nmom, n, plane_dtype(plan))
    _lib.check(_lib.lib().cloudy_sedimentation_flux(plan.handle, n, ld, ptr, as_device(o)[0], stream))
    return o


def rainshaft_sources(plan, mom, coal_source=None, sedi_flux=None, stream=None):
    ptr, planes, n, ld = as_device(mom)
    dt = plane_dtype(plan)
    cs = coal_source if coal_source is not None else DeviceArray(plan.nmom, n, dt)
    sf = sedi_flux if sedi_flux is not None else DeviceArray(plan.nmom, n, dt)
    _lib.check(_lib.lib().cloudy_rainshaft_sources(plan.handle, n, ld, ptr, as_device(cs)[0], as_device(sf)[0], stream))
    return cs, sf


def rhs_condensation(plan, dmom, mom, xi, s, stream=None):
    """rhs_condensation!(dmom, mom, p, s) (box_model_helpers.jl:55-67) -> get_cond_evap (Condensation.jl:22-37),
    batched.  `s`: scalar supersaturation or an (1, n) fp64 device array (one value per parcel); xi = p.xi."""
    ptr, planes, n, ld = as_device(mom)
    optr = as_device(dmom)[0]
    if hasattr(s, "data_ptr") or isinstance(s, DeviceArray):
        sptr, sval = as_device(s)[0], 0.0
    else:
        sptr, sval = None, float(s)
    _lib.check(_lib.lib().cloudy_cond_evap(plan.handle, n, ld, ptr, sptr, sval, float(xi), optr, stream))
    return dmom


def make_rainshaft_rhs(coal_type=None):
    """make_rainshaft_rhs(coal_type) (rainshaft_helpers.jl:45-89): returns rhs(m, p, t) -> d(m)/dt for a column
    (or a batch of columns stacked along the cell axis, `p.nz` cells each) -- coalescence source plus the upwind
    divergence of the sedimentation flux.  `m` is an (nmom, nz * n_columns) device array; `p` carries coal_data,
    pdists, NProgMoms, norms, vel and dz."""
    from .box_model import _plan_for
    from .device import dtype_code

    def rhs(m, p, t, out=None, work=None):
        plan = _plan_for(p, dtype_code(m))
        ptr, planes, n, ld = as_device(m)
        nz = int(getattr(p, "nz", n))
        if n % nz:
            raise ValueError("number of cells must be a multiple of p.nz")
        dt = plane_dtype(plan)
        o = out if out is not None else DeviceArray(plan.nmom, n, dt)
        w = work if work is not None else DeviceArray(plan.nmom, n, dt)
        _lib.check(_lib.lib().cloudy_rainshaft_rhs(plan.handle, nz, n // nz, ld, ptr, float(p.dz), as_device(w)[0],
                                                  as_device(o)[0], None))
        return o

    return rhs


def solve_rainshaft_ssprk33(par, u, n_steps, out=None, stream=None):
    """`solve(ODEProblem(make_rainshaft_rhs(...), m, tspan, p), SSPRK33(), dt = p.dt)` of the rainshaft drivers
    (rainshaft_gamma_mixture.jl:59-60), final state only, for a batch of independent columns of `par.nz` cells (fused in one launch up to 1024 cells -- workgroups of 256, 512 or
    1024 threads holding whole columns, picked by `nz` in the plan-time compiled kernel; taller columns stage by stage inside
    the library):
    one launch, state in registers, flux exchange through LDS (cloudy_rainshaft_ssprk33_steps).  `u` is advanced in
    place unless `out` is given."""
    from .box_model import _plan_for
    from .device import dtype_code

    plan = _plan_for(par, dtype_code(u))
    ptr, planes, n, ld = as_device(u)
    nz = int(getattr(par, "nz", n))
    if n % nz:
        raise ValueError("number of cells must be a multiple of par.nz")
    optr = as_device(out)[0] if out is not None else ptr
    _lib.check(_lib.lib().cloudy_rainshaft_ssprk33_steps(plan.handle, nz, n // nz, ld, ptr, optr, float(par.dz),
                                                         float(par.dt), int(n_steps), stream))
    return out if out is not None else u


_PER_CELL = " with one value per cell"   # (the supersaturation of a column call: scalar_or_plane(s, n, "s", _PER_CELL))


def make_rainshaft_cond_rhs(coal_type=None):
    """make_rainshaft_rhs(coal_type) with the third source of a column: returns rhs(m, p, t, xi, s) -> d(m)/dt, the
    coalescence source plus the upwind divergence of the sedimentation flux plus get_cond_evap of every cell
    (Condensation.jl:22-37) at the cell's supersaturation `s` (a float, or an (1, n) fp64 device array in the cell order of
    `m`); `xi` = p.xi.  One launch for columns of up to 1024 cells (cloudy_rainshaft_cond_rhs)."""
    from .box_model import _plan_for
    from .device import dtype_code

    def rhs(m, p, t, xi, s, out=None, work=None):
        plan = _plan_for(p, dtype_code(m))
        ptr, planes, n, ld = as_device(m)
        nz = int(getattr(p, "nz", n))
        if n % nz:
            raise ValueError("number of cells must be a multiple of p.nz")
        dt = plane_dtype(plan)
        o = out if out is not None else DeviceArray(plan.nmom, n, dt)
        w = work if work is not None else DeviceArray(plan.nmom, n, dt)
        sptr, sval = scalar_or_plane(s, n, "s", _PER_CELL)
        _lib.check(_lib.lib().cloudy_rainshaft_cond_rhs(plan.handle, nz, n // nz, ld, ptr, sptr, sval, float(xi), float(p.dz),
                                                       as_device(w)[0], as_device(o)[0], None))
        return o

    return rhs


def solve_rainshaft_cond_ssprk33(par, u, n_steps, xi, s, out=None, stream=None):
    """solve_rainshaft_ssprk33 for columns through air with a supersaturation profile: SSPRK33 steps of coalescence +
    sedimentation + condensation / evaporation, one closure inversion per stage for the three sources, one launch for columns
    of up to 1024 cells (cloudy_rainshaft_cond_ssprk33_steps; stage by stage inside the library otherwise).  `xi` = p.xi;
    `s`: the supersaturation, a float or an (1, n) fp64 device array with one value per cell in the cell order of `u`,
    constant over the call.  `u` is advanced in place unless `out` is given."""
    from .box_model import _plan_for
    from .device import dtype_code

    plan = _plan_for(par, dtype_code(u))
    ptr, planes, n, ld = as_device(u)
    nz = int(getattr(par, "nz", n))
    if n % nz:
        raise ValueError("number of cells must be a multiple of par.nz")
    optr = as_device(out)[0] if out is not None else ptr
    sptr, sval = scalar_or_plane(s, n, "s", _PER_CELL)
    _lib.check(_lib.lib().cloudy_rainshaft_cond_ssprk33_steps(plan.handle, nz, n // nz, ld, ptr, optr, sptr, sval, float(xi),
                                                              float(par.dz), float(par.dt), int(n_steps), stream))
    return out if out is not None else u


def _adaptive_columns(par, u, out, s, controller):
    """what the two adaptive column wrappers take alike -> (plan, o, n, ld, the C call's arguments up to s, the Controller of
    `controller` = (reltol, abstol, dt, max_steps, dt_dev, info) with one entry per column)"""
    from .box_model import _plan_for
    from .device import dtype_code

    plan = _plan_for(par, dtype_code(u))
    n = as_device(u)[2]
    nz = int(getattr(par, "nz", n))
    if n % nz:
        raise ValueError("number of cells must be a multiple of par.nz")
    ncol = n // nz
    o, uptr, optr, n, ld = state_pair(u, out, plan.nmom)
    sources = _lib.SRC_COAL | (0 if s is None else _lib.SRC_COND)
    sptr, sval = (None, 0.0) if s is None else scalar_or_plane(s, n, "s", _PER_CELL)
    ctl = Controller(*controller, ncol, max(ncol, 1), what="column")
    return plan, o, n, ld, (plan.handle, nz, ncol, ld, uptr, optr, sources, sptr, sval), ctl


def solve_rainshaft_tsit5_adaptive(par, u, t_span, xi=0.0, s=None, reltol=1e-6, abstol=1e-9, dt=None, max_steps=10000, out=None,
                                   dt_dev=None, info=False, stream=None):
    """Every column of `u` (`par.nz` cells each, stacked along the cell axis) from t = 0 to t = t_span with adaptive Tsit5 under
    a step-size controller per COLUMN (cloudy_rainshaft_tsit5_adaptive) -- the error-controlled counterpart of
    solve_rainshaft_ssprk33 / solve_rainshaft_cond_ssprk33.  `s` None: coalescence + sedimentation; otherwise the condensation
    source as well, `xi` and `s` as solve_rainshaft_cond_ssprk33 takes them (`s`: a float or an (1, n) fp64 device array, one
    supersaturation per cell).  `reltol`, `abstol`, `dt`, `max_steps` and `out` as solve_tsit5_adaptive; `dt_dev`: an
    (1, n_columns) fp64 device array, the proposed step of every column (in/out).  Returns the state -- `u` advanced in place
    unless `out` is given -- or with info=True (accepted, rejected, status, t_reached), one entry per column; then a column that
    did not reach t_span raises a RuntimeError, after the call."""
    plan, o, n, ld, head, ctl = _adaptive_columns(par, u, out, s, (reltol, abstol, dt, max_steps, dt_dev, info))
    _lib.check(_lib.lib().cloudy_rainshaft_tsit5_adaptive(*head, float(xi), float(par.dz), float(t_span), *ctl.args, stream))
    return ctl.result("solve_rainshaft_tsit5_adaptive", stream) if info else o


def solve_rainshaft_tsit5_adaptive_saveat(par, u, t_span, t_save, xi=0.0, s=None, reltol=1e-6, abstol=1e-9, dt=None, max_steps=10000,
                                          out=None, save_out=None, dt_dev=None, info=False, stream=None):
    """solve_rainshaft_tsit5_adaptive with dense output (cloudy_rainshaft_tsit5_adaptive_saveat): the same integration -- every column
    takes the steps solve_rainshaft_tsit5_adaptive takes, bit for bit, and none is clamped to a save time -- and the state of every
    cell at the batch-wide times `t_save` (host floats in [0, t_span], strictly increasing), from the free 4th-order interpolant of
    Tsit5 inside the accepted step that holds the time, clamped to >= 0 as the returned state is.  Returns (state, saved): the state
    as solve_rainshaft_tsit5_adaptive returns it, and the snapshots as a DeviceArray of n_save * planes rows of the leading dimension
    and plane type of `u` (`save_out`, where given, must be one): snapshot j, plane p is row j * planes + p; a snapshot at 0 equals
    the input and one at t_span the final state bit for bit; a column that stopped early has NaN in the snapshots it did not reach.
    With info=True returns (state, saved, accepted, rejected, status, t_reached), one entry per column, and raises as
    solve_rainshaft_tsit5_adaptive does -- keep the snapshots of a run that may stop early with info=False.  Everything else as
    solve_rainshaft_tsit5_adaptive."""
    from .device import dtype_code

    plan, o, n, ld, head, ctl = _adaptive_columns(par, u, out, s, (reltol, abstol, dt, max_steps, dt_dev, info))
    times = save_times(t_save, "t_save")
    rows = times.size * plan.nmom
    if save_out is None:
        saved = snapshot_planes(u, times.size, plan.nmom, ld)
    else:
        saved = save_out
        vptr, vplanes, vn, vld = as_device(saved)
        if vplanes != rows or vn != n or vld != ld or dtype_code(saved) != dtype_code(u):
            raise ValueError(f"save_out must be ({rows}, n) with the leading dimension and plane type of u")
    _lib.check(_lib.lib().cloudy_rainshaft_tsit5_adaptive_saveat(*head, float(xi), float(par.dz), float(t_span), *ctl.args, stream,
                                                                *save_args(times, as_device(saved)[0])))
    return (o, saved) + ctl.result("solve_rainshaft_tsit5_adaptive_saveat", stream) if info else (o, saved)
