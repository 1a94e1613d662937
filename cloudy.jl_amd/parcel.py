"""The adiabatic parcel of test/examples/Analytical/parcel_example.jl on the device: Y = (S, p, T, q_v, moments...) with the
saturation ratio, pressure, temperature and vapour content prognostic beside the moments and coupled to them through
get_cond_evap (cloudy_parcel_rhs, cloudy_parcel_ssprk33_steps, cloudy_parcel_tsit5_adaptive; the equations are in
include/cloudy_hip.h).

`y`, `dy` are (4 + nmom, n_parcels) fp64 device arrays: planes 0..3 are S, p, T, q_v, plane 4 + q is moment plane q in physical
units.  `par` carries what rhs_coal! reads (ODEParameters), or is a Plan."""
import ctypes as C
from dataclasses import dataclass, fields

import numpy as np

from . import _lib
from .device import DeviceArray, as_device, dtype_code

_R = 8.3144598


@dataclass
class ParcelParams:
    """cloudy_parcel_params with the defaults of cloudy_parcel_params_init (ClimaParams' values as recalled)."""
    R_d: float = _R / 0.02897
    R_v: float = _R / 0.018015
    cp_d: float = _R / 0.02897 * 7 / 2
    cp_v: float = 1859.0
    cp_l: float = 4181.0
    LH_v0: float = 2.5008e6
    T_0: float = 273.16
    press_triple: float = 611.657
    T_triple: float = 273.16
    grav: float = 9.81
    K_therm: float = 2.4e-2
    D_vapor: float = 2.26e-5
    rho_l: float = 1000.0

    def to_c(self):
        c = _lib.ParcelParamsC()
        c.struct_size = C.sizeof(_lib.ParcelParamsC)
        for f in fields(self):
            setattr(c, f.name, float(getattr(self, f.name)))
        return c


def _plan(par, y):
    if hasattr(par, "handle"):
        return par
    from .box_model import _numerical_plan_for, _plan_for

    return _numerical_plan_for(par, dtype_code(y)) if getattr(par, "coal_data", None) is None else _plan_for(par, dtype_code(y))


def _updraft(w, n):
    """w: a float, or an (1, n) fp64 device array (one value per parcel) -- validated as solve_box_ssprk33 validates s"""
    if hasattr(w, "data_ptr") or isinstance(w, DeviceArray):
        wptr, wplanes, wn, _ = as_device(w)
        if wplanes != 1 or wn != n or dtype_code(w) != 0:
            raise ValueError("w must be a float or an (1, n) fp64 device array")
        return wptr, 0.0
    return None, float(w)


def _sources(coal):
    return _lib.SRC_COND | (_lib.SRC_COAL if coal else 0)


def parcel_rhs(par, dy, y, w, params=None, coal=False, stream=None):
    """parcel_model_cloudy(dY, Y, p, t) (parcel_example.jl:15-85) for a batch, with the distributions updated from the current
    moments; `coal`: rhs_coal! added to the moments' tendency.  One launch."""
    plan = _plan(par, y)
    yptr, planes, n, ld = as_device(y)
    dptr, dplanes, dn, dld = as_device(dy)
    if planes != 4 + plan.nmom or dplanes != planes or dn != n or dld != ld:
        raise ValueError(f"y and dy must both be ({4 + plan.nmom}, n) with equal leading dimension")
    wptr, wval = _updraft(w, n)
    c = (params if params is not None else ParcelParams()).to_c()
    _lib.check(_lib.lib().cloudy_parcel_rhs(plan.handle, n, ld, yptr, wptr, wval, C.byref(c), _sources(coal), dptr, stream))
    return dy


def solve_parcel_ssprk33(par, y, w, dt, n_steps, params=None, coal=False, out=None, stream=None):
    """solve(ODEProblem(parcel_model_cloudy, Yinit, tspan, p), SSPRK33(), dt = dt) for n_steps fixed steps on the device
    (parcel_example.jl:104-111): the final state only, one launch, state in registers.  `y` is advanced in place unless `out`
    is given."""
    plan = _plan(par, y)
    yptr, planes, n, ld = as_device(y)
    o = out if out is not None else y
    optr, oplanes, on, old = as_device(o)
    if planes != 4 + plan.nmom or oplanes != planes or on != n or old != ld:
        raise ValueError(f"y and out must both be ({4 + plan.nmom}, n) with equal leading dimension")
    wptr, wval = _updraft(w, n)
    c = (params if params is not None else ParcelParams()).to_c()
    _lib.check(_lib.lib().cloudy_parcel_ssprk33_steps(plan.handle, n, ld, yptr, optr, _sources(coal), wptr, wval, C.byref(c),
                                                     float(dt), int(n_steps), stream))
    return o


def solve_parcel_tsit5_adaptive(par, y, w, t_span, params=None, coal=False, reltol=1e-6, abstol=1e-9, dt=None, max_steps=10000,
                                times=(), out=None, dt_dev=None, info=False, stream=None):
    """Every parcel of `y` from t = 0 to t = t_span with adaptive Tsit5 under a step-size controller of its own
    (cloudy_parcel_tsit5_adaptive): the error-controlled counterpart of solve_parcel_ssprk33, `w`, `params` and `coal` as it takes
    them; the controller, `reltol`, `abstol`, `dt`, `max_steps`, `dt_dev`, `out` and `info` as solve_box_tsit5_adaptive.  abstol
    applies to S, p, T, q_v in their own units and to the moments in the plan's normalised units.  `times` (empty: no snapshots):
    host times within [0, t_span], strictly increasing; the state at them comes back as a (len(times) * (4 + nmom), n) device
    array, snapshot j in planes j (4 + nmom) ...  Returns what solve_box_tsit5_adaptive returns: the state -- with `times` the
    snapshots --, or with info=True (accepted, rejected, status, t_reached), preceded by the snapshots with `times`.  With
    info=True a parcel that did not reach t_span raises RuntimeError, after the call."""
    from .box_model import ADAPTIVE_STATUS

    plan = _plan(par, y)
    yptr, planes, n, ld = as_device(y)
    o = out if out is not None else y
    optr, oplanes, on, old = as_device(o)
    if planes != 4 + plan.nmom or oplanes != planes or on != n or old != ld:
        raise ValueError(f"y and out must both be ({4 + plan.nmom}, n) with equal leading dimension")
    wptr, wval = _updraft(w, n)
    c = (params if params is not None else ParcelParams()).to_c()
    dptr = None
    if dt_dev is not None:
        dptr, dplanes, dn, _ = as_device(dt_dev)
        if dplanes != 1 or dn != n or dtype_code(dt_dev) != 0:
            raise ValueError("dt_dev must be an (1, n) fp64 device array")
    ts = np.ascontiguousarray(np.atleast_1d(np.asarray(times, dtype=np.float64)))
    if ts.ndim != 1:
        raise ValueError("times must be a sequence of times")
    n_save = int(ts.size)
    saved = DeviceArray(n_save * planes, ld) if n_save else None
    L = _lib.lib()
    opts = _lib.AdaptiveOptsC()
    L.cloudy_adaptive_opts_init(C.byref(opts))
    opts.reltol, opts.abstol, opts.dt_init, opts.max_steps = float(reltol), float(abstol), 0.0 if dt is None else float(dt), int(max_steps)
    t_arr = DeviceArray.zeros(1, n) if info else None
    i_arr = DeviceArray.zeros(3, ld, dtype=np.int32) if info else None
    _lib.check(L.cloudy_parcel_tsit5_adaptive(plan.handle, n, ld, yptr, optr, _sources(coal), wptr, wval, C.byref(c), float(t_span),
                                              C.byref(opts), dptr, t_arr.ptr if info else None, i_arr.ptr if info else None, stream,
                                              n_save, ts.ctypes.data_as(C.POINTER(C.c_double)) if n_save else None,
                                              saved.ptr if n_save else None))
    if not info:
        return saved if n_save else o
    _lib.check(L.cloudy_stream_synchronize(stream))
    counts = i_arr.to_numpy()[:, :n]
    accepted, rejected, status = counts[0].copy(), counts[1].copy(), counts[2].copy()
    bad = np.flatnonzero(status)
    if bad.size:
        raise RuntimeError(f"solve_parcel_tsit5_adaptive: {bad.size} of {n} parcels did not reach t_span; the first is parcel "
                           f"{int(bad[0])} (status {int(status[bad[0]])}: {ADAPTIVE_STATUS[int(status[bad[0]])]})")
    res = (accepted, rejected, status, t_arr.to_numpy()[0])
    return (saved,) + res if n_save else res
