"""The adiabatic parcel of test/examples/Analytical/parcel_example.jl on the device: Y = (S, p, T, q_v, moments...) with the
saturation ratio, pressure, temperature and vapour content prognostic beside the moments and coupled to them through
get_cond_evap (cloudy_parcel_rhs, cloudy_parcel_ssprk33_steps, cloudy_parcel_tsit5_adaptive; the equations are in
include/cloudy_hip.h).

`y`, `dy` are (4 + nmom, n_parcels) fp64 device arrays: planes 0..3 are S, p, T, q_v, plane 4 + q is moment plane q in physical
units.  `par` carries what rhs_coal! reads (ODEParameters), or is a Plan."""
import ctypes as C
from dataclasses import dataclass, fields

from . import _lib
from ._adaptive import Controller, save_args, save_times, scalar_or_plane, state_pair
from .device import DeviceArray, dtype_code

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


def _sources(coal):
    return _lib.SRC_COND | (_lib.SRC_COAL if coal else 0)


def _parcel_call(par, y, out, w, params, names="y and out"):
    """what the three entry points take alike -> (plan, o, yptr, optr, n, ld, wptr, wval, the cloudy_parcel_params); `w`: a float,
    or an (1, n) fp64 device array (one value per parcel)"""
    plan = _plan(par, y)
    o, yptr, optr, n, ld = state_pair(y, out, 4 + plan.nmom, names)
    wptr, wval = scalar_or_plane(w, n, "w")
    return plan, o, yptr, optr, n, ld, wptr, wval, (params if params is not None else ParcelParams()).to_c()


def parcel_rhs(par, dy, y, w, params=None, coal=False, stream=None):
    """parcel_model_cloudy(dY, Y, p, t) (parcel_example.jl:15-85) for a batch, with the distributions updated from the current
    moments; `coal`: rhs_coal! added to the moments' tendency.  One launch."""
    plan, dy, yptr, dptr, n, ld, wptr, wval, c = _parcel_call(par, y, dy, w, params, "y and dy")
    _lib.check(_lib.lib().cloudy_parcel_rhs(plan.handle, n, ld, yptr, wptr, wval, C.byref(c), _sources(coal), dptr, stream))
    return dy


def solve_parcel_ssprk33(par, y, w, dt, n_steps, params=None, coal=False, out=None, stream=None):
    """solve(ODEProblem(parcel_model_cloudy, Yinit, tspan, p), SSPRK33(), dt = dt) for n_steps fixed steps on the device
    (parcel_example.jl:104-111): the final state only, one launch, state in registers.  `y` is advanced in place unless `out`
    is given."""
    plan, o, yptr, optr, n, ld, wptr, wval, c = _parcel_call(par, y, out, w, params)
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
    plan, o, yptr, optr, n, ld, wptr, wval, c = _parcel_call(par, y, out, w, params)
    ctl = Controller(reltol, abstol, dt, max_steps, dt_dev, info, n, ld)
    ts = save_times(times, "times")
    saved = DeviceArray(ts.size * (4 + plan.nmom), ld) if ts.size else None
    _lib.check(_lib.lib().cloudy_parcel_tsit5_adaptive(plan.handle, n, ld, yptr, optr, _sources(coal), wptr, wval, C.byref(c),
                                                      float(t_span), *ctl.args, stream, *save_args(ts, saved.ptr if ts.size else None)))
    if not info:
        return saved if ts.size else o
    res = ctl.result("solve_parcel_tsit5_adaptive", stream)
    return (saved,) + res if ts.size else res
