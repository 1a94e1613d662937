"""What the solve_* wrappers of box_model.py, Sedimentation.py and parcel.py share above the C calls: the checks of their device
arrays, and for the adaptive Tsit5 family the controller's arguments, the save times and the reading of the info planes.
decode_info and save_times take plain numpy inputs (no device)."""
import ctypes as C

import numpy as np

from . import _lib
from .device import DeviceArray, as_device, dtype_code

ADAPTIVE_STATUS = ("reached t_span", "max_steps attempts", "dt below 1e-14 t_span or not finite")


def state_pair(u, out, planes, names="u and out"):
    """-> (o, uptr, optr, n, ld): `o` is `out`, or `u` where none is given; both must be (planes, n) with one leading dimension"""
    uptr, uplanes, n, ld = as_device(u)
    o = out if out is not None else u
    optr, oplanes, on, old = as_device(o)
    if uplanes != planes or oplanes != planes or on != n or old != ld:
        raise ValueError(f"{names} must both be ({planes}, n) with equal leading dimension")
    return o, uptr, optr, n, ld


def scalar_or_plane(v, n, name, tail=""):
    """-> (pointer or None, scalar): `v` a float, or an (1, n) fp64 device array with one value per parcel (cell)"""
    if hasattr(v, "data_ptr") or isinstance(v, DeviceArray):
        ptr, planes, vn, _ = as_device(v)
        if planes != 1 or vn != n or dtype_code(v) != 0:   # (the kernels read n doubles, whatever the plan's plane type)
            raise ValueError(f"{name} must be a float or an (1, n) fp64 device array{tail}")
        return ptr, 0.0
    return None, float(v)


def save_times(times, name):
    """-> the save times as a C-contiguous 1-D float64 array (a scalar: one time); `name`: the caller's argument"""
    ts = np.ascontiguousarray(np.atleast_1d(np.asarray(times, dtype=np.float64)))
    if ts.ndim != 1:
        raise ValueError(f"{name} must be a sequence of times")
    return ts


def snapshot_planes(u, n_save, planes, ld):
    """an uninitialised (n_save * planes, ld) DeviceArray in the plane type of `u`"""
    return DeviceArray(n_save * planes, ld, dtype=np.float32 if dtype_code(u) else np.float64)


def save_args(ts, saved_ptr):
    """-> the (n_save, t_save, u_save_dev) tail of a C call; nothing to save: no pointers"""
    n_save = int(ts.size)
    return (n_save, ts.ctypes.data_as(C.POINTER(C.c_double)), saved_ptr) if n_save else (0, None, None)


def decode_info(fn, counts, what="parcel"):
    """counts: the (3, m) rows accepted / rejected / status of a call -> copies of the three; raises if any status is not 0"""
    accepted, rejected, status = (np.array(row) for row in counts)
    bad = np.flatnonzero(status)
    if bad.size:
        raise RuntimeError(f"{fn}: {bad.size} of {status.size} {what}s did not reach t_span; the first is {what} {int(bad[0])} "
                           f"(status {int(status[bad[0]])}: {ADAPTIVE_STATUS[int(status[bad[0]])]})")
    return accepted, rejected, status


class Controller:
    """The controller's side of one adaptive call on m parcels (columns): `args`, the (opts, dt_dev, t_dev, info_dev) of the C call
    -- t_dev and info_dev (info_ld columns) allocated only with `info` -- and afterwards `result`."""

    def __init__(self, reltol, abstol, dt, max_steps, dt_dev, info, m, info_ld, what="parcel"):
        self.m, self.what = m, what
        dptr = None
        if dt_dev is not None:
            dptr, dplanes, dn, _ = as_device(dt_dev)
            if dplanes != 1 or dn != m or dtype_code(dt_dev) != 0:
                raise ValueError(f"dt_dev must be an (1, {'n' if what == 'parcel' else 'n_columns'}) fp64 device array")
        self.opts = _lib.AdaptiveOptsC()
        _lib.lib().cloudy_adaptive_opts_init(C.byref(self.opts))
        o = self.opts
        o.reltol, o.abstol, o.dt_init, o.max_steps = float(reltol), float(abstol), 0.0 if dt is None else float(dt), int(max_steps)
        self.t_arr = DeviceArray.zeros(1, max(m, 1)) if info else None
        self.i_arr = DeviceArray.zeros(3, info_ld, dtype=np.int32) if info else None
        self.args = (C.byref(o), dptr, self.t_arr.ptr if info else None, self.i_arr.ptr if info else None)

    def result(self, fn, stream):
        """(info=True) -> (accepted, rejected, status, t_reached) as numpy arrays; synchronises, raises as decode_info does"""
        _lib.check(_lib.lib().cloudy_stream_synchronize(stream))
        return decode_info(fn, self.i_arr.to_numpy()[:, :self.m], self.what) + (self.t_arr.to_numpy()[0, :self.m],)
