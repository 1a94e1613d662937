"""What every test of the adaptive Tsit5 family shares, once: the tableau, the interpolant and the controller constants as the
kernels hold them (csrc/adaptive.hpp), ONE NumPy restatement of the loop (`adaptive_tsit5`: parcels or columns, with or without
the clamp, with or without snapshots -- the device has one tsit5_adaptive_loop, and so has its reference), the small helpers of
the batches, and the refusals of cloudy_adaptive_opts that every entry point of the family answers in the same words.

The GPU tests run the restatement on the oracle's right-hand sides as the device's reference; the host tests check the
restatement itself (closed forms, order conditions, sensitivity to the last bit of the right-hand side)."""
import ctypes as C
import os

import numpy as np

import bench
from test_host_abi import ROOT, _c_prototypes, _julia_ccalls

EPS = float(np.finfo(np.float64).eps)

# ---- the tableau and the controller, restated (Tsitouras 2011; the PI controller of include/cloudy_hip.h)
C_NODES = (0.0, 0.161, 0.327, 0.9, 0.9800255409045097, 1.0, 1.0)
A_ROWS = ((0.161,),
          (-0.008480655492356989, 0.335480655492357),
          (2.8971530571054935, -6.359448489975075, 4.3622954328695815),
          (5.325864828439257, -11.748883564062828, 7.4955393428898365, -0.09249506636175525),
          (5.86145544294642, -12.92096931784711, 8.159367898576159, -0.071584973281401, -0.028269050394068383),
          (0.09646076681806523, 0.01, 0.4798896504144996, 1.379008574103742, -3.290069515436081, 2.324710524099774))
BTILDE = (-0.00178001105222577714, -0.0008164344596567469, 0.007880878010261995, -0.1447110071732629, 0.5823571654525552,
          -0.45808210592918697, 0.015151515151515152)
BETA1, BETA2, GAMMA, QMIN, QMAX, QOLD0 = 7 / 50, 2 / 25, 9 / 10, 1 / 5, 10.0, 1e-4
DONE, MAX_STEPS, DT_MIN = 0, 1, 2

# ---- the interpolant, restated (Tsitouras 2011, the free 4th-order interpolant over k1 .. k7): per weight the leading factor s,
# the roots r1, r2 and the quadratic factor th^2 - p th + q, in the forms of interp_weights
INTERP = {1: dict(s=-1.0530884977290216, r1=1.3299890189751412, p=1.4364028541716351, q=0.7139816917074209),
          2: dict(s=0.1017, p=2.1966568338249754, q=1.2949852507374631),
          3: dict(s=2.490627285651252793, p=2.38535645472061657, q=1.57803468208092486),
          4: dict(s=-16.54810288924490272, r1=1.21712927295533244, r2=0.61620406037800089),
          5: dict(s=47.37952196281928122, r1=1.203071208372362603, r2=0.658047292653547382),
          6: dict(s=-34.87065786149660974, r1=1.2, r2=0.666666666666666667),
          7: dict(s=2.5, r1=1.0, r2=0.6)}
# the twelve save times of every test, as fractions of t_span
SAVE_FRACS = (0.0, 0.013, 0.05, 0.051, 0.2, 0.37, 0.5, 0.62, 0.8, 0.97, 0.999, 1.0)


def interp_weights(th, coef=INTERP):
    """b_1 .. b_7 at th (a float or an array): b1 = s th (th - r1)(th^2 - p th + q), b2, b3 = s th^2 (th^2 - p th + q),
    b4 .. b7 = s th^2 (th - r1)(th - r2)"""
    th = np.asarray(th, dtype=np.float64)
    th2 = th * th
    quad = lambda c: th * (th - c["p"]) + c["q"]  # noqa: E731
    b = [coef[1]["s"] * th * (th - coef[1]["r1"]) * quad(coef[1]), coef[2]["s"] * th2 * quad(coef[2]), coef[3]["s"] * th2 * quad(coef[3])]
    b += [coef[i]["s"] * th2 * ((th - coef[i]["r1"]) * (th - coef[i]["r2"])) for i in (4, 5, 6, 7)]
    return b


def save_times(t_span):
    return np.array([f * t_span for f in SAVE_FRACS])


def plane_norms(nprog, norms=bench.NORMS):
    """mom_norms of a plan (helper_functions.jl:40-53): n0 m0^order per plane"""
    return np.array([norms[0] * norms[1] ** k for np_ in nprog for k in range(np_)])


def last_bit_noise(seed):
    rng = np.random.default_rng(seed)
    return lambda shape: 1.0 + 1e-15 * rng.choice([-1.0, 1.0], size=shape)


def adaptive_tsit5(rhs, u0, t_span, opts, *, nz=1, clamp=False, t_save=None):
    """u0 (planes, n) from t = 0 to t_span, one controller (t, dt, qold, cursor, status, counts) per GROUP of nz consecutive cells:
    nz = 1 a parcel, nz > 1 a column (group g holds cells g nz .. (g + 1) nz).  rhs(u) -> du/dt on the whole batch, in the units
    of u0 (physical).  opts: reltol, abstol, max_steps; dt (None / 0: automatic, a float, or one value per group); plane_norms
    (planes,): the plan's mom_norms; normalised (bool, default True): the state the controller sees is u / plane_norms (all-Inf
    plans) or u itself with abstol scaled by plane_norms (thresholded plans, columns).  The error norm sums the planes of a cell
    first, then the group's cells in cell order.

    clamp (the column rule): the first u is max(u0, 0), u_new is clamped before its evaluation (rhs itself evaluates on a clamped
    copy of its argument: the caller's function), and interpolated snapshots are clamped.

    t_save (None: no snapshot code runs): after an accepted step t -> t_new every save time t_save[j] <= t_new the group's cursor
    has not passed gets, in every cell of the group, u + h sum_i b_i(th) k_i with th = (t_save[j] - t) / h, or u_new itself where
    t_save[j] == t_new; a save time 0 gets the input as it is (not clamped); what a group does not reach stays NaN; t_span <= 0:
    every snapshot is the input (and rhs is never called).

    Returns dict(u, t, dt, accepted, rejected, status, evals), one entry per group but for u; with t_save also saved (n_save,
    planes, n), physical units, in_step: per group the number of save times that fell into each accepted step (a save time 0
    belongs to none), and rejected_before: per group the rejected steps it had when it took its first snapshot inside a step
    (-1: it took none)."""
    reltol, abstol, max_steps = float(opts["reltol"]), float(opts["abstol"]), int(opts["max_steps"])
    norms = np.asarray(opts["plane_norms"], dtype=np.float64)[:, None]
    normalised = bool(opts.get("normalised", True))
    planes, n = u0.shape
    ng = n // nz
    assert ng * nz == n
    count = planes * nz
    cells = lambda x: np.repeat(x, nz)   # noqa: E731  a group's value on its cells

    def group_sum(x):
        """(planes, n) -> (ng,): the planes of a cell first, then the group's cells in cell order"""
        part = x.sum(axis=0).reshape(ng, nz)
        s = np.zeros(ng)
        for j in range(nz):
            s = s + part[:, j]
        return s

    t = np.zeros(ng)
    accepted, rejected, status = np.zeros(ng, np.int64), np.zeros(ng, np.int64), np.zeros(ng, np.int64)
    evals = np.zeros(ng, np.int64)
    snap = {}
    if t_save is not None:
        t_save = np.asarray(t_save, dtype=np.float64)
        n_save = t_save.size
        saved = np.full((n_save, planes, n), np.nan)
        in_step = [[] for _ in range(ng)]
        rejected_before = np.full(ng, -1, np.int64)
        snap = dict(saved=saved, in_step=in_step, rejected_before=rejected_before)
    if not t_span > 0:
        if snap:
            saved[:] = u0[None]
        return dict(u=u0.copy(), t=t, dt=np.zeros(ng), accepted=accepted, rejected=rejected, status=status, evals=evals, **snap)
    if snap:
        cursor = np.zeros(ng, np.int64)
        if n_save and t_save[0] == 0.0:
            saved[0] = u0
            cursor += 1
    with np.errstate(all="ignore"):
        if normalised:
            u = u0 / norms
            f = lambda v: rhs(v * norms) / norms  # noqa: E731
            atol = np.full_like(u, abstol)
        else:
            u = u0.copy()
            f = rhs
            atol = abstol * norms * np.ones_like(u)
        if clamp:
            u = np.where(u < 0, 0.0, u)
        k1 = f(u)
        evals += 1
        dt0 = opts.get("dt")
        dt = np.zeros(ng) if dt0 is None else np.broadcast_to(np.asarray(dt0, dtype=np.float64), (ng,)).copy()
        auto = ~((dt > 0) & np.isfinite(dt))
        sc = atol + reltol * np.abs(u)
        d0, d1 = np.sqrt(group_sum((u / sc) ** 2) / count), np.sqrt(group_sum((k1 / sc) ** 2) / count)
        dt = np.where(auto, np.where(d1 == 0, t_span, 0.01 * d0 / d1), dt)
        dt = np.where(dt > t_span, t_span, dt)
        qold = np.full(ng, QOLD0)
        active = np.ones(ng, bool)
        t_last, dt_min = t_span * (1 - 4 * EPS), 1e-14 * t_span
        while True:
            over = active & (accepted + rejected >= max_steps)
            status[over], active[over] = MAX_STEPS, False
            small = active & (~(dt >= dt_min) | ~np.isfinite(dt))
            status[small], active[small] = DT_MIN, False
            if not active.any():
                break
            last = t + dt >= t_last
            h = np.where(last, t_span - t, dt)
            hc = cells(h)
            k = [k1]
            for row in A_ROWS[:-1]:
                k.append(f(u + hc * sum(a * ki for a, ki in zip(row, k))))
            u_new = u + hc * sum(a * ki for a, ki in zip(A_ROWS[-1], k))
            if clamp:
                u_new = np.where(u_new < 0, 0.0, u_new)
            k.append(f(u_new))
            evals[active] += 6
            err = hc * sum(b * ki for b, ki in zip(BTILDE, k))
            sc = atol + reltol * np.maximum(np.abs(u), np.abs(u_new))
            eest = np.sqrt(group_sum((err / sc) ** 2) / count)
            fin = np.isfinite(eest)
            q11 = np.where(eest > 0, np.where(fin, eest, 1.0) ** BETA1, 0.0)
            q = np.clip(q11 / qold ** BETA2 / GAMMA, 1 / QMAX, 1 / QMIN)
            acc = active & fin & (eest <= 1)
            rej = active & ~acc
            dt_acc = np.maximum(h / q, np.minimum(dt, dt / q))
            dt_rej = np.where(fin, h / np.minimum(1 / QMIN, q11 / GAMMA), h / 5.0)
            t_new = np.where(last, t_span, t + h)
            if snap:   # ---- the snapshots of this step (nothing in here feeds back into the integration)
                taken = np.zeros(ng, np.int64)
                while n_save:
                    ts = t_save[np.minimum(cursor, n_save - 1)]
                    m = acc & (cursor < n_save) & (ts <= t_new)
                    if not m.any():
                        break
                    b = interp_weights(cells((ts - t) / h))
                    mid = u + hc * sum(bi * ki for bi, ki in zip(b, k))
                    if clamp:
                        mid = np.where(mid < 0, 0.0, mid)
                    val = np.where(cells(ts == t_new), u_new, mid)
                    val = val * norms if normalised else val
                    idx = np.flatnonzero(cells(m))
                    saved[cells(cursor)[idx], :, idx] = val[:, idx].T
                    first = m & (rejected_before < 0)
                    rejected_before[first] = rejected[first]
                    cursor[m] += 1
                    taken[m] += 1
                for g in np.flatnonzero(acc):
                    in_step[g].append(int(taken[g]))
            t = np.where(acc, t_new, t)
            dt = np.where(acc, dt_acc, np.where(rej, dt_rej, dt))
            qold = np.where(acc, np.maximum(eest, QOLD0), qold)
            u = np.where(cells(acc), u_new, u)
            k1 = np.where(cells(acc), k[6], k1)
            accepted += acc
            rejected += rej
            active &= ~(acc & last)
    return dict(u=u * norms if normalised else u, t=t, dt=dt, accepted=accepted, rejected=rejected, status=status, evals=evals, **snap)


# ---- the C side: cloudy_adaptive_opts and what every entry point of the family answers to a bad one
def default_opts(cloudy, **kw):
    o = cloudy._lib.AdaptiveOptsC()
    cloudy.lib().cloudy_adaptive_opts_init(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def assert_adaptive_opts_refusals(cloudy, call, msg, *, n_parcels=4, buffers=("u_in", "u_out"), no_times=None, later=()):
    """The checks every entry point of the family makes through one path, in their order and before any device work: opts, its
    struct_size, reltol, abstol, dt_init, t_span, max_steps, ld, the two state buffers -- each answered with EINVAL and its
    message -- and the limits that pass them all and get as far as "plan is NULL".

    call(**kw) -> status: the file's closure; it takes opts= (an AdaptiveOptsC, None, or by default default_opts(cloudy, **kw)),
    ld=, t_span= and the two `buffers`, and its defaults hold n_parcels parcels with ld == n_parcels.  msg() -> the last error.
    no_times: the keywords that hand in no save times, for the entry points that compare their save times with t_span first.
    later: keyword dicts, each with arguments out of order that the entry point looks at AFTER all of these; every refusal is
    asserted as it stands and once more beside each of them."""
    EINVAL = cloudy._lib.EINVAL
    nan, inf = float("nan"), float("inf")
    plain = dict(no_times or {})

    def refused(words, exact=False, **kw):
        for extra in ({},) + tuple(later):
            assert call(**{**extra, **kw}) == EINVAL and (msg() == words if exact else words in msg()), (kw, extra, msg())

    def passes(**kw):
        assert call(**kw) == EINVAL and msg() == "plan is NULL", (kw, msg())

    refused("opts is NULL", exact=True, opts=None)
    short = default_opts(cloudy)
    short.struct_size -= 8
    refused("opts.struct_size", opts=short)
    for bad in (0.0, -1e-6, nan, inf):
        refused("reltol", reltol=bad)
    for bad in (-1e-9, nan, inf):
        refused("abstol", abstol=bad)
    passes(abstol=0.0)
    for bad in (-1.0, nan, inf):
        refused("dt_init", dt_init=bad)
    for bad in (-1.0, nan, inf, -inf):
        refused("t_span", t_span=bad, **plain)
    passes(t_span=0.0, **plain)
    for bad in (0, -1, 1000001):
        refused("max_steps", max_steps=bad)
    for good in (1, 1000000):
        passes(max_steps=good)
    refused(f"ld ({n_parcels - 1}) must be >= n_parcels ({n_parcels})", ld=n_parcels - 1)
    for buf in buffers:
        refused("device buffer is NULL", exact=True, **{buf: None})


def assert_symbol_agrees(cloudy, name, args):
    """One int-returning entry point with the argument kinds `args` ("ptr", "size_t", "int", "double") in the header, the ctypes
    table, the loaded library and exactly one ccall of the Julia shim"""
    assert _c_prototypes()[name] == ("int", list(args))
    res, argtypes = cloudy._lib.SYMBOLS[name]
    assert res is C.c_int and len(argtypes) == len(args) and hasattr(cloudy.lib(), name)
    calls = [c for c in _julia_ccalls(open(os.path.join(ROOT, "julia", "CloudyHIP.jl")).read()) if c[0] == name]
    assert len(calls) == 1 and calls[0][1] == "Cint" and len(calls[0][2]) == len(args)
