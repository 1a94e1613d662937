#!/usr/bin/env python3
"""Generator of tests/golden/special_functions.json: 40-digit (mpmath, 60 working digits) reference values for the
hand-written special functions of csrc/device_math.hpp and csrc/kernels.hpp, reached through the diagnostic entry points
(cloudy_finite_2d_integrals, cloudy_compute_thresholds, cloudy_standard_N_q, cloudy_sedimentation_flux, cloudy_cond_evap,
cloudy_update_dist_from_moments).  Every block is a fixed case list; nothing is random and nothing outside this file is read.

    python tools/make_special_goldens.py            writes the JSON
    python tools/make_special_goldens.py --check    regenerates it and compares with the committed file

Inputs are stored as doubles (repr round-trips), expected values as 17-digit decimal strings.  Every expected value is a
function of the STORED doubles (moments are rounded first and then inverted exactly), so the file carries no input error.
tests/test_special_goldens_host.py (oracle) and tests/test_gpu_special_goldens.py (device) read the file; the host test
regenerates every tenth case through the functions below."""
import json
import math
import os
import sys

import mpmath as mp

mp.mp.dps = 60
EPS = 2.0 ** -52
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "special_functions.json")
F = mp.mpf
P_TENSOR = 3          # tensor_p of the F plans: orders p1 <= p2 <= P + 1 = 4
M = P_TENSOR + 2
K_RANGE = (EPS, 40.0)  # of the moment-plane plan: the shape list crosses lgamma's shift at 10
CUTOFF = 1.0
MINX = 1e-18
GAMMA, EXP, MONO, LOGN = 1, 0, 2, 3


def s17(x):
    """17 significant digits; inf / 0 spelled so that float() reads them"""
    x = F(x)
    if mp.isinf(x):
        return "inf"
    return mp.nstr(x, 17, min_fixed=0, max_fixed=0, strip_zeros=False)


# ------------------------------------------------------------------------------------------------- F block
F_FORMULA = (
    "F[p1][p2] = min(M_p1 M_p2, H), p1 <= p2 <= 4, for Gamma(n, theta, k) (Exponential: k = 1) and threshold x_t; "
    "M_p = n theta^p Gamma(k+p)/Gamma(k); H = n^2 theta^(p2-k) Gamma(k+p2)/Gamma(k)^2 * dx * sum_{j=1..nb} w_j x_j^(p1+k) "
    "exp(-x_j/theta) P(k+p2, (x_t-x_j)/theta), the Simpson node sum of moment_source_helper itself (not the integral): "
    "x_lb = min(1e-5, 1e-5 x_t) and nb = floor(nbpl log10(x_t/x_lb)) in double arithmetic, ln x_j = ln x_lb + (j-1) dx, "
    "dx = (ln x_t - ln x_lb)/nb exactly, w = 17/48, 59/48, 43/48, 49/48 on the first four nodes and on nodes nb-2, nb-1, nb "
    "(49, 43, 59; the node nb+1 = x_t contributes 0), 1 elsewhere.  n is a power of two chosen so that every M_p >= 1 "
    "(the reference zeroes entries with M_p1 M_p2 < eps).  Stored per case: 'mm' = M_p1 M_p2 and 'F', both in the order "
    "(p1, p2) = (0,0), (0,1), ..., (0,4), (1,1), ..., (4,4).")

# plan slots: (plan, n_bins_per_log_unit, [(dist, x_t) for the three thresholded modes]); the fourth mode is unthresholded
F_PLANS = {
    "A": (15, [(GAMMA, 1e-6), (GAMMA, 3e-3), (GAMMA, 1.0)]),
    "B": (20, [(GAMMA, 0.5), (GAMMA, 7.0), (EXP, 1.0)]),
    "C": (10, [(GAMMA, 7.0), (EXP, 0.5), (GAMMA, 3e-3)]),
}
F_K = [EPS, 1e-9, 0.05, 0.5, 1.0, 2.0, 4.2, 9.6, 10.0]
F_Z0 = [1e-3, 0.4, 1.0, "sw-", "sw+", 15.0, 117.0, 300.0, 700.0]   # sw+-: a_top + 1 +- 1e-6, a_top = k + 4
# (k, z0, x_t) of tests/test_early_series_math.py; an x_t that no slot has goes to the slot x_t = 3e-3
EARLY = [(1e-9, 24.7, 1.0), (0.05, 0.4, 3e-3), (0.5, 117.0, 1.0), (1.0, 190.0, 5e-4), (1.0, 2.5e-3, 1.0), (2.7, 17.8, 5e-1),
         (4.2, 5.5, 5e-10 / 1e-9), (6.8, 3.7, 1.0), (8.2, 2e-3, 1e-2), (9.6, 2e-3, 1.0), (10.0, 15.0, 1.0), (10.0, 300.0, 7.0),
         (3.0, 57.0, 1e-6), (7.6, 38.7, 1.0)]
# the a E < 1e-18 exit of the continued-fraction branch fires for the top order near z = 60 and not for order 0
SHORTCUT = [(0.5, 55.0), (0.5, 62.0), (2.0, 66.0), (1e-9, 58.0)]


def f_case_inputs():
    """[(plan, mode, dist, x_t, nbpl, k, theta)] in file order"""
    out = []
    for si, (plan, (nbpl, slots)) in enumerate(F_PLANS.items()):
        for mode, (dist, xt) in enumerate(slots):
            s = 3 * si + mode
            kz = []
            for i, k in enumerate(F_K if dist == GAMMA else [1.0]):
                for j, z in enumerate(F_Z0):
                    if dist == GAMMA and (i + j + s) % 3:
                        continue
                    kz.append((k, (k + 5.0) - 1e-6 if z == "sw-" else (k + 5.0) + 1e-6 if z == "sw+" else z))
            if dist == GAMMA:
                for k, z0, x in EARLY:
                    if x == xt or (plan == "A" and xt == 3e-3 and x in (5e-4, 1e-2)):
                        kz.append((k, z0))
                if s % 3 == 0:
                    kz += SHORTCUT
            for k, z0 in kz:
                out.append((plan, mode, dist, xt, nbpl, k, xt / z0))
    return out


def f_grid(xt, nbpl):
    x_lb = min(1e-5, 1e-5 * xt)
    nb = int(math.floor(nbpl * math.log10(xt / x_lb)))
    return x_lb, nb


def gamma_ratio(k, q):
    """Gamma(k + q) / Gamma(k)"""
    return mp.gamma(F(k) + q) / mp.gamma(F(k)) if k > 1e-3 else mp.exp(mp.loggamma(F(k) + q) - mp.loggamma(F(k)))


def f_norm_n(theta, k):
    worst = min(F(theta) ** p * gamma_ratio(k, p) for p in range(M))
    return 2.0 ** max(0, int(mp.ceil(-mp.log(worst, 2))))


def f_expected(n, theta, k, xt, nbpl):
    n, th, k_, x_t = F(n), F(theta), F(k), F(xt)
    x_lb, nb = f_grid(xt, nbpl)
    lx0 = mp.log(F(x_lb))
    dx = (mp.log(x_t) - lx0) / nb
    wend = [F(17) / 48, F(59) / 48, F(43) / 48, F(49) / 48]
    acc = [[F(0)] * M for _ in range(M)]
    for j in range(1, nb + 1):
        w = F(1) if 5 <= j <= nb - 3 else F(0)
        if j <= 4:
            w += wend[j - 1]
        if nb + 1 - j in (1, 2, 3):
            w += wend[nb + 1 - j]
        x = mp.exp(lx0 + (j - 1) * dx)
        z = (x_t - x) / th
        Pz = [None] * M
        Pz[M - 1] = mp.gammainc(k_ + (M - 1), 0, z, regularized=True)
        for p2 in range(M - 2, -1, -1):   # P(a-1, z) = P(a, z) + z^(a-1) e^-z / Gamma(a): all terms positive
            a = k_ + p2 + 1
            Pz[p2] = Pz[p2 + 1] + mp.exp((a - 1) * mp.log(z) - z - mp.loggamma(a))
        base = w * x ** k_ * mp.exp(-x / th)
        for p1 in range(M):
            for p2 in range(p1, M):
                acc[p1][p2] += base * x ** p1 * Pz[p2]
    Mq = [n * th ** p * gamma_ratio(k, p) for p in range(M)]
    gk = mp.gamma(k_)
    mm, Fv = [], []
    for p1 in range(M):
        for p2 in range(p1, M):
            H = n * n * th ** (p2 - k_) * mp.gamma(k_ + p2) / (gk * gk) * dx * acc[p1][p2]
            m = Mq[p1] * Mq[p2]
            mm.append(s17(m))
            Fv.append(s17(min(m, H)))
    return mm, Fv


def f_block(only=None):
    cases = []
    for idx, (plan, mode, dist, xt, nbpl, k, theta) in enumerate(f_case_inputs()):
        if only is not None and idx not in only:
            continue
        n = f_norm_n(theta, k)
        mm, Fv = f_expected(n, theta, k, xt, nbpl)
        cases.append({"plan": plan, "mode": mode, "n": n, "theta": theta, "k": k, "nb": f_grid(xt, nbpl)[1], "mm": mm, "F": Fv})
    return cases


# ------------------------------------------------------------------------------------------------- thresholds
T_FORMULA = (
    "x = max(theta z, 1e-18) with P(k, z) = p (compute_threshold, MovingThreshold) for Gamma(., theta, k); p = 0 gives 1e-18, "
    "p = 1 gives inf.  z by mpmath bisection on ln z (70 halvings of a bracket from the bounds e^-z z^k <= Gamma(k+1) P <= z^k, "
    "then three Newton steps on the smaller tail: P - p for p <= 1/2, Q - (1 - p) otherwise, 1 - p exact in double).  Where the "
    "upper bound of theta z is below 1e-18 (the tiny-k exits) the value is the clamp and no root is sought.")
T_PLANS = {"T0": (1e-12, 1e-6, 0.01), "T1": (0.5, 0.9, 0.97), "T2": (0.99, 1 - 1e-6, 1 - 1e-12), "T3": (0.0, 1.0, 0.97)}
T_K = [EPS, 1e-8, 1e-3, 0.05, 0.5, 1 - 1e-9, 1 + 1e-9, 1.5, 2.0, 9.99, 10.0, 10.01, 40.0]
T_TH = [1.0, 3.7e-3, 250.0]


def t_case_inputs():
    out = []
    for plan, ps in T_PLANS.items():
        for mode, p in enumerate(ps):
            for i, k in enumerate(T_K):
                out.append((plan, mode, p, k, T_TH[(i + mode) % 3]))
    return out


def t_expected(p, k, theta):
    if p <= 0.0:
        return F(MINX)
    if p >= 1.0:
        return mp.inf
    k_, p_, th = F(k), F(p), F(theta)
    q_ = 1 - p_
    lg = mp.loggamma(k_ + 1)
    lo = (mp.log(p_) + lg) / k_ - 1                 # z^k >= Gamma(k+1) p
    if mp.log(th) + (1 + mp.log(p_) + lg) / k_ < mp.log(F(MINX)) - 1:   # z <= 1 and e^-1 z^k <= Gamma(k+1) p
        return F(MINX)
    hi = mp.log(k_ + 40 * mp.sqrt(k_) + 120)

    def err(l):
        z = mp.exp(l)
        if p <= 0.5:
            return mp.gammainc(k_, 0, z, regularized=True) - p_
        # (below z = 1 the upper function is 1 - P: nothing is lost to 60 digits, and mpmath's own upper series does not converge)
        return q_ - (mp.gammainc(k_, z, mp.inf, regularized=True) if l > 0 else 1 - mp.gammainc(k_, 0, z, regularized=True))

    assert err(lo) < 0 < err(hi), (p, k)
    for _ in range(70):
        mid = (lo + hi) / 2
        if err(mid) < 0:
            lo = mid
        else:
            hi = mid
    l = (lo + hi) / 2
    for _ in range(3):   # d/dl of P(k, e^l) = z^k e^-z / Gamma(k)
        z = mp.exp(l)
        l -= err(l) / mp.exp(k_ * l - z - mp.loggamma(k_))
    assert abs(err(l)) < mp.mpf(10) ** -44 * min(p_, q_), (p, k)
    return max(th * mp.exp(l), F(MINX))


def t_block(only=None):
    return [{"plan": plan, "mode": mode, "p": p, "k": k, "theta": th, "x": s17(t_expected(p, k, th))}
            for i, (plan, mode, p, k, th) in enumerate(t_case_inputs()) if only is None or i in only]


# ------------------------------------------------------------------------------------------------- moment-plane blocks
# one plan: modes (Exponential, Gamma, Lognormal, Monodisperse), norms (1, 1), k_range K_RANGE; a parcel is 10 moments
MODES = (EXP, GAMMA, LOGN, MONO)


def moments_of(dist, n, a, b=1.0):
    """the prognostic moments of a mode in 60 digits, rounded to double"""
    n, a_, b_ = F(n), F(a), F(b)
    if dist == GAMMA:
        m = [n, n * b_ * a_, n * b_ * (b_ + 1) * a_ * a_]          # (theta = a, k = b)
    elif dist == LOGN:
        m = [n, n * mp.exp(a_ + b_ * b_ / 2), n * mp.exp(2 * a_ + 2 * b_ * b_)]   # (mu = a, sigma = b)
    else:
        m = [n, n * a_]
    return [float(v) for v in m]


def invert(dist, m, k_range=K_RANGE):
    """update_dist_from_moments (ParticleDistributions.jl:456-541) in exact arithmetic on double moments"""
    m = [F(v) for v in m]
    e = F(EPS)
    if dist == LOGN:
        if not (m[0] > e and m[1] > e and m[2] > e):
            return F(0), F(1), F(1)
        mu = mp.log(m[1] * m[1] / m[0] ** F(1.5) / mp.sqrt(m[2]))
        sg = max(e, mp.sqrt(mp.log(m[0] * m[2] / (m[1] * m[1]))))
        return m[1] / mp.exp(mu + sg * sg / 2), mu, sg
    if not (m[0] > e and m[1] > e):
        return F(0), F(1), F(1)
    mean = m[1] / m[0]
    if dist != GAMMA:
        return m[0], mean, F(1)
    d = m[2] / m[1] - mean
    kk = mean / d if d != 0 else mp.inf
    k = max(F(k_range[0]), min(F(k_range[1]), kk))
    return m[0], mean / k, k


def moment(dist, prm, q):
    n, a, b = prm
    if dist in (GAMMA, EXP):
        return n * a ** q * mp.exp(mp.loggamma(b + q) - mp.loggamma(b))
    if dist == MONO:
        return n * a ** q
    return n * mp.exp(q * a + q * q * b * b / 2)


def partial(dist, prm, q, c):
    """(below, above) the size cutoff c of the q-th moment: partial_moment and its complement, each in closed form"""
    n, a, b = prm
    Mq = moment(dist, prm, q)
    if n == 0:
        return F(0), F(0)
    if dist in (GAMMA, EXP):
        return (Mq * mp.gammainc(b + q, 0, c / a, regularized=True), Mq * mp.gammainc(b + q, c / a, mp.inf, regularized=True))
    if dist == MONO:
        return (F(0), Mq) if c < a else (Mq, F(0))
    w = (mp.log(c) - a - q * b * b) / b
    return Mq * mp.ncdf(w), Mq * mp.ncdf(-w)


NQ_FORMULA = (
    "get_standard_N_q at size_cutoff = 1 for a parcel of four modes (Exponential, Gamma, Lognormal, Monodisperse; norms (1, 1), "
    "k_range (eps, 40)): 'mom' = the 10 double moments; the modes are inverted exactly (update_dist_from_moments with its "
    "clamps and its fallback (0, 1, 1) for moments <= eps) and out = (N_liq, N_rai, M_liq, M_rai) = sums over the modes of "
    "M_q P(k+q, 1/theta), M_q Q(k+q, 1/theta) (gammainc closed forms, q = 0, 1), the Lognormal ones "
    "M_q Phi(+-(ln 1 - mu - q sigma^2)/sigma) (erfc closed forms), Monodisperse a step.  Most parcels have one live mode "
    "(the others are empty) so that the bound applies to that mode alone; the last ones are mixtures.")
NQ_K = [1e-9, 0.05, 0.5, 1.0, 2.0, 4.2, 9.6, 10.0]
NQ_Z = [1e-6, 1e-3, 0.4, 1.0, "sw-", "sw+", 15.0, 60.0, 117.0, 300.0, 1e3]   # sw+-: (k + 1) + 1 +- 1e-6, the switch of P(k+1, z)


def nq_case_inputs():
    """[[(n, a, b) per mode]]"""
    dead = (0.0, 1.0, 1.0)
    out = []
    for i, k in enumerate(NQ_K):
        for j, z in enumerate(NQ_Z):
            if (i + j) % 2 and z not in ("sw-", "sw+"):
                continue
            zz = (k + 2.0) - 1e-6 if z == "sw-" else (k + 2.0) + 1e-6 if z == "sw+" else z
            out.append([dead, (3.0, CUTOFF / zz, k), dead, dead])
    for z in NQ_Z:
        if isinstance(z, float):
            out.append([(5.0, CUTOFF / z, 1.0), dead, dead, dead])
    for mu in (-13.8, -3.0, -0.4, 0.0, 0.7, 6.9):
        for sg in (0.02, 0.3, 1.0, 2.2):
            out.append([dead, dead, (2.0, mu, sg), dead])
    for th in (1e-3, 0.5, 2.0):
        out.append([dead, dead, dead, (7.0, th, 1.0)])
    for t in range(12):   # mixtures with comparable number in every mode
        z = [1e-6, 0.02, 0.4, 1.0, 3.0, 15.0, 60.0, 300.0, 1e3, 7.0, 0.1, 30.0][t]
        out.append([(1.0, CUTOFF / z, 1.0), (2.0, CUTOFF / z / 2, NQ_K[t % 8]), (1.5, -math.log(z), 0.5 + 0.1 * t), (0.5, 3.0 / z, 1.0)])
    return out


def pack_mom(modes):
    mom = []
    for dist, (n, a, b) in zip(MODES, modes):
        mom += [0.0] * (3 if dist in (GAMMA, LOGN) else 2) if n == 0 else moments_of(dist, n, a, b)
    return mom


def split_mom(mom):
    return [mom[0:2], mom[2:5], mom[5:8], mom[8:10]]


def nq_expected(mom):
    out = [F(0)] * 4
    for dist, m in zip(MODES, split_mom(mom)):
        prm = invert(dist, m)
        for q in (0, 1):
            lo, hi = partial(dist, prm, q, F(CUTOFF))
            out[2 * q] += lo
            out[2 * q + 1] += hi
    return [s17(v) for v in out]


def nq_block(only=None):
    return [{"mom": m, "out": nq_expected(m)} for i, m in enumerate(map(pack_mom, nq_case_inputs())) if only is None or i in only]


FM_FORMULA = (
    "fractional moments M_q = moment(dist, q) of the four modes of a parcel (same plan as standard_N_q) after the exact "
    "inversion of the 10 double moments 'mom': Gamma / Exponential n theta^q Gamma(k+q)/Gamma(k), Lognormal "
    "n exp(q mu + q^2 sigma^2/2), Monodisperse n theta^q.  'sed': -M_(j-1+1/6) (get_sedimentation_flux, one velocity term "
    "(1, 1/6)); 'sed2': -(M_(j-1+1/6) + M_(j-1+1/2)) (terms (1, 1/6), (1, 1/2)); 'cond': 3 (j-1) M_(j-1-2/3) (4 pi/3)^(2/3) / "
    "1000^(1/3) (get_cond_evap, xi = s = 1, rho_l = 1000); j = 1..nparams of the mode, planes in the plan's order.")
FM_K = [EPS, 1e-9, 1e-3, 0.3, 1.0, 2.0, 9.999, 10.0, 10.001, 37.0]
FM_TH = [1.0, 2.5e-4, 40.0, 0.3]


def fm_case_inputs():
    out = []
    for i, k in enumerate(FM_K):
        for t in range(3):
            th = FM_TH[(i + t) % 4]
            n_g = 3.0 * 2.0 ** max(0, math.ceil(-math.log2(k * th)))   # M1 = n k theta >= 1: a tiny shape is not the fallback
            out.append([(2.0, th * (1 + 0.1 * i), 1.0), (n_g, th, k), (1.5, math.log(th) + 0.1 * i, (0.05, 0.6, 1.7)[t]),
                        (0.5, th * (2 + t), 1.0)])
    return out


def fm_expected(mom):
    sed, sed2, cond = [], [], []
    c = (4 * mp.pi / 3) ** (F(2) / 3) / F(1000) ** (F(1) / 3)
    for dist, m in zip(MODES, split_mom(mom)):
        prm = invert(dist, m)
        for j in range(1, len(m) + 1):
            a, b = moment(dist, prm, j - 1 + F(1) / 6), moment(dist, prm, j - 1 + F(1) / 2)
            sed.append(s17(-a))
            sed2.append(s17(-(a + b)))
            cond.append(s17(3 * (j - 1) * moment(dist, prm, j - 1 - F(2) / 3) * c) if j > 1 else "0")
    return sed, sed2, cond


def fm_block(only=None):
    out = []
    for i, m in enumerate(map(pack_mom, fm_case_inputs())):
        if only is None or i in only:
            sed, sed2, cond = fm_expected(m)
            out.append({"mom": m, "sed": sed, "sed2": sed2, "cond": cond})
    return out


CL_FORMULA = (
    "update_dist_from_moments of the double moments 'mom' in exact arithmetic with k_range (eps, 40): 'params' = (n, theta, k) of "
    "the Exponential, Gamma and Monodisperse modes (the Lognormal mode of the plan holds fixed moments and is not part of "
    "this block).  The bound of the suite is 4 eps, and k = (M1/M0) / (M2/M1 - M1/M0) loses (2k + 1)/2 eps to the two "
    "quotients in ANY double evaluation, so the cases are of two kinds: 'generic' (n, theta, k) with k <= 2, where that loss "
    "stays inside the bound, and 'dyadic' ones (n, theta powers of two, k a multiple of 2^-20) whose moments and quotients are "
    "exact in double, up to k just below and just above either clamp.")
CL_GENERIC = [(3.0, 0.7, k) for k in (3 * EPS, 1e-9, 1e-3, 0.3, 1.0, 1.7, 2.0)] + [(1e6, 3.3e-9, 0.41), (2.5e-3, 811.0, 1.3)]
CL_DYADIC = [(4.0, 0.5, k) for k in (9.75, 10 - 2.0 ** -20, 10.0, 10 + 2.0 ** -20, 39.5, 40 - 2.0 ** -20, 40.0, 40 + 2.0 ** -20,
                                     41.0, 2.0 ** -20, 1.0, 0.5)]
CL_TINY = [(2.0 ** 60, 1.0, EPS / 2), (2.0 ** 60, 1.0, EPS), (2.0 ** 60, 1.0, 2 * EPS)]   # below, at and above the lower clamp


def cl_case_inputs():
    return [[(n, th * 1.5, 1.0), (n, th, k), (1.0, 0.0, 1.0), (n, th / 3, 1.0)] for n, th, k in CL_GENERIC + CL_DYADIC + CL_TINY]


def cl_expected(mom):
    out = []
    for dist, m in zip(MODES, split_mom(mom)):
        if dist != LOGN:
            out += [s17(v) for v in invert(dist, m)]
    return out


def cl_block(only=None):
    return [{"mom": m, "params": cl_expected(m)} for i, m in enumerate(map(pack_mom, cl_case_inputs())) if only is None or i in only]


BLOCKS = {"F": f_block, "thresholds": t_block, "standard_N_q": nq_block, "fractional_moments": fm_block, "closure": cl_block}


def generate():
    return {
        "generator": "tools/make_special_goldens.py (mpmath, 60 working digits; expected values as 17-digit decimals)",
        "F": {"formula": F_FORMULA, "tensor_p": P_TENSOR,
              "plans": {p: {"n_bins_per_log_unit": nb, "dist_types": [d for d, _ in sl] + [GAMMA], "x_t": [x for _, x in sl]}
                        for p, (nb, sl) in F_PLANS.items()},
              "cases": f_block()},
        "thresholds": {"formula": T_FORMULA, "method": "quantile by mpmath bisection on ln x",
                       "k_range": list(K_RANGE),
                       "plans": {p: list(v) for p, v in T_PLANS.items()}, "cases": t_block()},
        "moment_plan": {"dist_types": list(MODES), "k_range": list(K_RANGE), "norms": [1.0, 1.0], "size_cutoff": CUTOFF},
        "standard_N_q": {"formula": NQ_FORMULA, "cases": nq_block()},
        "fractional_moments": {"formula": FM_FORMULA, "cases": fm_block()},
        "closure": {"formula": CL_FORMULA, "cases": cl_block()},
    }


def main():
    text = json.dumps(generate(), indent=0, separators=(",", ":")) + "\n"
    if "--check" in sys.argv:
        with open(OUT) as f:
            same = f.read() == text
        print("special_functions.json:", "reproduced" if same else "DIFFERS from the generator's output")
        return 0 if same else 1
    with open(OUT, "w") as f:
        f.write(text)
    print("wrote", OUT, len(text), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
