#!/usr/bin/env python3
"""test/examples/Analytical/parcel_example.jl of the reference through the Python mirror of the Cloudy API (cloudy.jl_amd): an
adiabatic parcel rising at w = 10 m/s from T = 280.15 K, p = 800 hPa, S = 1, with 200 droplets per cm^3 of 8 um radius as a
Monodisperse, a Gamma (k = 2) and an Exponential + Gamma size distribution; SSPRK33 with dt = 0.5 s over 40 steps.  The
saturation ratio, pressure, temperature and vapour content are prognostic beside the moments (cloudy_parcel_ssprk33_steps).

    python examples/parcel_example.py [--adaptive]

--adaptive: the same 0.5 s series from ONE launch of the per-parcel adaptive Tsit5 (cloudy_parcel_tsit5_adaptive, reltol 1e-6)
through its dense output at the 41 save times, instead of 40 calls of one fixed step.

Needs a GPU (the package has no CPU path).  The Julia original plots; this prints the supersaturation [%] and the mean radius
[um] of the first mode every 2 s.  Unlike the driver as written, condensation acts on the distributions updated from the
current moments (include/cloudy_hip.h says why)."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

cl = load_package()

params = cl.ParcelParams()
rho_l = params.rho_l
r0, N = 8e-6, 200 * 1e6                                  # parcel_example.jl:116-118
m0 = 4 / 3 * math.pi * r0**3 * rho_l
p0, T0, S0, w, const_dt, t_max = 800 * 1e2, 273.15 + 7.0, 1.0, 10.0, 0.5, 20.0   # :174-184
norms = (1e8, 1e-12)


def init_conditions(kind):
    """:114-146"""
    if kind == "monodisperse":
        return (cl.MonodispersePrimitiveParticleDistribution(N, m0),)
    if kind == "gamma":
        return (cl.GammaPrimitiveParticleDistribution(N, m0 / 2, 2.0),)
    M0, M1 = [9 * N / 10, N / 10], [N * m0 / 2, N * m0 / 2]
    return (cl.ExponentialPrimitiveParticleDistribution(M0[0], M1[0] / M0[0]),
            cl.GammaPrimitiveParticleDistribution(M0[1], M1[1] / M0[1] / 2.0, 2.0))


def saturation_vapor_pressure(T):
    dcp = params.cp_v - params.cp_l
    return params.press_triple * (T / params.T_triple) ** (dcp / params.R_v) * math.exp(
        (params.LH_v0 - dcp * params.T_0) / params.R_v * (1 / params.T_triple - 1 / T))


if __name__ == "__main__":
    e = saturation_vapor_pressure(T0)                    # :176-179
    md_v, mv_v = (p0 - e) / params.R_d / T0, e / params.R_v / T0
    for kind in ("monodisperse", "gamma", "mixture"):
        pdists = init_conditions(kind)
        NProgMoms = tuple(cl.nparams(d) for d in pdists)
        moments = [cl.get_moments(d) for d in pdists]
        ml_v = sum(m[1] for m in moments)
        q_v = mv_v / (md_v + mv_v + ml_v)                # :218
        Y0 = np.concatenate([[S0, p0, T0, q_v]] + moments)
        cd = cl.CoalescenceData(cl.CoalescenceTensor([[1.0]]), NProgMoms, (math.inf,) * len(pdists), norms)
        par = cl.ODEParameters(pdists, cd, NProgMoms, norms)
        y = cl.DeviceArray.from_numpy(np.ascontiguousarray(Y0[:, None]))
        print(f"{kind}:  t [s]   supersaturation [%]   mean radius [um]   T [K]")
        n_out = int(round(t_max / const_dt)) + 1
        series = None
        if "--adaptive" in sys.argv[1:]:
            saved, acc, rej, _, _ = cl.solve_parcel_tsit5_adaptive(par, y, w, t_max, params=params, times=const_dt * np.arange(n_out),
                                                                   info=True)
            series = saved.to_numpy().reshape(n_out, len(Y0))
            print(f"    (adaptive: {int(acc[0])} accepted, {int(rej[0])} rejected steps)")
        for step in range(n_out):
            Y = y.to_numpy()[:, 0] if series is None else series[step]
            if step % 4 == 0:
                r_l = (Y[5] / Y[4] / rho_l / 4 / math.pi * 3) ** (1 / 3) * 1e6   # :246-249
                print(f"    {step * const_dt:6.1f}   {(Y[0] - 1) * 100:10.5f}   {r_l:14.5f}   {Y[2]:12.5f}")
            if series is None:
                cl.solve_parcel_ssprk33(par, y, w, const_dt, 1, params=params)
