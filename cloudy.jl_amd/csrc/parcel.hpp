// parcel.hpp -- the adiabatic parcel: prognostic supersaturation coupled to the moments through condensation
// (cloudy_parcel_ssprk33_steps, cloudy_parcel_rhs, cloudy_parcel_thermo_host).
//
// The reference's driver test/examples/Analytical/parcel_example.jl integrates Y = (S, p, T, q_v, mom...) with SSPRK33 and a fixed
// dt: the saturation ratio, pressure, temperature and vapour content of a parcel rising at speed w are prognostic beside the moments
// and coupled to them through get_cond_evap (src/Sources/Condensation.jl:22-37) -- droplet growth depletes the vapour, latent heat
// warms the parcel, the supersaturation peaks and relaxes (Rogers 1975).  Its thermodynamics come from Thermodynamics.jl and
// CloudMicrophysics.jl, which are not part of the reference tree; the closure is restated here in full, every constant a field of
// ParcelParams (cloudy_parcel_params of include/cloudy_hip.h):
//   R_m(q_t, q_l)  = R_d (1 + (R_v/R_d - 1) q_t - (R_v/R_d) q_l)
//   cp_m(q_t, q_l) = cp_d + (cp_v - cp_d) q_t + (cp_l - cp_v) q_l
//   L(T)           = LH_v0 + (cp_v - cp_l)(T - T_0)
//   p_vs(T)        = press_triple (T/T_triple)^((cp_v-cp_l)/R_v) exp((LH_v0 - (cp_v-cp_l) T_0)/R_v (1/T_triple - 1/T))
//   xi(T)          = 1 / ( L/(K_therm T) (L/(R_v T) - 1) + R_v T / (D_vapor p_vs) )
//   rho0 = p / (R_m(q_v, 0) T)                       parcel_example.jl:34
//   q_l  = sum_modes M1_mode / rho0                  :37-41
//   R = R_m(q_v + q_l, q_l), cp = cp_m(q_v + q_l, q_l), rho = p / (R T)      :44-47
//   a1 = L g/(cp T^2 R_v) - g/(R T), a2 = 1/q_v, a3 = L^2/(R_v T^2 cp)       :50-52
//   dmom = get_cond_evap(update_dist_from_moments(mom), S - 1, xi(T), rho_l), dq_l = sum_modes dmom[M1_mode] / rho
//   dS = a1 w S - (a2 + a3) S dq_l, dp = -p g w/(R T), dT = -g w/cp + L dq_l/cp, dq_v = -dq_l
// Normalisation goes through the plan's norms as in rhs_condensation! (box_model_helpers.jl:55-67), with rho_l from ParcelParams
// instead of the fixed 1000 of cloudy_cond_evap.
//
// SEMANTICS.  parcel_example.jl:19 binds `pdists` before :55-61 rebuild `p.pdists`, so the driver as written hands
// get_cond_evap the INITIAL distributions at every call.  This file builds the intended form -- the distributions updated from
// the current moments, as every other right-hand side of the reference does.  (Against the Rogers points the driver plots, 40
// steps of the monodisperse case: 0.078 percentage points / 0.029 um with the updated distributions, 0.25 / 0.054 with the stale.)
//
// The body calls the per-parcel device functions of kernels.hpp (invert_closure, cond_evap_parcel, coal_ints_parcel,
// div_by_const); this header includes kernels.hpp alone.
#pragma once
#include "kernels.hpp"

namespace cloudy {

#ifndef CLOUDY_SRC_BITS   // (box_sources.hpp defines the same two)
#define CLOUDY_SRC_BITS
enum { SRC_COAL = 1, SRC_COND = 2 };  // CLOUDY_SRC_* of include/cloudy_hip.h
#endif

// cloudy_parcel_params without its struct_size: a kernel argument
struct ParcelParams {
    double R_d, R_v, cp_d, cp_v, cp_l, LH_v0, T_0, press_triple, T_triple, grav, K_therm, D_vapor, rho_l;
};
struct ParcelThermo {
    double rho, R, cp, L, p_vs, xi, a1, a3;
};

// The closure, (S, p, T, q_v, sum of the modes' mass moments in physical units) -> (rho, R, cp, L, p_vs, xi, a1, a3): ONE
// definition for the kernels and for cloudy_parcel_thermo_host.  p_vs is one logarithm and one exponential; on the device they
// are log_pos / exp_fin of device_math.hpp (T / T_triple is positive and finite for any state worth stepping, the exponent a
// few units), on the host the library routines.  S does not enter: it multiplies a1 .. a3 in the tendencies.
__host__ __device__ inline ParcelThermo parcel_thermo(const ParcelParams &c, double /*S*/, double p, double T, double q_v, double m_liq) {
    ParcelThermo o;
    const double rvd = c.R_v / c.R_d, dcp = c.cp_v - c.cp_l;
    const double rho0 = p / (c.R_d * (1.0 + (rvd - 1.0) * q_v) * T);
    const double q_l = m_liq / rho0, q_t = q_v + q_l;
    o.R = c.R_d * (1.0 + (rvd - 1.0) * q_t - rvd * q_l);
    o.cp = c.cp_d + (c.cp_v - c.cp_d) * q_t + (c.cp_l - c.cp_v) * q_l;
    o.rho = p / (o.R * T);
    o.L = c.LH_v0 + dcp * (T - c.T_0);
    const double e1 = dcp / c.R_v, e2 = (c.LH_v0 - dcp * c.T_0) / c.R_v, inv_T = 1.0 / T;
    const double arg = e2 * (1.0 / c.T_triple - inv_T);
#if defined(__HIP_DEVICE_COMPILE__)
    o.p_vs = c.press_triple * exp_fin(fma(e1, log_pos(T / c.T_triple), arg));
#else
    o.p_vs = c.press_triple * std::exp(e1 * std::log(T / c.T_triple) + arg);
#endif
    const double LT = o.L * inv_T;   // L / T
    o.xi = 1.0 / (LT / c.K_therm * (LT / c.R_v - 1.0) + c.R_v * T / (c.D_vapor * o.p_vs));
    o.a1 = LT * inv_T * c.grav / (o.cp * c.R_v) - c.grav / (o.R * T);
    o.a3 = LT * LT / (c.R_v * o.cp);
    return o;
}

// dY of one parcel: t = (S, p, T, q_v), u the moments in normalised units -> ft, f (normalised units).  One closure inversion
// feeds the condensation term -- cond_evap_parcel with coef0 xi(T) and s = S - 1 as its coef / sv; coef0 = 3 (4 pi/3)^(2/3) /
// (rho_l^(1/3) norms[2]^(2/3)) is folded on the host -- and, with SRC_COAL, coal_ints_parcel<MODE_ALLINF>.  Only the condensation
// term enters dq_l (coalescence conserves the mass of the modes' sum).
template <int N, int P, bool SPEC, int SRC>
__device__ __forceinline__ void parcel_tendency(const KArgs<N, P> &As, const ParcelParams &c, double coef0, double w, const double (&t)[4],
                                                const double (&u)[N][3], double (&ft)[4], double (&f)[N][3]) {
    double m_liq = 0.0;
#pragma unroll
    for (int m = 0; m < N; ++m) m_liq += u[m][1] * As.norm[3 * m + 1];
    const ParcelThermo x = parcel_thermo(c, t[0], t[1], t[2], t[3], m_liq);
    double nn[N], th[N], kk[N];
#pragma unroll
    for (int m = 0; m < N; ++m) invert_closure(As.dist_type[m], u[m][0], u[m][1], u[m][2], As.kmin, As.kmax, nn[m], th[m], kk[m]);
    cond_evap_parcel<N, P, false>(As, coef0 * x.xi, t[0] - 1.0, nn, th, kk, f);
    double dm_liq = 0.0;
#pragma unroll
    for (int m = 0; m < N; ++m) dm_liq += f[m][1] * As.norm[3 * m + 1];
    const double dq_l = dm_liq / x.rho;
    if constexpr ((SRC & SRC_COAL) != 0) {   // (the condensation term first, as in box_ssprk33_body)
        double acc[N][3];
        coal_ints_parcel<N, P, MODE_ALLINF, false, SPEC>(As, nullptr, nn, th, kk, acc);
#pragma unroll
        for (int m = 0; m < N; ++m) {
            f[m][0] = acc[m][0];  // (condensation leaves the number alone)
            f[m][1] = acc[m][1] + f[m][1];
            f[m][2] = (As.np[m] == 3) ? acc[m][2] + f[m][2] : 0.0;
        }
    }
    ft[0] = x.a1 * w * t[0] - (1.0 / t[3] + x.a3) * t[0] * dq_l;
    ft[1] = -t[1] * c.grav * w / (x.R * t[2]);
    ft[2] = (x.L * dq_l - c.grav * w) / x.cp;
    ft[3] = -dq_l;
}

// n_steps SSPRK33 steps of dY/dt above for one parcel per lane; y has 4 + nmom planes of leading dimension ld: S, p, T, q_v, then
// the plan's moment planes in physical units.  The four thermodynamic values, the moments (normalised units, as in
// box_ssprk33_body with SRC_COND) and their u_prev stay in registers over all stages and steps; the state is read once and
// written once, w is loaded once; the update formulas are OrdinaryDiffEq's, as in ssprk33_body (exact "/ 4", correctly rounded
// "/ 3").  SRC: SRC_COND (any plan: nothing of the coalescence data is read) or SRC_COAL | SRC_COND (tensor plans whose
// thresholds are all Inf).  n_steps = 0 stores what was loaded.
// RHS_ONLY: ONE evaluation of dY, stored in physical units, no update (dt, n_steps unused).
template <int N, int P, typename TIO, bool SPEC, int BS, int SRC, bool RHS_ONLY = false>
__device__ __forceinline__ void parcel_ssprk33_body(const KArgs<N, P> *__restrict__ Ag, const ParcelParams par, size_t n, size_t ld,
                                                    const TIO *y_in, TIO *y_out, double coef0, double w_scalar,
                                                    const double *__restrict__ w_dev, double dt, int n_steps) {
    static_assert((SRC & SRC_COND) != 0 && (SRC & ~(SRC_COAL | SRC_COND)) == 0, "SRC_COND or SRC_COAL | SRC_COND");
    const KArgs<N, P> &A = *Ag;
    const size_t i = (size_t)blockIdx.x * BS + threadIdx.x;
    if (i >= n) return;
    const bool stepping = RHS_ONLY || n_steps > 0;  // (wave-uniform)
    double t[4], tp[4], ft[4], u[N][3], up[N][3], f[N][3];
#pragma unroll
    for (int q = 0; q < 4; ++q) t[q] = (double)y_in[(size_t)q * ld + i];
#pragma unroll
    for (int m = 0; m < N; ++m) {
        const int off = 4 + A.off[m];
        u[m][0] = (double)y_in[(size_t)(off + 0) * ld + i];
        u[m][1] = (double)y_in[(size_t)(off + 1) * ld + i];
        u[m][2] = (A.np[m] == 3) ? (double)y_in[(size_t)(off + 2) * ld + i] : 0.0;
        if (stepping) {
#pragma unroll
            for (int q = 0; q < 3; ++q) u[m][q] = div_by_const(u[m][q], A.norm[3 * m + q], A.inv_norm[3 * m + q]);
        }
    }
    const double w = w_dev ? w_dev[i] : w_scalar;
    if constexpr (RHS_ONLY) {
        parcel_tendency<N, P, SPEC, SRC>(A, par, coef0, w, t, u, ft, f);
#pragma unroll
        for (int q = 0; q < 4; ++q) t[q] = ft[q];
#pragma unroll
        for (int m = 0; m < N; ++m)
#pragma unroll
            for (int q = 0; q < 3; ++q) u[m][q] = f[m][q];
    } else {
#pragma unroll 1
        for (int step = 0; step < n_steps; ++step) {
#pragma unroll
            for (int q = 0; q < 4; ++q) tp[q] = t[q];
#pragma unroll
            for (int m = 0; m < N; ++m)
#pragma unroll
                for (int q = 0; q < 3; ++q) up[m][q] = u[m][q];
#pragma unroll 1
            for (int stage = 0; stage < 3; ++stage) {
                // the plan constants through an opaque zero offset per stage (see ssprk33_body); none when compiled for the plan
                size_t opaque_zero = 0;
                if (!SPEC) asm volatile("" : "+s"(opaque_zero));
                const KArgs<N, P> &As = *(Ag + opaque_zero);
                parcel_tendency<N, P, SPEC, SRC>(As, par, coef0, w, t, u, ft, f);
                // OrdinaryDiffEq SSPRK33: u = uprev + dt k;  u = (3 uprev + u + dt k)/4;  u = (uprev + 2u + 2dt k)/3
                if (stage == 0) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) t[q] = tp[q] + dt * ft[q];
#pragma unroll
                    for (int m = 0; m < N; ++m)
#pragma unroll
                        for (int q = 0; q < 3; ++q) u[m][q] = up[m][q] + dt * f[m][q];
                } else if (stage == 1) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) t[q] = (3.0 * tp[q] + t[q] + dt * ft[q]) * 0.25;  // "/ 4" is exact
#pragma unroll
                    for (int m = 0; m < N; ++m)
#pragma unroll
                        for (int q = 0; q < 3; ++q) u[m][q] = (3.0 * up[m][q] + u[m][q] + dt * f[m][q]) * 0.25;
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)  // "/ 3" as a correctly rounded division
                        t[q] = div_by_const(tp[q] + 2.0 * t[q] + 2.0 * dt * ft[q], 3.0, 1.0 / 3.0);
#pragma unroll
                    for (int m = 0; m < N; ++m)
#pragma unroll
                        for (int q = 0; q < 3; ++q)
                            u[m][q] = div_by_const(up[m][q] + 2.0 * u[m][q] + 2.0 * dt * f[m][q], 3.0, 1.0 / 3.0);
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) y_out[(size_t)q * ld + i] = (TIO)t[q];
#pragma unroll
    for (int m = 0; m < N; ++m) {
        const int off = 4 + A.off[m];
        if (stepping) {
#pragma unroll
            for (int q = 0; q < 3; ++q) u[m][q] *= A.norm[3 * m + q];
        }
        y_out[(size_t)(off + 0) * ld + i] = (TIO)u[m][0];
        y_out[(size_t)(off + 1) * ld + i] = (TIO)u[m][1];
        if (A.np[m] == 3) y_out[(size_t)(off + 2) * ld + i] = (TIO)u[m][2];
    }
}

}  // namespace cloudy
