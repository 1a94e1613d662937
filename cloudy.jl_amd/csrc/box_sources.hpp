// box_sources.hpp -- the fused SSPRK33 box integrator with the condensation source (cloudy_box_ssprk33_steps).
//
// The reference's box drivers integrate du/dt = rhs!(u) with SSPRK33 and a fixed dt; rhs! is rhs_coal! (kernels.hpp:
// ssprk33_body), rhs_condensation! (test/examples/utils/box_model_helpers.jl:55-67 -> get_cond_evap,
// src/Sources/Condensation.jl:22-37; the drivers test/examples/Analytical/condensation_single_gamma.jl:28 and
// condensation_exp_gamma.jl:31), or -- in a host model that carries both processes -- their sum.  Stepped stage by stage the sum
// costs two right-hand-side launches and an update launch per stage, seven passes over the state; here a lane keeps its parcel in
// registers over all stages and steps as in ssprk33_body, and ONE closure inversion per stage feeds both sources.
//
// The body here calls the per-parcel device functions of kernels.hpp (invert_closure, coal_ints_parcel, coal_ints_ranked_impl,
// cond_evap_parcel -- which the column integrator with the condensation source shares -- and div_by_const).
#pragma once
#include "kernels.hpp"

namespace cloudy {

#ifndef CLOUDY_SRC_BITS   // (parcel.hpp defines the same two)
#define CLOUDY_SRC_BITS
enum { SRC_COAL = 1, SRC_COND = 2 };  // CLOUDY_SRC_* of include/cloudy_hip.h
#endif

// One evaluation of the box's right-hand side for the lane's parcel, f = [coal](u) + [cond](u; sv) by SRC as above: what a stage
// of box_ssprk33_body and a stage of the adaptive loop (adaptive_box.hpp) both call.  u and f are in the units the instance keeps
// its state in: physical where the parcels are ranked (SRC_COAL with a threshold), normalised otherwise.  Ranked: every lane of the
// workgroup calls it (coal_ints_ranked_impl's barriers), `valid` = the lane's result is wanted; the condensation term sits
// after the barriers.  Otherwise nodes and valid are not read.
template <int N, int P, int MODE, bool SPEC, int BS, int SRC>
__device__ __forceinline__ void box_rhs(const KArgs<N, P> &As, const double *__restrict__ nodes, bool valid, double coef, double sv,
                                        const double (&u)[N][3], double (&f)[N][3]) {
    static_assert((SRC & SRC_COND) != 0 && (SRC & ~(SRC_COAL | SRC_COND)) == 0, "SRC_COND or SRC_COAL | SRC_COND");
    constexpr bool kCoal = (SRC & SRC_COAL) != 0;
    constexpr bool kRanked = kCoal && MODE != MODE_ALLINF;
    double nn[N], th[N], kk[N];
#pragma unroll
    for (int m = 0; m < N; ++m) {
        if (!kRanked) {
            invert_closure(As.dist_type[m], u[m][0], u[m][1], u[m][2], As.kmin, As.kmax, nn[m], th[m], kk[m]);
        } else {
            const double m0 = div_by_const(u[m][0], As.norm[3 * m + 0], As.inv_norm[3 * m + 0]);
            const double m1 = div_by_const(u[m][1], As.norm[3 * m + 1], As.inv_norm[3 * m + 1]);
            const double m2 = div_by_const(u[m][2], As.norm[3 * m + 2], As.inv_norm[3 * m + 2]);
            invert_closure(As.dist_type[m], m0, m1, m2, As.kmin, As.kmax, nn[m], th[m], kk[m]);
        }
    }
    if constexpr (!kCoal) {
        cond_evap_parcel<N, P, false>(As, coef, sv, nn, th, kk, f);
    } else if constexpr (!kRanked) {
        // (the condensation term first: its 2N values are fewer to keep across the tensor contractions than the
        // 3N closure parameters)
        double fc[N][3], acc[N][3];
        cond_evap_parcel<N, P, false>(As, coef, sv, nn, th, kk, fc);
        coal_ints_parcel<N, P, MODE_ALLINF, false, SPEC>(As, nullptr, nn, th, kk, acc);
#pragma unroll
        for (int m = 0; m < N; ++m) {
            f[m][0] = acc[m][0];  // (condensation leaves the number alone)
            f[m][1] = acc[m][1] + fc[m][1];
            f[m][2] = (As.np[m] == 3) ? acc[m][2] + fc[m][2] : 0.0;
        }
    } else {
        double fc[N][3], acc[N][3];
        double (*rows)[BS];
        coal_ints_ranked_impl<N, P, MODE, SPEC, BS, true>(As, nodes, valid, nn, th, kk, acc, rows);
        cond_evap_parcel<N, P, true>(As, coef, sv, nn, th, kk, fc);  // (n, theta, k) as the ranking's LDS rows hold them
#pragma unroll
        for (int m = 0; m < N; ++m) {
            f[m][0] = acc[m][0] * As.out_scale[3 * m + 0];
            f[m][1] = acc[m][1] * As.out_scale[3 * m + 1] + fc[m][1];
            f[m][2] = (As.np[m] == 3) ? acc[m][2] * As.out_scale[3 * m + 2] + fc[m][2] : 0.0;
        }
    }
}

// n_steps SSPRK33 steps of du/dt = [coal](u) + [cond](u; s) for one parcel per lane; SRC: SRC_COND or SRC_COAL | SRC_COND
// (coalescence alone is ssprk33_body).  State and u_prev stay in registers over all stages and steps, the state is read once
// and written once, the parcel's supersaturation is loaded once; the update formulas are OrdinaryDiffEq's, as in ssprk33_body.
//   SRC_COND: closure inversion + cond_evap_parcel per stage.  No Simpson pass is involved, so the state is kept in normalised
//     units (see rhs_normalised) whatever the plan's thresholds are, and nothing of the coalescence data is read.
//   SRC_COAL | SRC_COND, thresholds all Inf: one inversion per stage feeds both sources; normalised state.
//   SRC_COAL | SRC_COND, fixed or moving thresholds: the workgroup re-ranks its parcels in every stage (coal_ints_ranked_impl),
//     so lanes without a parcel stay for the barriers; the state is physical as in rhs_physical.  The condensation term is formed
//     AFTER the Simpson passes, for the lane's own parcel, from the (n, theta, k) the ranking hands back out of its LDS rows:
//     nothing of it is live across the passes.
// n_steps = 0 stores what was loaded (no round trip through the normalised units).  BS: workgroup size, as ssprk33_body.
template <int N, int P, int MODE, typename TIO, bool SPEC, int BS, int SRC>
__device__ __forceinline__ void box_ssprk33_body(const KArgs<N, P> *__restrict__ Ag, const double *__restrict__ nodes, size_t n,
                                                 size_t ld, const TIO *u_in, TIO *u_out, double coef, double s_scalar,
                                                 const double *__restrict__ s_dev, double dt, int n_steps) {
    static_assert((SRC & SRC_COND) != 0 && (SRC & ~(SRC_COAL | SRC_COND)) == 0, "SRC_COND or SRC_COAL | SRC_COND");
    constexpr bool kCoal = (SRC & SRC_COAL) != 0;
    constexpr bool kRanked = kCoal && MODE != MODE_ALLINF;
    constexpr bool kNormalisedState = !kRanked;
    const KArgs<N, P> &A = *Ag;
    const size_t i = (size_t)blockIdx.x * BS + threadIdx.x;
    const bool valid = i < n;
    if (!kRanked && !valid) return;
    const bool stepping = n_steps > 0;  // (wave-uniform)
    double u[N][3], up[N][3], f[N][3];
#pragma unroll
    for (int m = 0; m < N; ++m) {
        const int off = A.off[m];
        u[m][0] = valid ? (double)u_in[(size_t)(off + 0) * ld + i] : 0.0;
        u[m][1] = valid ? (double)u_in[(size_t)(off + 1) * ld + i] : 0.0;
        u[m][2] = (valid && A.np[m] == 3) ? (double)u_in[(size_t)(off + 2) * ld + i] : 0.0;
        if (kNormalisedState && stepping) {
#pragma unroll
            for (int q = 0; q < 3; ++q) u[m][q] = div_by_const(u[m][q], A.norm[3 * m + q], A.inv_norm[3 * m + q]);
        }
    }
    const double sv = valid ? (s_dev ? s_dev[i] : s_scalar) : 0.0;
#pragma unroll 1
    for (int step = 0; step < n_steps; ++step) {
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
            box_rhs<N, P, MODE, SPEC, BS, SRC>(As, nodes, valid, coef, sv, u, f);
            // OrdinaryDiffEq SSPRK33: u = uprev + dt k;  u = (3 uprev + u + dt k)/4;  u = (uprev + 2u + 2dt k)/3
            if (stage == 0) {
#pragma unroll
                for (int m = 0; m < N; ++m)
#pragma unroll
                    for (int q = 0; q < 3; ++q) u[m][q] = up[m][q] + dt * f[m][q];
            } else if (stage == 1) {
#pragma unroll
                for (int m = 0; m < N; ++m)
#pragma unroll
                    for (int q = 0; q < 3; ++q) u[m][q] = (3.0 * up[m][q] + u[m][q] + dt * f[m][q]) * 0.25;  // "/ 4" is exact
            } else {
#pragma unroll
                for (int m = 0; m < N; ++m)
#pragma unroll
                    for (int q = 0; q < 3; ++q)  // "/ 3" as a correctly rounded division
                        u[m][q] = div_by_const(up[m][q] + 2.0 * u[m][q] + 2.0 * dt * f[m][q], 3.0, 1.0 / 3.0);
            }
        }
    }
    if (!valid) return;
#pragma unroll
    for (int m = 0; m < N; ++m) {
        const int off = A.off[m];
        if (kNormalisedState && stepping) {
#pragma unroll
            for (int q = 0; q < 3; ++q) u[m][q] *= A.norm[3 * m + q];
        }
        u_out[(size_t)(off + 0) * ld + i] = (TIO)u[m][0];
        u_out[(size_t)(off + 1) * ld + i] = (TIO)u[m][1];
        if (A.np[m] == 3) u_out[(size_t)(off + 2) * ld + i] = (TIO)u[m][2];
    }
}

}  // namespace cloudy
