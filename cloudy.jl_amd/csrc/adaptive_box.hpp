// adaptive_box.hpp -- per-parcel adaptive Tsit5 for boxes with condensation (cloudy_box_tsit5_adaptive): the loop of adaptive.hpp
// (tsit5_adaptive_loop: stages, error estimate, controller, FSAL hand-over, snapshots, final store -- nothing of it is restated
// here) on the right-hand side of box_sources.hpp (box_rhs: what a stage of box_ssprk33_body evaluates),
//   du/dt = [coal](u) + [cond](u; s, xi),
// rhs_coal! + rhs_condensation! of the reference (test/examples/utils/box_model_helpers.jl:29-53 and :55-67 -> get_cond_evap,
// src/Sources/Condensation.jl:22-37).  Condensation is the source whose time scale differs most from parcel to parcel -- the
// supersaturation is a per-parcel input of either sign, and x^(2/3) of an evaporating mode falls linearly in t -- which is
// what a controller per parcel is for.
//
//   SRC_COND: closure inversion + cond_evap_parcel per evaluation, for any plan: a plain per-lane loop without a barrier, the
//     state in normalised units whatever the plan's thresholds are; nothing of the coalescence data is read.
//   SRC_COAL | SRC_COND, thresholds all Inf: one inversion per evaluation feeds both sources; per-lane loop, normalised state.
//   SRC_COAL | SRC_COND, fixed or moving thresholds: the workgroup re-ranks its parcels in every evaluation
//     (coal_ints_ranked_impl), so every lane makes the same sequence of evaluations, the loop runs while any lane of the
//     workgroup is active, and a lane without a parcel or with a finished one passes valid = false; the state is physical.  The
//     condensation term is formed after the ranking's barriers from the (n, theta, k) the ranking hands back.
// The parcel's supersaturation is loaded once.  Coalescence alone is tsit5_adaptive_body.
#pragma once
#include "adaptive.hpp"
#include "box_sources.hpp"

namespace cloudy {

template <int N, int P, int MODE, typename TIO, bool SPEC, int BS, bool SAVE, int SRC>
__device__ __forceinline__ void box_tsit5_adaptive_body(const KArgs<N, P> *__restrict__ Ag, const double *__restrict__ nodes, size_t n,
                                                        size_t ld, const TIO *u_in, TIO *u_out, double coef, double s_scalar,
                                                        const double *__restrict__ s_dev, double t_span, AdaptiveOpts o,
                                                        double *dt_dev, double *t_dev, int *info_dev, size_t n_save = 0,
                                                        const double *__restrict__ t_save = nullptr,
                                                        TIO *__restrict__ u_save = nullptr) {
    constexpr bool kRanked = (SRC & SRC_COAL) != 0 && MODE != MODE_ALLINF;
    const size_t i = (size_t)blockIdx.x * BS + threadIdx.x;
    const double sv = i < n ? (s_dev ? s_dev[i] : s_scalar) : 0.0;
    // the plan constants through an opaque zero offset per evaluation (see ssprk33_body); none when compiled for the plan
    // (condensation alone: the number planes come out as they went in)
    tsit5_adaptive_loop<N, P, TIO, kRanked, BS, SAVE, (SRC & SRC_COAL) == 0>(
        *Ag, adaptive::LaneGroup<BS>(n, ld), ld, u_in, u_out, t_span, o, dt_dev, t_dev, info_dev, n_save, t_save, u_save,
        [&](bool live, const double (&state)[N][3], double (&deriv)[N][3]) {
            size_t oz = 0;
            if (!SPEC) asm volatile("" : "+s"(oz));
            box_rhs<N, P, MODE, SPEC, BS, SRC>(*(Ag + oz), nodes, live, coef, sv, state, deriv);
        });
}

}  // namespace cloudy
