// adaptive_thermo.hpp -- per-parcel adaptive Tsit5 for the adiabatic parcel (cloudy_parcel_tsit5_adaptive): the loop of the adaptive
// coalescence integrator (tsit5_adaptive_loop: stages, error estimate, controller, FSAL hand-over, snapshots, final store -- nothing
// of it is restated here) on the right-hand side of the fixed-step parcel integrator (parcel_tendency: what a stage of
// parcel_ssprk33_body evaluates),
//   dY/dt of Y = (S, p, T, q_v, mom...),
// the updated-distribution form of test/examples/Analytical/parcel_example.jl with xi(T) formed per evaluation.  The parcel's
// fastest time scale is the relaxation of the supersaturation, about 1 / (4 pi D_vapor N r): 2 s for the driver's N = 2e8, a
// tenth of that at 2e9, and moving as the droplets grow and the supersaturation peaks and relaxes -- a batch whose droplet
// numbers and updraft speeds span a decade each has no common dt that is both safe and cheap.
//
// The four thermodynamic values are the loop's EXTRA state (tsit5_adaptive_loop<..., X = 4>): planes 0 .. 3 of y, unnormalised,
// counted in the error norm with abstol in their own units, snapshotted and interpolated like the moments, which follow in planes
// 4 .. and stay in normalised units between load and store.
//   SRC_COND: any plan, nothing of the coalescence data is read; dM0/dt is zero identically and the number planes come out with
//     the bits they went in with (KEEP0).
//   SRC_COAL | SRC_COND: tensor plans whose thresholds are all Inf; one closure inversion per evaluation feeds both sources.
// Either way a plain per-lane loop without a barrier: a lane leaves when its parcel is done.  The updraft speed is loaded once.
//
// Registers: 4 + 3N doubles per array, ten arrays (twelve with snapshots): 200 (240) VGPRs for N = 2 before any temporary -- one
// wave per SIMD of the 512-register file, which is what the kernels ask for (jit.hpp, parcel_adaptive_kernel).
#pragma once
#include "adaptive.hpp"
#include "parcel.hpp"

namespace cloudy {

template <int N, int P, typename TIO, bool SPEC, int BS, bool SAVE, int SRC>
__device__ __forceinline__ void parcel_tsit5_adaptive_body(const KArgs<N, P> *__restrict__ Ag, const ParcelParams par, size_t n, size_t ld,
                                                           const TIO *y_in, TIO *y_out, double coef0, double w_scalar,
                                                           const double *__restrict__ w_dev, double t_span, AdaptiveOpts o,
                                                           double *dt_dev, double *t_dev, int *info_dev, size_t n_save = 0,
                                                           const double *__restrict__ t_save = nullptr,
                                                           TIO *__restrict__ y_save = nullptr) {
    static_assert((SRC & SRC_COND) != 0 && (SRC & ~(SRC_COAL | SRC_COND)) == 0, "SRC_COND or SRC_COAL | SRC_COND");
    const size_t i = (size_t)blockIdx.x * BS + threadIdx.x;
    const double w = i < n ? (w_dev ? w_dev[i] : w_scalar) : 0.0;
    // the plan constants through an opaque zero offset per evaluation (see ssprk33_body); none when compiled for the plan
    // (condensation alone: the number planes come out as they went in)
    tsit5_adaptive_loop<N, P, TIO, false, BS, SAVE, (SRC & SRC_COAL) == 0, 4>(
        *Ag, adaptive::LaneGroup<BS>(n, ld), ld, y_in, y_out, t_span, o, dt_dev, t_dev, info_dev, n_save, t_save, y_save,
        [&](bool /*live*/, const double (&t)[4], const double (&u)[N][3], double (&ft)[4], double (&f)[N][3]) {
            size_t oz = 0;
            if (!SPEC) asm volatile("" : "+s"(oz));
            parcel_tendency<N, P, SPEC, SRC>(*(Ag + oz), par, coef0, w, t, u, ft, f);
        });
}

}  // namespace cloudy
