// host_plan.hpp -- host-side plan (the CoalescenceData + ODE_parameters of the reference, flattened)
// and the launch request passed to the per-N instantiation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/cloudy_hip.h"
#include "quad.hpp"

namespace cloudy {

struct HostPlan {
    int N = 0, P = 0, nmom = 0;
    int dist_type[CLOUDY_MAX_MODES] = {0}, np[CLOUDY_MAX_MODES] = {0}, off[CLOUDY_MAX_MODES] = {0};
    int finite[CLOUDY_MAX_MODES] = {0}, node_off[CLOUDY_MAX_MODES] = {0}, n_bins[CLOUDY_MAX_MODES] = {0};
    int n_2d[CLOUDY_MAX_MODES] = {0};
    int n_mom_max = 0, threshold_style = 0, nbpl = 15, mode = 0, dtype = 0;  // dtype: the PLANE type (F64 / F32 / F32_FAST)
    bool relaxed = false;  // desc.dtype == CLOUDY_F64_RELAXED: fp64 planes, series / continued fraction stopped at 1e-11
    double thr[CLOUDY_MAX_MODES] = {0};                 // Coalescence.jl:78-84
    double mom_norm[CLOUDY_MAX_MODES][3] = {{0}};       // helper_functions.jl:40-53, per (mode, order)
    double norms[2] = {1, 1};
    double kmin = 0, kmax = 10;
    double c[CLOUDY_MAX_MODES][CLOUDY_MAX_MODES][CLOUDY_MAX_P][CLOUDY_MAX_P] = {{{{0}}}};
    int n_vel = 0;
    double vel[CLOUDY_MAX_VEL][2] = {{0}};              // physical
    double vel_n[CLOUDY_MAX_VEL][2] = {{0}};            // rainshaft_helpers.jl:74-76
    // MovingThreshold: start-value fit of the percentile inversion (kernels.hpp, KArgs::inv_tab)
    double inv_map[2] = {0.0, 0.0}, inv_klo = 0.0;
    double inv_tab[CLOUDY_MAX_MODES][16] = {{0}};
    int device = 0;
    int jit_conv_rounds = 1;  // parcels per lane of the plan-time compiled converged-mode RHS kernel (quad_kernels.hpp: ROUNDS)
    int jit_conv_bs = 0;    // ... of the plan-time compiled converged-mode kernels (NumericalCoalStyle), likewise
    int jit_sorted_bs = 0;  // workgroup size of the plan-time compiled threshold kernels, fixed at plan creation (jit.hpp)
    int force_ppl1 = 0;  // CLOUDY_HIP_PPL1=1: always the one-parcel-per-lane ALLINF kernel (A/B timing)
    double *nodes_dev = nullptr;                        // [n_nodes][kNodeStride]
    int n_nodes = 0;
    double *partial_dev = nullptr;                      // moment_sums workspace
    void *kargs_dev = nullptr;                          // KArgs<N,P> of (moments in, physical out) followed by SediArgs, uploaded at plan creation
    // NumericalCoalStyle plans (quad.hpp): P = 1, no tensors, no thresholds
    int coal_style = 0;                                 // CLOUDY_ANALYTICAL_COAL / CLOUDY_NUMERICAL_COAL
    QArgs q = {};                                       // kernel function (normalised), rule order, start-value table shape
    std::vector<double> qtab;                           // quad_tab_size(q.nq, q.deg) doubles (host copy: the plan-time compiled kernel embeds it)
    double *qtab_dev = nullptr;
};

enum Op {
    OP_COAL = 0, OP_UPDATE_DIST = 1, OP_FINITE_2D = 2, OP_SEDI = 3, OP_SSPRK33 = 4, OP_COND = 5,
    OP_PREPARE = 6 /* plan creation: upload the constant block */, OP_NQ = 7, OP_RAINSHAFT_SSPRK33 = 8, OP_TSIT5 = 9,
    OP_RAINSHAFT_RHS = 10 /* one evaluation of the column right-hand side (cloudy_rainshaft_rhs) */,
    OP_BOX_SSPRK33 = 11 /* fused SSPRK33 steps with the condensation source (cloudy_box_ssprk33_steps, box_sources.hpp) */,
    OP_RAINSHAFT_COND_SSPRK33 = 12 /* the column integrator with the condensation source (cloudy_rainshaft_cond_ssprk33_steps) */,
    OP_RAINSHAFT_COND_RHS = 13 /* one evaluation of the column right-hand side with it (cloudy_rainshaft_cond_rhs) */,
    OP_PARCEL_SSPRK33 = 14 /* fused SSPRK33 steps of the adiabatic parcel (cloudy_parcel_ssprk33_steps, parcel.hpp) */,
    OP_PARCEL_RHS = 15 /* one evaluation of its right-hand side (cloudy_parcel_rhs) */,
    // the adaptive operations: to t_span, and -- n_save > 0 -- with snapshots at the caller's save times (the kernel that saves)
    OP_TSIT5_ADAPTIVE = 16 /* per-parcel adaptive Tsit5 (cloudy_tsit5_adaptive, cloudy_tsit5_adaptive_saveat, adaptive.hpp) */,
    OP_BOX_TSIT5_ADAPTIVE = 17 /* the same with the condensation source (cloudy_box_tsit5_adaptive, adaptive_box.hpp) */,
    OP_PARCEL_TSIT5_ADAPTIVE = 18 /* the same on the adiabatic parcel (cloudy_parcel_tsit5_adaptive, adaptive_thermo.hpp) */,
    OP_RAINSHAFT_TSIT5_ADAPTIVE = 19 /* per-column adaptive Tsit5 of the rainshaft columns (cloudy_rainshaft_tsit5_adaptive[_saveat], adaptive_column.hpp) */,
    OP_MOMENTS = 20 /* moments of every mode at real orders, up to a cutoff or not (cloudy_moments, spectra.hpp) */,
    OP_DENSITY = 21 /* densities of every mode on a grid of masses (cloudy_density) */
};

struct LaunchReq {
    int op;
    int input_kind = 0;    // IN_MOMENTS (0) / IN_PARAMS (1), kernels.hpp
    int physical_out = 1;  // 1: multiply by mom_norms (rhs_coal!), 0: normalised units (get_coal_ints)
    int rainshaft = 0;     // clamp negatives + skip empty cells
    size_t n, ld;
    const void *in;   // planes of the plan's dtype (double, or float for CLOUDY_F32 plans)
    void *out;        // OP_COAL: dmom; OP_UPDATE_DIST: params; OP_FINITE_2D: F (may be null); OP_SEDI: flux; OP_RAINSHAFT_RHS: rhs
    void *out2 = nullptr;  // OP_FINITE_2D: thresholds (may be null); rainshaft OP_COAL: the sedimentation flux (null: not wanted);
                           // OP_RAINSHAFT_RHS: the cell fluxes (work planes)
    hipStream_t stream;
    double dt = 0.0;  // OP_SSPRK33, OP_TSIT5, OP_RAINSHAFT_SSPRK33, OP_BOX_SSPRK33; OP_*TSIT5_ADAPTIVE: t_span
    int n_steps = 0;  // likewise
    double coef = 0.0, s_scalar = 0.0;  // OP_COND, OP_BOX_*, OP_RAINSHAFT_COND_*
    const double *s_dev = nullptr;      // OP_COND, OP_BOX_*, OP_RAINSHAFT_COND_* (optional per-parcel supersaturation)
    int sources = 0;                    // OP_BOX_*, OP_PARCEL_*: CLOUDY_SRC_* bits
    const void *parcel = nullptr;       // OP_PARCEL_*: the ParcelParams (parcel.hpp); coef = coef0, s_scalar / s_dev = w / w_dev
    const void *spectra = nullptr;      // OP_MOMENTS: the MomentArgs; OP_DENSITY: the DensityArgs (spectra.hpp), its grid in s_dev
    const void *adaptive = nullptr;     // OP_*TSIT5_ADAPTIVE: the AdaptiveOpts (adaptive.hpp) ...
    double *dt_dev = nullptr, *t_dev = nullptr;   // ... and its optional per-parcel planes: next dt (in/out), time reached,
    int32_t *info_dev = nullptr;                  // accepted / rejected / status ([3][ld]); OP_RAINSHAFT_TSIT5_ADAPTIVE: per column ([3][n_columns])
    size_t n_save = 0;                  // OP_*TSIT5_ADAPTIVE, > 0: the save times (host; the launch uploads them into the plan's scratch) and,
    const double *t_save = nullptr;     // in `out2`, the snapshot planes
    size_t nz = 0;    // OP_RAINSHAFT_*: cells per column (n = nz * n_columns)
    double dz = 0.0;  // OP_RAINSHAFT_*
    LaunchReq(int op_, size_t n_, size_t ld_, const void *in_, void *out_, void *stream_)
        : op(op_), n(n_), ld(ld_), in(in_), out(out_), stream(static_cast<hipStream_t>(stream_)) {}
};

// Parcels per lane of the all-Inf RHS kernels (ahead-of-time launch_io() and the plan's main unit alike): 4 where the plan has
// the packed single-precision kernel (CLOUDY_F32_FAST, for every layout: the arithmetic is a property of the plan, not of the
// batch's alignment), 2 where both planes allow 2-element accesses, else 1 (CLOUDY_HIP_PPL1=1: always 1).  esz: bytes per
// plane element.
inline int allinf_parcels_per_lane(const HostPlan &h, const LaunchReq &r, size_t esz, bool packed4) {
    if (h.force_ppl1) return 1;
    if (packed4) return 4;
    const uintptr_t amask = 2 * esz - 1;
    const bool aligned2 = ((reinterpret_cast<uintptr_t>(r.in) | reinterpret_cast<uintptr_t>(r.out)) & amask) == 0 && r.ld % 2 == 0;
    return aligned2 ? 2 : 1;
}

// every kernel family of one (N, P), explicitly instantiated one per unit (inst.hip -> inst_n<N>_p<P>.o) so that the families
// compile in parallel
template <int N, int P>
hipError_t launch_np(const HostPlan &h, const LaunchReq &r);
// the fused integrators (cloudy_ssprk33_steps, cloudy_rainshaft_ssprk33_steps) live in their own units
// (int.hip -> int_n<N>_p<P>.o), compiled with machine LICM off: see launch_int_impl.hpp
template <int N, int P>
hipError_t launch_int(const HostPlan &h, const LaunchReq &r);
// cloudy_coal_rhs / cloudy_get_coal_ints of a NumericalCoalStyle plan, ahead-of-time kernels (quad.hip -> quad_n<N>.o)
hipError_t launch_quad_n1(const HostPlan &h, const LaunchReq &r);
hipError_t launch_quad_n2(const HostPlan &h, const LaunchReq &r);
hipError_t launch_quad_n3(const HostPlan &h, const LaunchReq &r);
hipError_t launch_quad_n4(const HostPlan &h, const LaunchReq &r);

}  // namespace cloudy
