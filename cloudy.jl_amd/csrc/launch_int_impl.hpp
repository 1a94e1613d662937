// launch_int_impl.hpp -- the fused on-device integrators of one (N, P) family.  Included only by int.hip, which the
// Makefile compiles once per family (int_n<N>_p<P>.o) with `-mllvm -disable-machine-licm`: the step/stage loops of
// these kernels wrap the whole right-hand side, and machine LICM hoists every literal of the libm polynomials (exp,
// log, lgamma) and of the series out of them into registers for the life of the kernel -- 256 VGPRs, occupancy 1 and
// spills, against 108-170 VGPRs without (measured on MI355X: cloudy_ssprk33_steps on the cfg3b batch 1.12 -> 0.53 ms
// per RHS evaluation per 1e6 parcels, the rainshaft column integrator 1.53 -> 0.78).  The single-pass kernels of
// inst.hip keep LICM: their Simpson node loops gain from the hoisting (cfg3b, at the time: 4.85 ms with, 4.96 ms
// without).
#pragma once
#include "launch_impl.hpp"

namespace cloudy {

template <int N, int P, typename TIO>
hipError_t launch_int_io(const HostPlan &h, const LaunchReq &r) {
    if (!h.kargs_dev) return hipErrorNotInitialized;  // uploaded by OP_PREPARE at plan creation
    const KArgs<N, P> *Ad = static_cast<const KArgs<N, P> *>(h.kargs_dev);
    const TIO *in = static_cast<const TIO *>(r.in);
    TIO *out = static_cast<TIO *>(r.out);
    switch (r.op) {
    case OP_SSPRK33:
        return pick<MODE_MOVING, MODE_FIXED, MODE_ALLINF>(h.mode, [&](auto M) {
            return pick<kBlock, 512>(sorted_block_size(h), [&](auto BS) {
                if constexpr (!sorted_block_exists<N, M, BS>) return hipErrorInvalidValue;
                else {
                    hipLaunchKernelGGL((ssprk33_kernel<N, P, M, TIO, BS>), dim3(grid_for(r.n, BS)), dim3(BS), 0, r.stream, Ad,
                                       h.nodes_dev, r.n, r.ld, in, out, r.dt, r.n_steps);
                    return hipGetLastError();
                }
            });
        });
    case OP_TSIT5:  // cloudy_tsit5_steps: thresholds Inf, fixed or moving; fp64 or float planes
        return pick<MODE_MOVING, MODE_FIXED, MODE_ALLINF>(h.mode, [&](auto M) {
            hipLaunchKernelGGL((tsit5_kernel<N, P, M, TIO>), dim3(grid_for(r.n)), dim3(kBlock), 0, r.stream, Ad, h.nodes_dev, r.n,
                               r.ld, in, out, r.dt, r.n_steps);
            return hipGetLastError();
        });
    case OP_RAINSHAFT_SSPRK33: {
        if (r.nz < 1 || r.nz > (size_t)kBlock) return hipErrorInvalidValue;
        const size_t cpb = kRainshaftBlock / r.nz, n_columns = r.n / r.nz;
        // make_rainshaft_rhs is FixedThreshold only (rainshaft_helpers.jl:70): no MovingThreshold kernel
        return pick<MODE_FIXED, MODE_ALLINF>(h.mode, [&](auto M) {
            hipLaunchKernelGGL((rainshaft_ssprk33_kernel<N, P, M, TIO>), dim3(grid_for(n_columns, cpb)), dim3(kRainshaftBlock), 0,
                               r.stream, Ad, h.nodes_dev, (int)r.nz, n_columns, r.ld, in, out, r.dt, r.dz, r.n_steps);
            return hipGetLastError();
        });
    }
    default: return hipErrorInvalidValue;
    }
}

template <int N, int P>
hipError_t launch_int(const HostPlan &h, const LaunchReq &r) {
    if (h.dtype != CLOUDY_F64) return launch_int_io<N, P, float>(h, r);
    return launch_int_io<N, P, double>(h, r);
}

}  // namespace cloudy
