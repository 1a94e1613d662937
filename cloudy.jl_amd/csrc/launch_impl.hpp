// launch_impl.hpp -- fills KArgs<N,P> from the host plan and launches the kernels of one (N, P) family (all modes).
// Included by inst.hip, compiled once per family (inst_n<N>_p<P>.o) so that the instantiations compile in parallel.
#pragma once
#include <type_traits>

#include "host_plan.hpp"
#include "kernels.hpp"

namespace cloudy {

// workgroups for n items, per_wg of them per workgroup (one parcel per lane by default: see kernels.hpp)
inline unsigned grid_for(size_t n, size_t per_wg = kBlock) {
    size_t blocks = (n + per_wg - 1) / per_wg;
    if (blocks < 1) blocks = 1;
    return (unsigned)blocks;
}

// Calls f(std::integral_constant<T, V>{}) for the one V of Vs equal to the run-time value v (none: hipErrorInvalidValue), so
// that the launch of a kernel family is written once and instantiated for the listed values only.  The kernels one pick()
// instantiates land in the code object in the reverse order of Vs, and that order changes the code generated for kernels that
// share device functions: the value lists below run backwards, which keeps every unit's kernels, and their code, in the order of
// the launch ladders they replace.
template <auto... Vs, typename T, typename F>
auto pick(T v, F &&f) {
    hipError_t e = hipErrorInvalidValue;
    (void)((v == Vs && (e = f(std::integral_constant<decltype(Vs), Vs>{}), true)) || ...);
    return e;
}

template <int N, int P>
void fill_args(const HostPlan &h, const LaunchReq &r, KArgs<N, P> &A) {
    for (int i = 0; i < N; ++i) {
        A.dist_type[i] = h.dist_type[i];
        A.np[i] = h.np[i];
        A.off[i] = h.off[i];
        A.finite[i] = h.finite[i];
        A.node_off[i] = h.node_off[i];
        A.n_bins[i] = h.n_bins[i];
        A.n_2d[i] = h.n_2d[i];
        A.thr[i] = h.thr[i];
        for (int m = 0; m < 3; ++m) {
            A.norm[3 * i + m] = h.mom_norm[i][m];
            A.inv_norm[3 * i + m] = 1.0 / h.mom_norm[i][m];
            A.out_scale[3 * i + m] = r.physical_out ? h.mom_norm[i][m] : 1.0;
        }
    }
    A.n_mom_max = h.n_mom_max;
    A.input_kind = r.input_kind;
    A.rainshaft = r.rainshaft;
    A.nbpl = h.nbpl;
    A.kmin = h.kmin;
    A.kmax = h.kmax;
    for (int j = 0; j < N; ++j)
        for (int k = 0; k < N; ++k)
            for (int a = 0; a < P; ++a)
                for (int b = 0; b < P; ++b) A.c[j][k][a][b] = h.c[j][k][a][b];
    static_assert(kInvTerms == 16, "HostPlan::inv_tab holds 16 coefficients per mode");
    A.inv_map[0] = h.inv_map[0];
    A.inv_map[1] = h.inv_map[1];
    A.inv_klo = h.inv_klo;
    for (int i = 0; i < N; ++i)
        for (int d = 0; d < kInvTerms; ++d) A.inv_tab[i][d] = h.inv_tab[i][d];
}

// workgroup size of the threshold kernel for a plan (see coal_rhs_sorted_kernel in kernels.hpp)
inline int sorted_block_size(const HostPlan &h) {
    if (h.mode != MODE_FIXED || h.N > 2) return kBlock;
    int passes = 0;
    for (int i = 0; i < h.N - 1; ++i) passes += h.finite[i] ? 1 : 0;
    return passes == 1 ? 512 : kBlock;
}
// the workgroup sizes of the threshold kernels of mode M: 512 threads for MODE_FIXED plans of N <= 2 only
template <int N, int M, int BS>
constexpr bool sorted_block_exists = BS == kBlock || (N <= 2 && M == MODE_FIXED);

inline void fill_sedi(const HostPlan &h, SediArgs &S) {
    S.n_vel = h.n_vel;
    S.pad = 0;
    for (int v = 0; v < 4; ++v) {
        S.vel[v][0] = v < h.n_vel ? h.vel_n[v][0] : 0.0;
        S.vel[v][1] = v < h.n_vel ? h.vel_n[v][1] : 0.0;
    }
}

// kernels that exist for both plane types (double / float storage)
template <int N, int P, typename TIO>
hipError_t launch_io(const HostPlan &h, const LaunchReq &r, const KArgs<N, P> &A) {
    const TIO *in = static_cast<const TIO *>(r.in);
    TIO *out = static_cast<TIO *>(r.out);
    switch (r.op) {
    case OP_COAL: {
        if (h.mode == MODE_ALLINF) {
            if (r.input_kind == IN_MOMENTS && !r.rainshaft && allinf_parcels_per_lane(h, r, sizeof(TIO), false) == 2)
                hipLaunchKernelGGL((coal_rhs_allinf2_kernel<N, P, TIO>), dim3(grid_for(r.n, 2 * kBlock)), dim3(kBlock), 0, r.stream,
                                   A, r.n, r.ld, in, out);
            else
                hipLaunchKernelGGL((coal_rhs_kernel<N, P, MODE_ALLINF, TIO>), dim3(grid_for(r.n)), dim3(kBlock), 0, r.stream, A,
                                   h.nodes_dev, r.n, r.ld, in, out);
            break;
        }
        const bool fast = h.dtype == CLOUDY_F32_FAST && sizeof(TIO) == 4 && r.input_kind == IN_MOMENTS;
        return pick<kBlock, 512>(sorted_block_size(h), [&](auto BS) {
            return pick<false, true>(fast, [&](auto FAST) {
                return pick<MODE_MOVING, MODE_FIXED>(h.mode, [&](auto M) {
                    if constexpr (!sorted_block_exists<N, M, BS>) return hipErrorInvalidValue;
                    else {
                        hipLaunchKernelGGL((coal_rhs_sorted_kernel<N, P, M, TIO, FAST, BS>), dim3(grid_for(r.n, BS)), dim3(BS), 0,
                                           r.stream, A, h.nodes_dev, r.n, r.ld, in, out);
                        return hipGetLastError();
                    }
                });
            });
        });
    }
    case OP_SEDI: {
        SediArgs S;
        fill_sedi(h, S);
        hipLaunchKernelGGL((sedi_flux_kernel<N, P, TIO>), dim3(grid_for(r.n)), dim3(kBlock), 0, r.stream, A, S, r.n, r.ld, in, out);
        break;
    }
    case OP_NQ:  // r.s_scalar = size cutoff in physical mass units
        hipLaunchKernelGGL((standard_nq_kernel<N, P, TIO>), dim3(grid_for(r.n)), dim3(kBlock), 0, r.stream, A,
                           r.s_scalar / h.norms[1], h.norms[0], h.norms[1], r.n, r.ld, in, out);
        break;
    case OP_COND:
        hipLaunchKernelGGL((cond_evap_kernel<N, P, TIO>), dim3(grid_for(r.n)), dim3(kBlock), 0, r.stream, A,
                           r.coef, r.s_scalar, r.s_dev, r.n, r.ld, in, out);
        break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <int N, int P>
hipError_t launch_np(const HostPlan &h, const LaunchReq &r) {
    KArgs<N, P> A;
    fill_args<N, P>(h, r, A);
    switch (r.op) {
    case OP_PREPARE: {  // constant block in device memory for the fused integrators (moments in, physical units out)
        struct Block {  // SediArgs directly behind KArgs: rainshaft_ssprk33_kernel reads it at (Ag + 1)
            KArgs<N, P> A;
            SediArgs S;
        } blk;
        static_assert(sizeof(KArgs<N, P>) % 8 == 0 && offsetof(Block, S) == sizeof(KArgs<N, P>), "block layout");
        blk.A = A;
        fill_sedi(h, blk.S);
        void *dev = nullptr;
        hipError_t e = hipMalloc(&dev, sizeof(blk));
        if (e != hipSuccess) return e;
        e = hipMemcpy(dev, &blk, sizeof(blk), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(dev);
            return e;
        }
        *static_cast<void **>(r.out) = dev;
        return hipSuccess;
    }
    case OP_SSPRK33:
    case OP_TSIT5:
    case OP_RAINSHAFT_SSPRK33:
        return launch_int<N, P>(h, r);  // int.hip (int_n<N>_p<P>.o)
    case OP_COAL:
    case OP_SEDI:
    case OP_COND:
    case OP_NQ:
        // get_coal_ints on (n, theta, k) planes is an fp64 interface for every plan
        if (h.dtype != CLOUDY_F64 && r.input_kind == IN_MOMENTS) return launch_io<N, P, float>(h, r, A);
        return launch_io<N, P, double>(h, r, A);
    case OP_UPDATE_DIST:
        hipLaunchKernelGGL((update_dist_kernel<N, P>), dim3(grid_for(r.n)), dim3(kBlock), 0, r.stream, A, r.n, r.ld,
                           static_cast<const double *>(r.in), static_cast<double *>(r.out));
        break;
    case OP_FINITE_2D:
        return pick<MODE_MOVING, MODE_FIXED, MODE_ALLINF>(h.mode, [&](auto M) {
            hipLaunchKernelGGL((finite_2d_kernel<N, P, M>), dim3(grid_for(r.n)), dim3(kBlock), 0, r.stream, A, h.nodes_dev, r.n,
                               r.ld, static_cast<const double *>(r.in), static_cast<double *>(r.out), static_cast<double *>(r.out2));
            return hipGetLastError();
        });
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace cloudy
