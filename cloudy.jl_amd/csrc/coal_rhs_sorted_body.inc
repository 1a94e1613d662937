// body of coal_rhs_sorted_kernel / coal_rhs_sorted_body (kernels.hpp): in scope A, nodes, n, ld, in, out, sedi, out2;
// CLOUDY_SPEC, CLOUDY_BS (workgroup size)
//
// Phase 0: every lane loads and inverts its own parcel (n, theta, k of all modes -> LDS).
// Phase 1, once per mode that runs a Simpson pass: the workgroup ranks its parcels (256 or 512) by THAT mode's regime, lane t
//          integrates the mode of the parcel of rank t and leaves the three promoted amounts T_m in the parcel's LDS
//          slot.  (One ranking per mode: with several thresholded modes a single permutation only makes the waves
//          homogeneous for the mode it was built on -- 58 % active lanes on cfg4, 3 thresholds on the 4-mode moving
//          example -- and the pass needs none of the other modes' parameters or partial sums in registers.)
// Phase 2: every lane is back on its own parcel: moments, pair terms, plus the T_m from LDS; coalesced stores.
    constexpr int M_ = P + 2;
    __shared__ double sh_par[3 * N][CLOUDY_BS];
    __shared__ double sh_T[(N > 1 ? N - 1 : 1) * 3][CLOUDY_BS];
    __shared__ unsigned int sh_cnt[CLOUDY_BS];
    __shared__ unsigned short sh_perm[CLOUDY_BS];
    bool all_small = true;
    double nn[N], th[N], kk[N];
    const int t0 = threadIdx.x;
    if ((size_t)blockIdx.x * CLOUDY_BS + t0 < n) {
        all_small = load_parcel<N, P, TIO>(A, (size_t)blockIdx.x * CLOUDY_BS + t0, ld, in, nn, th, kk);
    } else {
#pragma unroll
        for (int m = 0; m < N; ++m) {
            nn[m] = 0.0;
            th[m] = 1.0;
            kk[m] = 1.0;
        }
    }
#pragma unroll
    for (int m = 0; m < N; ++m) {
        sh_par[3 * m + 0][t0] = nn[m];
        sh_par[3 * m + 1][t0] = th[m];
        sh_par[3 * m + 2][t0] = kk[m];
    }
#pragma unroll
    for (int k = 0; k < N - 1; ++k) {
        if (!mode_has_pass<N, P, MODE>(A, k)) continue;  // wave-uniform
        // Which branch a Simpson node takes depends on (x_t / theta) / (a_top + 1) of the parcel; how many terms its
        // series or continued fraction needs, on z0 = x_t / theta itself: ranking by z0 measured 3 % (fp64) to 5 % (fp32
        // pass) faster than ranking by the ratio.  For a moving threshold z0 = P^-1(k; p) is a monotone function of k
        // -> rank by k.  (Ranking moving-threshold parcels by the node count of their grid first -- 75 to ~150 with
        // x_t -- and k second was measured: 4 % slower; ranking fixed-threshold parcels by max(z0, c (k + P)), which sets
        // the number of late nodes since the early group ends at min(3 theta, 1.5 x_t / (a_top - 1)): 0 to 17 % slower.)
        // Nothing but the pass's own operands stays in registers across it: the lane index goes through an opaque copy per
        // pass (LDS addresses are re-derived instead of kept), own parameters come from the lane's LDS slot, and the
        // rank's parcel index and its n are read again after the pass (cfg4, P = 5: these were the last spilled VGPRs).
        int tk = threadIdx.x;
        asm volatile("" : "+v"(tk));
        const double th_own = sh_par[3 * k + 1][tk], kk_own = sh_par[3 * k + 2][tk], nn_own = sh_par[3 * k + 0][tk];
        const float r = (MODE == MODE_FIXED) ? (float)(A.thr[k] / th_own) : (float)kk_own;
        regime_rank<CLOUDY_BS>(nn_own > 0.0 && r == r, regime_bucket<CLOUDY_BS>(r), sh_cnt, sh_perm);
        double msh[M_ * (M_ + 1) / 2];
        PromotedFlags pf;
        {
            const int src = sh_perm[tk];
            pf = promoted_pass<N, P, MODE, FAST>(A, nodes, k, sh_par[3 * k + 0][src] > 0.0, sh_par[3 * k + 1][src],
                                                 sh_par[3 * k + 2][src], msh);
        }
        int tf = threadIdx.x;
        asm volatile("" : "+v"(tf));
        const int src = sh_perm[tf];
        const double n_s = sh_par[3 * k + 0][src], th_s = sh_par[3 * k + 1][src], kk_s = sh_par[3 * k + 2][src];
        double Mk[M_], T0, T1, T2;
        moment_row<M_>(A.dist_type[k], n_s, th_s, kk_s, A.n_mom_max, Mk);
        promoted_finish<N, P>(A, k, n_s, kk_s, Mk, pf, msh, T0, T1, T2);
        sh_T[3 * k + 0][src] = T0;
        sh_T[3 * k + 1][src] = T1;
        sh_T[3 * k + 2][src] = T2;
        __syncthreads();
    }
    int t = threadIdx.x;  // (opaque again: the parcel index and the LDS addresses are re-derived, not kept across the passes)
    asm volatile("" : "+v"(t));
    const size_t i = (size_t)blockIdx.x * CLOUDY_BS + t;
    if (i < n) {
        // the lane's own (n, theta, k) come back from its LDS slots: held in registers across the Simpson passes they
        // were the registers the P = 5 families spilled (18-31 VGPRs to scratch: 2.4x the algorithmic HBM traffic)
        double nn2[N], th2[N], kk2[N];
#pragma unroll
        for (int m = 0; m < N; ++m) {
            nn2[m] = sh_par[3 * m + 0][t];
            th2[m] = sh_par[3 * m + 1][t];
            kk2[m] = sh_par[3 * m + 2][t];
        }
        if (sedi != nullptr && out2 != nullptr) {
            // cloudy_rainshaft_sources: the sedimentation flux of the cell (get_sedimentation_flux, Sedimentation.jl:22-37)
            // from the same (n, theta, k) -- one launch, one read of the moments, one closure inversion for both sources
            double fl[N][3];
            sedi_flux_parcel<N>(A.dist_type, *sedi, nn2, th2, kk2, fl);
#pragma unroll
            for (int m = 0; m < N; ++m)
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    if (q < A.np[m]) st_stream(out2 + (size_t)(A.off[m] + q) * ld + i, fl[m][q] * A.out_scale[3 * m + q]);
        }
        double Mm[N][M_], acc[N][3];
#pragma unroll
        for (int m = 0; m < N; ++m) moment_row<M_>(A.dist_type[m], nn2[m], th2[m], kk2[m], A.n_mom_max, Mm[m]);
#pragma unroll
        for (int k = 0; k < N; ++k) acc[k][0] = acc[k][1] = acc[k][2] = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k) {
            double T0, T1, T2;
            if (k < N - 1 && mode_has_pass<N, P, MODE>(A, k)) {
                T0 = sh_T[3 * k + 0][t];
                T1 = sh_T[3 * k + 1][t];
                T2 = sh_T[3 * k + 2][t];
            } else {  // no threshold on this mode: only the (rare) M_p M_q < eps rule can promote anything
                promoted_mode<N, P, MODE, FAST>(A, nodes, k, nn2[k], th2[k], kk2[k], Mm[k], T0, T1, T2);
            }
            promoted_transfer<N>(k, T0, T1, T2, acc);
        }
        pair_terms<N, P, CLOUDY_SPEC>(A, Mm, acc);
        const bool skip = A.rainshaft && all_small;  // rainshaft_helpers.jl:67-68
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const int off = A.off[k];
            st_stream(out + (size_t)(off + 0) * ld + i, skip ? 0.0 : acc[k][0] * A.out_scale[3 * k + 0]);
            st_stream(out + (size_t)(off + 1) * ld + i, skip ? 0.0 : acc[k][1] * A.out_scale[3 * k + 1]);
            if (A.np[k] == 3) st_stream(out + (size_t)(off + 2) * ld + i, skip ? 0.0 : acc[k][2] * A.out_scale[3 * k + 2]);
        }
    }
