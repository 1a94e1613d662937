// adaptive_column.hpp -- per-COLUMN adaptive Tsit5 for rainshaft columns (cloudy_rainshaft_tsit5_adaptive): every column of a batch
// is one ODE system -- its cells couple through the upwind flux -- and carries one time, one step size and one error estimate
// from t = 0 to t = t_span.
//
// The sedimentation CFL limit dz / v(x) follows the largest drops of a column, the coalescence rate the number concentration of
// its cloud slab, and evaporation below cloud base shrinks a mode linearly in t: a batch of columns has no common dt that is both
// stable and cheap.  The loop is tsit5_adaptive_loop<RANKED = true> of adaptive.hpp -- stages, error estimate, controller, last-
// and first-step rules, statuses, max_steps, FSAL hand-over, snapshots, final store: nothing of it is restated here -- with
// adaptive::ColumnGroup in the place of the lane group: the nz lanes that hold a column's cells share one controller.  This file
// holds the column's right-hand side and the body that puts the two together.  What the group decides, and why:
//
//   layout     as rainshaft_ssprk33_body: a workgroup of BS threads owns floor(BS / nz) whole columns, one lane per cell; the state
//              is physical for every plan (abstol_i = abstol norm_i).
//   rhs        column_rhs below: ONE evaluation of the column right-hand side (cloudy_rainshaft_rhs; COND: cloudy_rainshaft_cond_rhs)
//              on a clamped COPY of its argument -- the stage arguments are not mutated.  The flux of the cell above comes through
//              LDS in every evaluation.
//   clamp      (kClamp) u is clamped to >= 0 on load and u_new before k7 = f(u_new): what the reference's in-place clamp
//              (rainshaft_helpers.jl:52) does to the state under a FSAL method.  The clamped u_new is what the error scale, the
//              acceptance and the store see, so the returned state is clamped, as cloudy_rainshaft_ssprk33_steps returns it.
//   norm       (sum, count) EEst = sqrt(sum over the column's nz cells and the planes a mode has of (err / sc)^2 / (nz n_moms));
//              empty cells count in the mean; Hairer's first guess uses the same two column means.  Every lane puts its cell's
//              partial sum into an LDS row, and after a barrier every lane of the column adds the column's nz entries in cell
//              order: the order depends on nz alone, not on where the column sits in the workgroup nor on BS, and the lanes of a
//              column hold the same bits.
//   control    t, dt, qold, the counts and the status are kept by every lane of the column, as the loop keeps them for a parcel;
//              computed from the same bits by the same instructions they stay equal, so the lanes of a column take the same
//              accept / reject branch and a column's result depends neither on its neighbours nor on the workgroup size.
//   loop       barrier-synchronous: every lane of the workgroup makes the same sequence of right-hand-side calls while ANY column
//              of the workgroup is active (__syncthreads_or); the lanes of a finished column and the lanes without a cell pass
//              live = false and sit through the barriers.  The sums hold barriers too (kBarriers), so the two of the first step
//              are formed whether or not the caller gave a dt.  max_steps bounds the loop whatever the input.
//   outputs    dt_dev, t_dev (one double per column) and info_dev (int32 [3][n_columns]: accepted, rejected, status) are written by
//              the lane of the column's lowest cell (leader); each may be null.
//
// Registers: u, k1 .. k6 and the stage state are eight [N][3] arrays per lane; the error combination goes into k2 and k7 into k3.
// Nothing is parked in LDS.
//
// Dense output (SAVE = true, cloudy_rainshaft_tsit5_adaptive_saveat): tsit5_adaptive_loop's SAVE -- the cursor, the interpolant, the
// snapshot at the end of a step, at 0 and at t_span, the NaN fill, t_span = 0 -- and nothing of it feeds back into a step.
//   cursor     the lanes of a column hold equal t, h and t_new, so their cursors stay equal and they take the same branches.
//   snapshots  where t_save[j] == t_new the clamped u_new; inside a step the interpolant CLAMPED to >= 0 on the way out (kClamp):
//              the clamped u_new is what the integrator returns and what k7 was evaluated at, and without the clamp a snapshot just
//              inside a step whose u_new was clamped would be negative where the one at its end is not.  A save time 0: the bits of
//              u_in as loaded, before the clamp.  A column that stops with status 1 or 2 leaves a quiet NaN in every plane of every
//              cell for every snapshot beyond the time it reached.
//   layout     snapshot j, plane p, cell i = col nz + iz at u_save[((size_t)j planes + p) ld + i], physical units, the plan's plane
//              type, planes = the plan's; the lanes of a wave write neighbouring elements of a plane; columns nz n_columns .. ld
//              are not written, and neither does a lane without a cell write anything.
//   registers  k1 .. k7, u and w are all live when a step is accepted.  k7 has an array of its own (a ninth); the k1 .. k6 part of the
//              error estimate has none (kOwnErr = false, where a parcel's loop gives it a tenth): k1 .. k6 are still there after
//              k7 = f(u_new), and the norm forms the same expression from the same operands there -- the same bits as the copy
//              SAVE = false keeps in k2.  What does not fit the architectural registers goes to the accumulation registers or to
//              scratch (DESIGN 3.5 has the figures); no LDS row is parked, so the LDS is that of SAVE = false.
//   barriers   the snapshot code sits after `if (!active) continue;`, outside column_rhs and the group's sum, and holds no barrier:
//              the sequence of barriers per loop trip is that of SAVE = false.
//
// This header includes adaptive.hpp alone; kernels.hpp and the fixed-step column units do not know it.
#pragma once
#include "adaptive.hpp"

namespace cloudy {

// One evaluation of the column right-hand side for the cell of this lane: (live, state) -> deriv, physical units.  The expressions
// and their order are those of rainshaft_ssprk33_body<RHS_ONLY> -- the clamp, the closure inversion, the empty-cell rule, the
// coalescence integrals (coal_ints_parcel; with a threshold coal_ints_ranked_impl, which re-ranks the workgroup at barriers, so
// every lane of the workgroup must call this), the sedimentation flux and its exchange through LDS, the condensation tendency, and
// (coal scale + divergence) + cond -- on a clamped copy of `state`.  live: the lane holds a cell of a column that is still being
// integrated (false: deriv = 0; the lane only sits through the barriers).  top: the lane's cell is the column's highest (zero
// flux from above).  Two barriers of its own: the fluxes are complete, the fluxes have been read.
template <int N, int P, int MODE, bool SPEC, int BS, bool COND>
__device__ __forceinline__ void column_rhs(const KArgs<N, P> &A, const SediArgs &S, const double *__restrict__ nodes, bool live, bool top,
                                           double dz, double coef, double sv, const double (&state)[N][3], double (&deriv)[N][3]) {
    const int pos = threadIdx.x;
    double nn[N], th[N], kk[N], acc[N][3];
    bool all_small = true;
#pragma unroll
    for (int m = 0; m < N; ++m) {
        nn[m] = 0.0;
        th[m] = 1.0;
        kk[m] = 1.0;
        acc[m][0] = acc[m][1] = acc[m][2] = 0.0;
    }
    if (live) {
#pragma unroll
        for (int m = 0; m < N; ++m) {
            double c[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) c[q] = state[m][q] < 0.0 ? 0.0 : state[m][q];   // rainshaft_helpers.jl:52, on a copy
            const double m0 = div_by_const(c[0], A.norm[3 * m + 0], A.inv_norm[3 * m + 0]);
            const double m1 = div_by_const(c[1], A.norm[3 * m + 1], A.inv_norm[3 * m + 1]);
            const double m2 = div_by_const(c[2], A.norm[3 * m + 2], A.inv_norm[3 * m + 2]);
            all_small = all_small && (m0 < kEps) && (m1 < kEps) && (A.np[m] != 3 || m2 < kEps);
            invert_closure(A.dist_type[m], m0, m1, m2, A.kmin, A.kmax, nn[m], th[m], kk[m]);
        }
    }
    double (*fx)[BS];   // the flux-exchange rows of this evaluation
    if constexpr (MODE == MODE_ALLINF) {
        __shared__ double sh_flux[3 * N][BS];
        fx = sh_flux;
        if (live) coal_ints_parcel<N, P, MODE, false, SPEC>(A, nodes, nn, th, kk, acc);
    } else {
        // every lane of the workgroup: barriers inside.  (n, theta, k) come back from the lane's LDS slots, and those 3N rows --
        // read by nobody but their owner once the passes are done -- then carry the flux exchange
        coal_ints_ranked_impl<N, P, MODE, SPEC, BS, true>(A, nodes, live, nn, th, kk, acc, fx);
    }
    double fc[COND ? N : 1][3];   // the condensation tendency of the lane's own cell, physical units
    if (live) {
        double fl[N][3];
        sedi_flux_parcel<N>(A.dist_type, S, nn, th, kk, fl);
#pragma unroll
        for (int m = 0; m < N; ++m)
#pragma unroll
            for (int q = 0; q < 3; ++q) fx[3 * m + q][pos] = (q < A.np[m]) ? fl[m][q] * A.out_scale[3 * m + q] : 0.0;
        if constexpr (COND) cond_evap_parcel<N, P, true>(A, coef, sv, nn, th, kk, fc);
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < N; ++m)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            double ft = 0.0;
            if (live) {   // (a live lane below the top of its column: pos + 1 is the cell above, inside the workgroup)
                const double f_up = top ? 0.0 : fx[3 * m + q][pos + 1];
                const double fd = -(f_up - fx[3 * m + q][pos]) / dz;   // :83-85
                // coal_source .+ sedi_source (:88), empty cells skip coalescence (:67-72)
                ft = ((q < A.np[m] && !all_small) ? acc[m][q] * A.out_scale[3 * m + q] : 0.0) + fd;
                if constexpr (COND) ft += fc[m][q];
            }
            deriv[m][q] = ft;
        }
    __syncthreads();   // (the next evaluation writes these rows)
}

// cloudy_rainshaft_tsit5_adaptive / cloudy_rainshaft_tsit5_adaptive_saveat: the loop for column groups on column_rhs.  u_in /
// u_out: the plan's planes (they may alias: a lane reads and writes its own cell).  s_dev: one supersaturation per cell, loaded
// once (null: s_scalar).  SAVE: n_save, t_save and u_save as tsit5_adaptive_loop takes them; without it they are not read.
template <int N, int P, int MODE, typename TIO, bool SPEC, int BS, bool COND, bool SAVE = false>
__device__ __forceinline__ void column_tsit5_adaptive_body(const KArgs<N, P> *__restrict__ Ag, const SediArgs *__restrict__ Sg,
                                                           const double *__restrict__ nodes, int nz, size_t n_columns, size_t ld,
                                                           const TIO *u_in, TIO *u_out, double dz, double t_span, AdaptiveOpts o,
                                                           double *dt_dev, double *t_dev, int *info_dev, double coef = 0.0,
                                                           double s_scalar = 0.0, const double *__restrict__ s_dev = nullptr,
                                                           size_t n_save = 0, const double *__restrict__ t_save = nullptr,
                                                           TIO *__restrict__ u_save = nullptr) {
    const adaptive::ColumnGroup<BS> g(nz, n_columns);
    const double sv = COND && g.valid ? (s_dev ? s_dev[g.i] : s_scalar) : 0.0;
    const bool top = g.iz == nz - 1;
    // the plan constants through an opaque zero offset per evaluation (see ssprk33_body); none when compiled for the plan
    tsit5_adaptive_loop<N, P, TIO, true, BS, SAVE>(
        *Ag, g, ld, u_in, u_out, t_span, o, dt_dev, t_dev, info_dev, n_save, t_save, u_save,
        [&](bool live, const double (&state)[N][3], double (&deriv)[N][3]) {
            size_t oz = 0;
            if (!SPEC) asm volatile("" : "+s"(oz));
            column_rhs<N, P, MODE, SPEC, BS, COND>(*(Ag + oz), *(Sg + oz), nodes, live, top, dz, coef, sv, state, deriv);
        });
}

}  // namespace cloudy
