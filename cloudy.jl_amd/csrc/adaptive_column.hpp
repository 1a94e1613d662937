// adaptive_column.hpp -- per-COLUMN adaptive Tsit5 for rainshaft columns (cloudy_rainshaft_tsit5_adaptive): every column of a batch
// is one ODE system -- its cells couple through the upwind flux -- and carries one time, one step size and one error estimate
// from t = 0 to t = t_span.
//
// The sedimentation CFL limit dz / v(x) follows the largest drops of a column, the coalescence rate the number concentration of
// its cloud slab, and evaporation below cloud base shrinks a mode linearly in t: a batch of columns has no common dt that is both
// stable and cheap.  tsit5_adaptive_loop (adaptive.hpp) gives every LANE its own t, dt and error norm; here the nz lanes that hold
// a column's cells share them.  The tableau (tsit5:: of kernels.hpp), the error weights bt1 .. bt7 and the controller constants
// (adaptive::k*) are the ones of adaptive.hpp, and so are the controller, the last-step rule, the first-step rule, the statuses
// and max_steps: nothing of them is restated here.  What differs:
//
//   layout     as rainshaft_ssprk33_body: a workgroup of BS threads owns floor(BS / nz) whole columns, one lane per cell; the state
//              is physical for every plan (abstol_i = abstol norm_i).
//   rhs        column_rhs below: ONE evaluation of the column right-hand side (cloudy_rainshaft_rhs; COND: cloudy_rainshaft_cond_rhs)
//              on a clamped COPY of its argument -- the stage arguments are not mutated.  The flux of the cell above comes through
//              LDS in every evaluation.
//   clamp      u is clamped to >= 0 on load and u_new before k7 = f(u_new): what the reference's in-place clamp
//              (rainshaft_helpers.jl:52) does to the state under a FSAL method.  The clamped u_new is what the error scale, the
//              acceptance and the store see, so the returned state is clamped, as cloudy_rainshaft_ssprk33_steps returns it.
//   norm       EEst = sqrt(sum over the column's nz cells and the planes a mode has of (err / sc)^2 / (nz n_moms)); empty cells
//              count in the mean; Hairer's first guess uses the same two column means.  Every lane puts its cell's partial sum
//              into an LDS row, and after a barrier every lane of the column adds the column's nz entries in cell order: the order
//              depends on nz alone, not on where the column sits in the workgroup nor on BS, and the lanes of a column hold the
//              same bits.
//   control    t, dt, qold, the counts and the status are kept by every lane of the column; computed from the same bits by the
//              same instructions they stay equal, so the lanes of a column take the same accept / reject branch and a column's
//              result depends neither on its neighbours nor on the workgroup size.
//   loop       barrier-synchronous: every lane of the workgroup makes the same sequence of right-hand-side calls while ANY column
//              of the workgroup is active (__syncthreads_or); the lanes of a finished column and the lanes without a cell pass
//              live = false and sit through the barriers.  max_steps bounds the loop whatever the input.
//   outputs    dt_dev, t_dev (one double per column) and info_dev (int32 [3][n_columns]: accepted, rejected, status) are written by
//              the lane of the column's lowest cell; each may be null.
//
// Registers: u, k1 .. k6 and the stage state are eight [N][3] arrays per lane; the error combination goes into k2 and k7 into k3
// as in tsit5_adaptive_loop.  Nothing is parked in LDS.
//
// Dense output (SAVE = true, cloudy_rainshaft_tsit5_adaptive_saveat): the rules of tsit5_adaptive_loop's SAVE, restated for a
// column; the same loop, the same expressions, the same controller and the same barriers -- nothing of it feeds back into a step.
//   cursor     every lane keeps a cursor j into t_save[0 .. n_save) (device doubles, strictly increasing, within [0, t_span]); the
//              lanes of a column hold equal t, h and t_new, so their cursors stay equal and they take the same branches.
//   snapshots  after an accepted step t -> t_new, while t_save[j] <= t_new: where t_save[j] == t_new the clamped u_new (w) through
//              the expressions of the final store (a snapshot at t_span has the bits of u_out); otherwise u + h sum_i b_i(th) k_i,
//              i = 1 .. 7, th = (t_save[j] - t) / h (tsit5::interp_weights), CLAMPED to >= 0 on the way out: the clamped u_new is
//              what the integrator returns and what k7 was evaluated at, and without the clamp a snapshot just inside a step
//              whose u_new was clamped would be negative where the one at its end is not.  A save time 0: the bits of u_in as
//              loaded, before the clamp.  t_span = 0: every snapshot is the input.  A column that stops with status 1 or 2 leaves
//              a quiet NaN in every plane of every cell for every snapshot beyond the time it reached.
//   layout     snapshot j, plane p, cell i = col nz + iz at u_save[((size_t)j planes + p) ld + i], physical units, the plan's plane
//              type, planes = the plan's; the lanes of a wave write neighbouring elements of a plane; columns nz n_columns .. ld
//              are not written, and neither does a lane without a cell write anything.
//   registers  k1 .. k7, u and w are all live when a step is accepted.  k7 has an array of its own (a ninth); the k1 .. k6 part of the
//              error estimate has none: k1 .. k6 are still there after k7 = f(u_new), and the norm forms the same expression
//              from the same operands there -- the same bits as the copy SAVE = false keeps in k2.  What does not fit the
//              architectural registers goes to the accumulation registers or to scratch (DESIGN 3.5 has the figures); no LDS row
//              is parked, so the LDS is that of SAVE = false.
//   barriers   the snapshot code sits after `if (!active) continue;`, outside column_rhs and column_sum, and holds no barrier:
//              the sequence of barriers per loop trip is that of SAVE = false.
//
// This header includes adaptive.hpp alone; kernels.hpp, adaptive.hpp and the fixed-step column units do not know it.
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

// The loop.  u_in / u_out: the plan's planes (they may alias: a lane reads and writes its own cell).  s_dev: one supersaturation
// per cell, loaded once (null: s_scalar).  SAVE: n_save, t_save and u_save (n_save x planes planes of leading dimension ld,
// aliasing neither u_in nor u_out) as above; without it they are not read.
template <int N, int P, int MODE, typename TIO, bool SPEC, int BS, bool COND, bool SAVE = false>
__device__ __forceinline__ void column_tsit5_adaptive_body(const KArgs<N, P> *__restrict__ Ag, const SediArgs *__restrict__ Sg,
                                                           const double *__restrict__ nodes, int nz, size_t n_columns, size_t ld,
                                                           const TIO *u_in, TIO *u_out, double dz, double t_span, AdaptiveOpts o,
                                                           double *dt_dev, double *t_dev, int *info_dev, double coef = 0.0,
                                                           double s_scalar = 0.0, const double *__restrict__ s_dev = nullptr,
                                                           size_t n_save = 0, const double *__restrict__ t_save = nullptr,
                                                           TIO *__restrict__ u_save = nullptr) {
    using namespace tsit5;
    using St = adaptive::State<N, 0>;
    __shared__ double sh_sum[BS];   // the cells' partial sums of a column norm
    const KArgs<N, P> &A = *Ag;
    const int cpb = BS / nz;        // whole columns per workgroup
    const int pos = threadIdx.x;    // cell slot of the workgroup: column pos / nz, level pos % nz
    const int cl = pos / nz, iz = pos - cl * nz;
    const size_t col = (size_t)blockIdx.x * cpb + cl;
    const bool valid = (cl < cpb) && (col < n_columns);
    const size_t i = col * (size_t)nz + iz;
    const bool top = iz == nz - 1, first = iz == 0;
    // SAVE: component (m, q) of snapshot js of this lane's cell, as the final store writes u -- physical units, the planes a mode has
    size_t planes = 0;
    if constexpr (SAVE) {
#pragma unroll
        for (int m = 0; m < N; ++m) planes += A.np[m] == 3 ? 3 : 2;
    }
    auto save = [&](size_t js, int m, int q, TIO x) {
        if (q < A.np[m]) u_save[(js * planes + (size_t)(A.off[m] + q)) * ld + i] = x;
    };
    if (!(t_span > 0.0)) {   // (workgroup-uniform: a kernel argument) nothing to integrate, the planes as they are
        if (!valid) return;
#pragma unroll
        for (int m = 0; m < N; ++m)
#pragma unroll
            for (int q = 0; q < 3; ++q)
                if (q < A.np[m]) {
                    const TIO v = u_in[(size_t)(A.off[m] + q) * ld + i];
                    u_out[(size_t)(A.off[m] + q) * ld + i] = v;
                    if constexpr (SAVE)   // (every save time is 0)
                        for (size_t js = 0; js < n_save; ++js) save(js, m, q, v);
                }
        if (first) {
            if (t_dev) t_dev[col] = 0.0;
            if (info_dev) info_dev[col] = 0, info_dev[n_columns + col] = 0, info_dev[2 * n_columns + col] = ADAPT_DONE;
        }
        return;
    }
    St u, atol;
    int count = 0;
    const bool save0 = SAVE && valid && n_save > 0 && t_save[0] == 0.0;
    size_t j = save0 ? 1 : 0;   // SAVE: the lane's cursor into t_save
#pragma unroll
    for (int m = 0; m < N; ++m) {
        count += A.np[m] == 3 ? 3 : 2;   // (the planes a mode has: the third slot of a two-moment mode is padding)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const double v = (valid && q < A.np[m]) ? (double)u_in[(size_t)(A.off[m] + q) * ld + i] : 0.0;
            if constexpr (SAVE)   // a save time 0: the values as loaded, before the clamp
                if (save0) save(0, m, q, (TIO)v);
            u.m[m][q] = v < 0.0 ? 0.0 : v;   // the clamp of the first evaluation, in place in the reference
            atol.m[m][q] = o.abstol * A.norm[3 * m + q];
        }
    }
    const double sv = COND && valid ? (s_dev ? s_dev[i] : s_scalar) : 0.0;
    const double n_norm = (double)count * (double)nz;   // components of a column
    bool active = valid;
    auto rhs = [&](const St &state, St &deriv) {
        size_t oz = 0;   // the plan constants through an opaque zero offset per evaluation (see ssprk33_body); none when compiled for the plan
        if (!SPEC) asm volatile("" : "+s"(oz));
        column_rhs<N, P, MODE, SPEC, BS, COND>(*(Ag + oz), *(Sg + oz), nodes, active, top, dz, coef, sv, state.m, deriv.m);
    };
    // the column's sum of the cells' partial sums `part`, in cell order, the same bits in every lane of the column (a lane without
    // a cell: 0); every lane of the workgroup calls it
    auto column_sum = [&](double part) {
        __syncthreads();   // (whoever still reads the row's last sums)
        sh_sum[pos] = part;
        __syncthreads();
        double s = 0.0;
        if (cl < cpb) {
            const int base = cl * nz;
            for (int j = 0; j < nz; ++j) s += sh_sum[base + j];
        }
        return s;
    };
    St k1, k2, k3, k4, k5, k6, w;
    // where the error combination and k7 go: k2 and k3, dead by then (see tsit5_adaptive_loop) -- SAVE keeps k1 .. k7 for the
    // interpolant: k7 gets an array of its own (not touched, and so not there, without it) and the error combination is formed
    // in the norm, from k1 .. k6
    St k7_own;
    St &ke = k2;
    St &k7 = *[&]() -> St * { if constexpr (SAVE) return &k7_own; else return &k3; }();
    rhs(u, k1);
    // ---- the first step
    double dt = dt_dev && valid ? dt_dev[col] : o.dt_init;
    {   // (every lane attends the two sums; a column with a dt of the caller's does not use them)
        double s0 = 0.0, s1 = 0.0;
        adaptive::counted<N, 0>(A.np, [&](double uu, double kk, double at) {
            const double sc = fma(o.reltol, fabs(uu), at);
            const double r0 = uu / sc, r1 = kk / sc;
            s0 = fma(r0, r0, s0);
            s1 = fma(r1, r1, s1);
        }, u, k1, atol);
        s0 = column_sum(s0);
        s1 = column_sum(s1);
        if (!(dt > 0.0 && adaptive::is_finite(dt))) {
            const double d0 = sqrt(s0 / n_norm), d1 = sqrt(s1 / n_norm);
            dt = d1 == 0.0 ? t_span : 0.01 * d0 / d1;
        }
    }
    dt = dt > t_span ? t_span : dt;   // (keeps a NaN: status 2 below)
    double t = 0.0, qold = adaptive::kQold0;
    int n_acc = 0, n_rej = 0, status = ADAPT_DONE;
    const double t_last = t_span * (1.0 - 4.0 * kEps), dt_min = 1e-14 * t_span;
#pragma unroll 1
    for (;;) {
        if (active) {
            if (n_acc + n_rej >= o.max_steps) status = ADAPT_MAX_STEPS, active = false;
            else if (!(dt >= dt_min) || !adaptive::is_finite(dt)) status = ADAPT_DT_MIN, active = false;
        }
        if (!__syncthreads_or(active ? 1 : 0)) break;
        const bool last = t + dt >= t_last;
        const double h = last ? t_span - t : dt;
        adaptive::each<N, 0>([&](double &ww, double c1, double uu) { ww = fma(h * a21, c1, uu); }, w, k1, u);
        rhs(w, k2);
        adaptive::each<N, 0>([&](double &ww, double c1, double c2, double uu) { ww = fma(h, fma(a31, c1, a32 * c2), uu); }, w, k1, k2, u);
        rhs(w, k3);
        adaptive::each<N, 0>([&](double &ww, double c1, double c2, double c3, double uu) {
            ww = fma(h, fma(a41, c1, fma(a42, c2, a43 * c3)), uu);
        }, w, k1, k2, k3, u);
        rhs(w, k4);
        adaptive::each<N, 0>([&](double &ww, double c1, double c2, double c3, double c4, double uu) {
            ww = fma(h, fma(a51, c1, fma(a52, c2, fma(a53, c3, a54 * c4))), uu);
        }, w, k1, k2, k3, k4, u);
        rhs(w, k5);
        adaptive::each<N, 0>([&](double &ww, double c1, double c2, double c3, double c4, double c5, double uu) {
            ww = fma(h, fma(a61, c1, fma(a62, c2, fma(a63, c3, fma(a64, c4, a65 * c5)))), uu);
        }, w, k1, k2, k3, k4, k5, u);
        rhs(w, k6);
        // u_new, clamped, into w; the k1 .. k6 part of the error estimate into k2, which is dead from here; then k7 into k3
        if constexpr (!SAVE) {
            adaptive::each<N, 0>([&](double &ww, double &ee, double c1, double c2, double c3, double c4, double c5, double c6, double uu) {
                const double un = fma(h, fma(a71, c1, fma(a72, c2, fma(a73, c3, fma(a74, c4, fma(a75, c5, a76 * c6))))), uu);
                ww = un < 0.0 ? 0.0 : un;
                ee = fma(bt1, c1, fma(bt2, c2, fma(bt3, c3, fma(bt4, c4, fma(bt5, c5, bt6 * c6)))));
            }, w, ke, k1, k2, k3, k4, k5, k6, u);
        } else {
            adaptive::each<N, 0>([&](double &ww, double c1, double c2, double c3, double c4, double c5, double c6, double uu) {
                const double un = fma(h, fma(a71, c1, fma(a72, c2, fma(a73, c3, fma(a74, c4, fma(a75, c5, a76 * c6))))), uu);
                ww = un < 0.0 ? 0.0 : un;
            }, w, k1, k2, k3, k4, k5, k6, u);
        }
        rhs(w, k7);
        double s = 0.0;
        if constexpr (!SAVE) {
            adaptive::counted<N, 0>(A.np, [&](double c7, double ee, double uu, double ww, double at) {
                const double err = h * fma(bt7, c7, ee);
                const double sc = fma(o.reltol, fmax(fabs(uu), fabs(ww)), at);
                const double r = err / sc;
                s = fma(r, r, s);
            }, k7, ke, u, w, atol);
        } else {   // (ee: the expression above, on the same operands)
            adaptive::counted<N, 0>(A.np, [&](double c7, double c1, double c2, double c3, double c4, double c5, double c6, double uu,
                                              double ww, double at) {
                const double ee = fma(bt1, c1, fma(bt2, c2, fma(bt3, c3, fma(bt4, c4, fma(bt5, c5, bt6 * c6)))));
                const double err = h * fma(bt7, c7, ee);
                const double sc = fma(o.reltol, fmax(fabs(uu), fabs(ww)), at);
                const double r = err / sc;
                s = fma(r, r, s);
            }, k7, k1, k2, k3, k4, k5, k6, u, w, atol);
        }
        const double eest = sqrt(column_sum(s) / n_norm);
        if (!active) continue;   // (a finished column, a lane without a cell: it only sat through the barriers)
        if (!adaptive::is_finite(eest)) {
            ++n_rej;
            dt = h / 5.0;
            continue;
        }
        const double q11 = eest > 0.0 ? exp_fin(adaptive::kBeta1 * log_pos(eest)) : 0.0;
        if (eest <= 1.0) {
            double q = q11 / exp_fin(adaptive::kBeta2 * log_pos(qold)) / adaptive::kSafety;
            q = fmin(fmax(q, 1.0 / adaptive::kQmax), 1.0 / adaptive::kQmin);
            ++n_acc;
            if constexpr (SAVE) {
                const double t_new = last ? t_span : t + h;
                while (j < n_save) {
                    const double ts = t_save[j];
                    if (!(ts <= t_new)) break;
                    if (ts == t_new) {   // (the end of the step: u_new itself, what the final store writes at t_span)
#pragma unroll
                        for (int m = 0; m < N; ++m)
#pragma unroll
                            for (int q = 0; q < 3; ++q) save(j, m, q, (TIO)w.m[m][q]);
                    } else {
                        double b[7];
                        interp_weights((ts - t) / h, b);
#pragma unroll
                        for (int m = 0; m < N; ++m)
#pragma unroll
                            for (int q = 0; q < 3; ++q) {
                                const double v = fma(h, fma(b[0], k1.m[m][q], fma(b[1], k2.m[m][q], fma(b[2], k3.m[m][q], fma(b[3], k4.m[m][q],
                                                    fma(b[4], k5.m[m][q], fma(b[5], k6.m[m][q], b[6] * k7.m[m][q])))))), u.m[m][q]);
                                save(j, m, q, (TIO)(v < 0.0 ? 0.0 : v));
                            }
                    }
                    ++j;
                }
            }
            t = last ? t_span : t + h;
            dt = fmax(h / q, fmin(dt, dt / q));
            qold = fmax(eest, adaptive::kQold0);
            adaptive::each<N, 0>([&](double &uu, double &c1, double ww, double c7) { uu = ww, c1 = c7; }, u, k1, w, k7);
            if (last) active = false;   // status 0
        } else {
            ++n_rej;
            dt = h / fmin(1.0 / adaptive::kQmin, q11 / adaptive::kSafety);
        }
    }
    if (!valid) return;
    if constexpr (SAVE) {   // what a column stopped by the budget or by dt did not reach (status 0: the cursor is at n_save)
        const TIO nan = (TIO)__builtin_nan("");
        for (; j < n_save; ++j) {
#pragma unroll
            for (int m = 0; m < N; ++m)
#pragma unroll
                for (int q = 0; q < 3; ++q) save(j, m, q, nan);
        }
    }
#pragma unroll
    for (int m = 0; m < N; ++m)
#pragma unroll
        for (int q = 0; q < 3; ++q)
            if (q < A.np[m]) u_out[(size_t)(A.off[m] + q) * ld + i] = (TIO)u.m[m][q];
    if (first) {
        if (dt_dev) dt_dev[col] = dt;
        if (t_dev) t_dev[col] = t;
        if (info_dev) info_dev[col] = n_acc, info_dev[n_columns + col] = n_rej, info_dev[2 * n_columns + col] = status;
    }
}

}  // namespace cloudy
