// adaptive.hpp -- per-parcel adaptive Tsit5 (cloudy_tsit5_adaptive): every parcel of a batch is its own ODE and carries its own
// time, step size and error estimate from t = 0 to t = t_span.
//
// The fused integrators of kernels.hpp take one dt and one n_steps for the whole batch.  A host model advances 1e6-1e7 boxes whose
// number concentrations span decades by ONE model time step; collision rates scale with n, so a dt that is safe for the densest box
// wastes work on nearly every other one.  Here a lane steps its parcel with the 5(4) pair of the Tsit5 tableau (tsit5:: of
// kernels.hpp, the stage arithmetic of tsit5_advance) under a step-size controller of its own, and reports what happened.
//
//   stages     k1 .. k6 as tsit5_advance, u_new from the 5th-order weights a71 .. a76, then k7 = f(u_new): the error estimate needs
//              it and an accepted step hands it on as the next k1 (FSAL); a rejected step keeps k1.  6 evaluations per attempted
//              step + 1 at the start.
//   estimate   err_i = h sum_j bt_j k_j,i with bt = b - b^ (the embedded 4th-order weights), h the step tried;
//              sc_i = abstol_i + reltol max(|u_i|, |u_new,i|);  EEst = sqrt(mean_i (err_i / sc_i)^2) over the parcel's prognostic
//              moments (the padded third slot of a two-moment mode does not count).  abstol is in the plan's NORMALISED units
//              (mom ./ norms): all-Inf plans keep their state normalised (abstol_i = abstol), thresholded plans keep it physical
//              (abstol_i = abstol norm_i).
//   controller a PI controller with these constants (stated here, not taken from a run of any other solver, and no bit identity
//              with one is claimed): beta1 = 7/50, beta2 = 2/25, gamma = 9/10, qmin = 1/5, qmax = 10, qold_0 = 1e-4;
//              q11 = EEst^beta1, q = clamp(q11 / qold^beta2 / gamma, 1/qmax, 1/qmin) (EEst = 0: q = 1/qmax).
//              EEst <= 1: accept -- t += h, dt <- max(h / q, min(dt, dt / q)), qold <- max(EEst, qold_0);
//              otherwise reject -- dt <- h / min(1/qmin, q11 / gamma); an EEst that is not finite rejects with dt <- h / 5.
//              The powers are exp_fin(beta log_pos(.)) of device_math.hpp.
//   last step  t + dt >= t_span (1 - 4 eps): the step tried is h = t_span - t and t lands on t_span exactly; otherwise h = dt, and
//              the accept rule reads dt <- dt / q.  For a clamped step (h < dt) the proposal that goes out is the UNCLAMPED one: dt
//              shrinks as the estimate of the shorter step asks (dt / q, q >= 1) but does not grow past what that step supports
//              (max(h / q, dt), q < 1) -- a caller that comes back with dt_dev for the next model step starts warm, not from the
//              remainder of the last one.
//   first step the caller's dt where it is positive and finite (dt_dev[i], else opts.dt_init); otherwise Hairer's first guess
//              0.01 ||u||_sc / ||f(u)||_sc with sc_i = abstol_i + reltol |u_i| (||f|| = 0: t_span); capped at t_span.
//   stop       t = t_span (status 0); accepted + rejected = max_steps (status 1); dt < 1e-14 t_span or not finite (status 2).
//              max_steps bounds the loop whatever the input.
//
// All-Inf plans: a plain per-lane loop; the lanes of a wave finish at different times (the cost of per-parcel control; the entry
// point's info planes give the active-lane fraction).  Thresholded plans: rhs_physical re-ranks the workgroup at barriers in
// every evaluation, so every lane makes the same sequence of calls: the loop runs while ANY lane of the workgroup is active
// (__syncthreads_or), a finished or out-of-range lane passes valid = false and discards the result, and nothing returns before
// the loop ends.
//
// Registers: u, k1 .. k6 and the stage state are eight [N][3] arrays as in tsit5_advance; the k1 .. k6 part of the error estimate
// is accumulated into k2 (dead once u_new exists) and k7 goes into k3, so no further array is live.
//
// Dense output (SAVE = true, cloudy_tsit5_adaptive_saveat): the same loop, the same expressions and the same controller -- nothing
// of what follows feeds back into a step -- plus the state at the batch-wide save times t_save[0 .. n_save) (device doubles,
// strictly increasing, within [0, t_span]).  Every lane keeps a cursor j.  After an accepted step t -> t_new, while t_save[j] <=
// t_new: th = (t_save[j] - t) / h and snapshot j is u + h sum_i b_i(th) k_i, i = 1 .. 7 (tsit5::interp_weights: the free 4th-order
// interpolant of the pair, no further evaluation), or u_new through the expressions of the final store where t_save[j] == t_new
// (a snapshot at t_span has the bits of u_out).  A save time 0 gets the values as loaded (the bits of u_in); what a stopped
// parcel (status 1, 2) did not reach gets a quiet NaN.  Snapshots are stored in physical units in the plan's plane type at
// u_save[((size_t)j * planes + p) * ld + i]: the lanes of a wave write neighbouring elements of a plane.  So that k1 .. k7, u and
// u_new are all live when a step is accepted, the error combination and k7 have arrays of their own (two more than above).
// The snapshot code sits outside the right-hand side: the barriers of a thresholded plan are the ones of SAVE = false.
//
// This header includes kernels.hpp alone and kernels.hpp does not know it: the text of every other plan-time unit stays as it is.
#pragma once
#include "kernels.hpp"

namespace cloudy {

namespace tsit5 {
// btilde = b - b^ ; sum_j bt_j c_j^p = 0 for p = 0 .. 3 with c = (0, 0.161, 0.327, 0.9, 0.9800255409045097, 1, 1)
constexpr double bt1 = -0.00178001105222577714, bt2 = -0.0008164344596567469, bt3 = 0.007880878010261995,
                 bt4 = -0.1447110071732629, bt5 = 0.5823571654525552, bt6 = -0.45808210592918697, bt7 = 0.015151515151515152;
__device__ __forceinline__ double err_k1_k6(double c1, double c2, double c3, double c4, double c5, double c6) {   // (bt7 k7 is added in the norm)
    return fma(bt1, c1, fma(bt2, c2, fma(bt3, c3, fma(bt4, c4, fma(bt5, c5, bt6 * c6)))));
}
// the interpolant over k1 .. k7, th in [0, 1]: b1 = s th (th - r1)(th^2 - p th + q); b2, b3 = s th^2 (th^2 - p th + q);
// b4 .. b7 = s th^2 (th - r1)(th - r2).  b_i(1) = a7i, b7(1) = 0; sum_i b_i(th) c_i^p = th^(p+1) / (p+1) for p = 0 .. 3
constexpr double bi1_s = -1.0530884977290216, bi1_r1 = 1.3299890189751412, bi1_p = 1.4364028541716351, bi1_q = 0.7139816917074209;
constexpr double bi2_s = 0.1017, bi2_p = 2.1966568338249754, bi2_q = 1.2949852507374631;
constexpr double bi3_s = 2.490627285651252793, bi3_p = 2.38535645472061657, bi3_q = 1.57803468208092486;
constexpr double bi4_s = -16.54810288924490272, bi4_r1 = 1.21712927295533244, bi4_r2 = 0.61620406037800089;
constexpr double bi5_s = 47.37952196281928122, bi5_r1 = 1.203071208372362603, bi5_r2 = 0.658047292653547382;
constexpr double bi6_s = -34.87065786149660974, bi6_r1 = 1.2, bi6_r2 = 0.666666666666666667;
constexpr double bi7_s = 2.5, bi7_r1 = 1.0, bi7_r2 = 0.6;
// (the quadratic factors by Horner: th (th - p) + q)
__device__ __forceinline__ void interp_weights(double th, double (&b)[7]) {
    const double th2 = th * th;
    b[0] = bi1_s * th * (th - bi1_r1) * fma(th, th - bi1_p, bi1_q);
    b[1] = bi2_s * th2 * fma(th, th - bi2_p, bi2_q);
    b[2] = bi3_s * th2 * fma(th, th - bi3_p, bi3_q);
    b[3] = bi4_s * th2 * ((th - bi4_r1) * (th - bi4_r2));
    b[4] = bi5_s * th2 * ((th - bi5_r1) * (th - bi5_r2));
    b[5] = bi6_s * th2 * ((th - bi6_r1) * (th - bi6_r2));
    b[6] = bi7_s * th2 * ((th - bi7_r1) * (th - bi7_r2));
}
}  // namespace tsit5

// cloudy_adaptive_opts without its struct_size: a kernel argument
struct AdaptiveOpts {
    double reltol, abstol, dt_init;
    int max_steps;
};
enum { ADAPT_DONE = 0, ADAPT_MAX_STEPS = 1, ADAPT_DT_MIN = 2 };   // the status plane

namespace adaptive {
constexpr double kBeta1 = 7.0 / 50.0, kBeta2 = 2.0 / 25.0, kSafety = 9.0 / 10.0 /* gamma */, kQmin = 1.0 / 5.0, kQmax = 10.0, kQold0 = 1e-4;
__device__ __forceinline__ bool is_finite(double x) { return fabs(x) < INFINITY; }   // (false for NaN)

// The state of one parcel in the loop: the [N][3] moment arrays and, beside them, X further scalars that the plan's norms do not
// touch (X = 0: none -- the member is never read or written, and so is not there).  each() applies f to one component of several
// states at a time, the scalars first, then every slot of the arrays (the padded third slot of a two-moment mode included: its
// tendency is zero); counted() likewise over the components that count in the norms (the planes a mode has).
template <int N, int X>
struct State {
    double x[X > 0 ? X : 1];
    double m[N][3];
};
template <int N, int X, typename F, typename... S>
__device__ __forceinline__ void each(F f, S &...s) {
#pragma unroll
    for (int q = 0; q < X; ++q) f(s.x[q]...);
#pragma unroll
    for (int m = 0; m < N; ++m)
#pragma unroll
        for (int q = 0; q < 3; ++q) f(s.m[m][q]...);
}
template <int N, int X, typename F, typename... S>
__device__ __forceinline__ void counted(const int (&np)[N], F f, S &...s) {
#pragma unroll
    for (int q = 0; q < X; ++q) f(s.x[q]...);
#pragma unroll
    for (int m = 0; m < N; ++m)
#pragma unroll
        for (int q = 0; q < 3; ++q)
            if (q < 2 || np[m] == 3) f(s.m[m][q]...);
}

// Who shares a controller.  The loop keeps t, dt, qold, the counts and the status in every lane; a GROUP says which lanes hold one
// ODE system between them and therefore one of each:
//   i, valid       the element of the planes this lane loads, advances and stores, and whether there is one
//   ctl, ctl_ld    the group's index into dt_dev / t_dev / info_dev, and the leading dimension of info_dev's three rows
//   leader         this lane writes them
//   count          lanes per group: the norms are means over count x (the components a lane counts)
//   sum(part)      the group's sum of its lanes' partial sums, the same bits in every lane of the group
//   kBarriers      sum holds workgroup barriers: every lane of the workgroup calls it, each time (RANKED loops only)
//   kClamp         the state is clamped to >= 0 wherever the loop forms one: on load, u_new before k7 = f(u_new), and an
//                  interpolated snapshot on the way out
//   kOwnErr        SAVE: the k1 .. k6 part of the error estimate has an array of its own (otherwise the norm forms it again from
//                  k1 .. k6, which SAVE keeps: the same expression on the same operands, one array less)
// LaneGroup: a lane is a parcel and a group -- element blockIdx.x BS + threadIdx.x of n, the planes' ld for the control planes.
// Every member folds: no barrier, no LDS and no clamp reaches a kernel that uses it.
template <int BS>
struct LaneGroup {
    static constexpr bool kBarriers = false, kClamp = false, kOwnErr = true, leader = true;
    static constexpr int count = 1;
    size_t i, ctl, ctl_ld;
    bool valid;
    __device__ __forceinline__ LaneGroup(size_t n, size_t ld) : i((size_t)blockIdx.x * BS + threadIdx.x), ctl(i), ctl_ld(ld), valid(i < n) {}
    __device__ __forceinline__ double sum(double part) const { return part; }
};
// ColumnGroup: the nz lanes that hold the cells of a column (adaptive_column.hpp).  A workgroup of BS threads owns cpb = floor(BS /
// nz) whole columns, one lane per cell, cell iz of column col at element col nz + iz; the control planes have one entry per column.
template <int BS>
struct ColumnGroup {
    static constexpr bool kBarriers = true, kClamp = true, kOwnErr = false;
    size_t i, ctl, ctl_ld;
    bool valid, leader;
    int count, iz, cl, cpb;   // (count = nz; iz: the lane's level; cl: its column's slot in the workgroup)
    __device__ __forceinline__ ColumnGroup(int nz, size_t n_columns) : ctl_ld(n_columns), count(nz), cpb(BS / nz) {
        cl = (int)threadIdx.x / nz, iz = (int)threadIdx.x - cl * nz;
        ctl = (size_t)blockIdx.x * cpb + cl;
        valid = (cl < cpb) && (ctl < n_columns);
        i = ctl * (size_t)nz + iz;
        leader = iz == 0;
    }
    // every lane puts its cell's partial sum into an LDS row, and after a barrier every lane of the column adds the column's nz
    // entries in cell order: the order depends on nz alone (a lane without a cell: 0)
    __device__ __forceinline__ double sum(double part) const {
        __shared__ double sh_sum[BS];
        __syncthreads();   // (whoever still reads the row's last sums)
        sh_sum[threadIdx.x] = part;
        __syncthreads();
        double s = 0.0;
        if (cl < cpb) {
            const int base = cl * count;
            for (int j = 0; j < count; ++j) s += sh_sum[base + j];
        }
        return s;
    }
};
}  // namespace adaptive

// The loop itself -- the seven-stage step, the error estimate, the controller, the FSAL hand-over, the snapshots and the final
// store -- for any right-hand side: rhs(live, state, deriv) writes d(state)/dt into deriv, in the units of the state.
//   RANKED = false: a plain per-lane loop; the state is kept in normalised units (mom ./ norms) between load and store and rhs
//     sees it so; a lane without a parcel returns at once and `live` is always true.
//   RANKED = true: rhs holds workgroup barriers, so every lane of the workgroup makes the same sequence of calls and the loop
//     runs while ANY lane is active; `live` = the lane's result is wanted (false: a lane without a parcel or one that has
//     finished, which only sits through the barriers); the state is physical.
// g: who shares a controller (adaptive::LaneGroup, adaptive::ColumnGroup above).
// A: the plan constants the loop itself reads (off, np, norm, inv_norm).  u_in / u_out: the plan's planes (they may alias);
// dt_dev (in/out, one double per group: the next proposed dt), t_dev (out: the time reached) and info_dev (out, int32
// [3][g.ctl_ld]: accepted, rejected, status) may each be null.  SAVE: n_save, t_save and u_save (n_save x planes planes of leading dimension
// ld, aliasing neither u_in nor u_out) as above; without it they are not read.
// KEEP0: the right-hand side leaves the number plane of every mode alone (condensation without coalescence: dM0/dt is zero
// identically), so u_out and every snapshot get that plane's value as loaded, not its round trip through the normalised units.
// X: a right-hand side with X scalars of state beside the moments (RANKED = false; the parcel's S, p, T, q_v: adaptive_thermo.hpp)
// is rhs(live, x, state, dx, deriv); the scalars are planes 0 .. X - 1 of u_in / u_out / every snapshot and the plan's planes follow
// them; they are never normalised (abstol_i = abstol in their own units), count in the norms (n_moms), and are advanced, interpolated
// and stored like the rest.
template <int N, int P, typename TIO, bool RANKED, int BS, bool SAVE, bool KEEP0 = false, int X = 0, typename G, typename RHS>
__device__ __forceinline__ void tsit5_adaptive_loop(const KArgs<N, P> &A, const G g, size_t ld, const TIO *u_in, TIO *u_out,
                                                    double t_span, AdaptiveOpts o, double *dt_dev, double *t_dev, int *info_dev,
                                                    size_t n_save, const double *__restrict__ t_save, TIO *__restrict__ u_save,
                                                    RHS rhs_of) {
    using namespace tsit5;
    using St = adaptive::State<N, X>;
    static_assert(X == 0 || !RANKED, "extra state belongs to the per-lane loop");
    static_assert(RANKED || !G::kBarriers, "a sum with barriers belongs to the loop every lane sits through");
    const size_t i = g.i;
    const bool valid = g.valid;
    constexpr bool kRanked = RANKED;
    constexpr bool kNormalisedState = !kRanked;  // see rhs_normalised
    // SAVE: snapshot js of this lane's parcel from v (the units of the state) as the final store writes u -- physical units, the
    // planes a mode has
    size_t planes = X;
#pragma unroll
    for (int m = 0; m < N; ++m) planes += A.np[m] == 3 ? 3 : 2;
    double number_in[N];   // KEEP0: the number planes as loaded
    auto snapshot = [&](size_t js, const St &v) {
#pragma unroll
        for (int q = 0; q < X; ++q) u_save[(js * planes + (size_t)q) * ld + i] = (TIO)v.x[q];
#pragma unroll
        for (int m = 0; m < N; ++m)
#pragma unroll
            for (int q = 0; q < 3; ++q)
                if (q < 2 || A.np[m] == 3) {
                    double x = v.m[m][q];
                    if (kNormalisedState) x *= A.norm[3 * m + q];
                    if constexpr (KEEP0)
                        if (q == 0) x = number_in[m];
                    u_save[(js * planes + (size_t)(X + A.off[m] + q)) * ld + i] = (TIO)x;
                }
    };
    if (!(t_span > 0.0)) {   // (wave- and workgroup-uniform: a kernel argument) nothing to integrate, the planes as they are
        if (!valid) return;
        auto copy = [&](size_t p) {
            const TIO v = u_in[p * ld + i];
            u_out[p * ld + i] = v;
            if (SAVE)   // (every save time is 0)
                for (size_t js = 0; js < n_save; ++js) u_save[(js * planes + p) * ld + i] = v;
        };
#pragma unroll
        for (int q = 0; q < X; ++q) copy((size_t)q);
#pragma unroll
        for (int m = 0; m < N; ++m)
#pragma unroll
            for (int q = 0; q < 3; ++q)
                if (q < 2 || A.np[m] == 3) copy((size_t)(X + A.off[m] + q));
        if (g.leader) {
            if (t_dev) t_dev[g.ctl] = 0.0;
            if (info_dev) info_dev[g.ctl] = 0, info_dev[g.ctl_ld + g.ctl] = 0, info_dev[2 * g.ctl_ld + g.ctl] = ADAPT_DONE;
        }
        return;
    }
    if (!kRanked && !valid) return;
    St u, atol;
    int count = X;
    const bool save0 = SAVE && valid && n_save > 0 && t_save[0] == 0.0;
    size_t j = save0 ? 1 : 0;   // SAVE: the lane's cursor into t_save
#pragma unroll
    for (int q = 0; q < X; ++q) {
        u.x[q] = (double)u_in[(size_t)q * ld + i];
        atol.x[q] = o.abstol;
        if constexpr (SAVE)
            if (save0) u_save[(size_t)q * ld + i] = (TIO)u.x[q];
    }
#pragma unroll
    for (int m = 0; m < N; ++m) {
        const int off = X + A.off[m];
        u.m[m][0] = valid ? (double)u_in[(size_t)(off + 0) * ld + i] : 0.0;
        u.m[m][1] = valid ? (double)u_in[(size_t)(off + 1) * ld + i] : 0.0;
        u.m[m][2] = (valid && A.np[m] == 3) ? (double)u_in[(size_t)(off + 2) * ld + i] : 0.0;
        count += A.np[m] == 3 ? 3 : 2;   // (the planes a mode has: the third slot of a two-moment mode is padding)
        if constexpr (KEEP0) number_in[m] = u.m[m][0];
        if constexpr (SAVE)   // a save time 0: the values as loaded, before any normalisation
            if (save0) {
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    if (q < 2 || A.np[m] == 3) u_save[(size_t)(off + q) * ld + i] = (TIO)u.m[m][q];
            }
        if constexpr (G::kClamp) {
#pragma unroll
            for (int q = 0; q < 3; ++q) u.m[m][q] = u.m[m][q] < 0.0 ? 0.0 : u.m[m][q];
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            if (kNormalisedState) u.m[m][q] = div_by_const(u.m[m][q], A.norm[3 * m + q], A.inv_norm[3 * m + q]);
            atol.m[m][q] = kNormalisedState ? o.abstol : o.abstol * A.norm[3 * m + q];
        }
    }
    const double n_moms = (double)count * (double)g.count;   // components of a group
    // live: the lane's result is wanted (ranked: every lane calls, idle ones sit through the ranking's barriers)
    bool active = valid;
    auto rhs = [&](const St &state, St &deriv) {
        if constexpr (X == 0) rhs_of(valid && active, state.m, deriv.m);
        else rhs_of(valid && active, state.x, state.m, deriv.x, deriv.m);
    };
    St k1, k2, k3, k4, k5, k6, w;
    // where the error combination and k7 go: k2 and k3, which are dead by then -- SAVE keeps k1 .. k7 for the interpolant and
    // gives both an array of its own (not touched, and so not there, without it), or the first none: then k2 stays k2 and the
    // norm forms the combination (kErrInNorm)
    constexpr bool kErrInNorm = SAVE && !G::kOwnErr;
    St ke_own, k7_own;
    St &ke = *[&]() -> St * { if constexpr (SAVE && G::kOwnErr) return &ke_own; else return &k2; }();
    St &k7 = *[&]() -> St * { if constexpr (SAVE) return &k7_own; else return &k3; }();
    rhs(u, k1);
    // ---- the first step
    double dt = dt_dev && valid ? dt_dev[g.ctl] : o.dt_init;
    const bool guess = !(dt > 0.0 && adaptive::is_finite(dt));
    if (G::kBarriers || guess) {   // (a sum with barriers: every lane attends it, whoever uses the result)
        double s0 = 0.0, s1 = 0.0;
        adaptive::counted<N, X>(A.np, [&](double uu, double kk, double at) {
            const double sc = fma(o.reltol, fabs(uu), at);
            const double r0 = uu / sc, r1 = kk / sc;
            s0 = fma(r0, r0, s0);
            s1 = fma(r1, r1, s1);
        }, u, k1, atol);
        s0 = g.sum(s0);
        s1 = g.sum(s1);
        if (guess) {
            const double d0 = sqrt(s0 / n_moms), d1 = sqrt(s1 / n_moms);
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
        if (kRanked) {
            if (!__syncthreads_or(active ? 1 : 0)) break;
        } else if (!active) {
            break;
        }
        const bool last = t + dt >= t_last;
        const double h = last ? t_span - t : dt;
        adaptive::each<N, X>([&](double &ww, double c1, double uu) { ww = fma(h * a21, c1, uu); }, w, k1, u);
        rhs(w, k2);
        adaptive::each<N, X>([&](double &ww, double c1, double c2, double uu) { ww = fma(h, fma(a31, c1, a32 * c2), uu); }, w, k1, k2, u);
        rhs(w, k3);
        adaptive::each<N, X>([&](double &ww, double c1, double c2, double c3, double uu) {
            ww = fma(h, fma(a41, c1, fma(a42, c2, a43 * c3)), uu);
        }, w, k1, k2, k3, u);
        rhs(w, k4);
        adaptive::each<N, X>([&](double &ww, double c1, double c2, double c3, double c4, double uu) {
            ww = fma(h, fma(a51, c1, fma(a52, c2, fma(a53, c3, a54 * c4))), uu);
        }, w, k1, k2, k3, k4, u);
        rhs(w, k5);
        adaptive::each<N, X>([&](double &ww, double c1, double c2, double c3, double c4, double c5, double uu) {
            ww = fma(h, fma(a61, c1, fma(a62, c2, fma(a63, c3, fma(a64, c4, a65 * c5)))), uu);
        }, w, k1, k2, k3, k4, k5, u);
        rhs(w, k6);
        // u_new into w; the k1 .. k6 part of the error estimate into k2, which is dead from here; then k7 into k3 (ke, k7 above)
        // (ke may be k2: the lambda takes its k2 by value)
        adaptive::each<N, X>([&](double &ww, double &ee, double c1, double c2, double c3, double c4, double c5, double c6, double uu) {
            ww = fma(h, fma(a71, c1, fma(a72, c2, fma(a73, c3, fma(a74, c4, fma(a75, c5, a76 * c6))))), uu);
            if constexpr (G::kClamp) ww = ww < 0.0 ? 0.0 : ww;
            if constexpr (!kErrInNorm) ee = err_k1_k6(c1, c2, c3, c4, c5, c6);
        }, w, ke, k1, k2, k3, k4, k5, k6, u);
        rhs(w, k7);
        double s = 0.0;
        adaptive::counted<N, X>(A.np, [&](double c7, double ee, double c1, double c2, double c3, double c4, double c5, double c6, double uu,
                                          double ww, double at) {
            if constexpr (kErrInNorm) ee = err_k1_k6(c1, c2, c3, c4, c5, c6);
            const double err = h * fma(bt7, c7, ee);
            const double sc = fma(o.reltol, fmax(fabs(uu), fabs(ww)), at);
            const double r = err / sc;
            s = fma(r, r, s);
        }, k7, ke, k1, k2, k3, k4, k5, k6, u, w, atol);
        const double eest = sqrt(g.sum(s) / n_moms);
        if (!active) continue;   // (an idle lane of a thresholded plan: it only sat through the barriers)
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
                        snapshot(j, w);
                    } else {
                        double b[7];
                        St v;
                        interp_weights((ts - t) / h, b);
                        adaptive::each<N, X>([&](double &vv, double c1, double c2, double c3, double c4, double c5, double c6, double c7,
                                                 double uu) {
                            vv = fma(h, fma(b[0], c1, fma(b[1], c2, fma(b[2], c3, fma(b[3], c4, fma(b[4], c5, fma(b[5], c6, b[6] * c7)))))),
                                     uu);
                            if constexpr (G::kClamp) vv = vv < 0.0 ? 0.0 : vv;
                        }, v, k1, k2, k3, k4, k5, k6, k7, u);
                        snapshot(j, v);
                    }
                    ++j;
                }
            }
            t = last ? t_span : t + h;
            dt = fmax(h / q, fmin(dt, dt / q));
            qold = fmax(eest, adaptive::kQold0);
            adaptive::each<N, X>([&](double &uu, double &c1, double ww, double c7) { uu = ww, c1 = c7; }, u, k1, w, k7);
            if (last) active = false;   // status 0
        } else {
            ++n_rej;
            dt = h / fmin(1.0 / adaptive::kQmin, q11 / adaptive::kSafety);
        }
    }
    if (!valid) return;
    if constexpr (SAVE) {   // what a parcel stopped by the budget or by dt did not reach (status 0: the cursor is at n_save)
        const TIO nan = (TIO)__builtin_nan("");
        for (; j < n_save; ++j) {
#pragma unroll
            for (int q = 0; q < X; ++q) u_save[(j * planes + (size_t)q) * ld + i] = nan;
#pragma unroll
            for (int m = 0; m < N; ++m)
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    if (q < 2 || A.np[m] == 3) u_save[(j * planes + (size_t)(X + A.off[m] + q)) * ld + i] = nan;
        }
    }
#pragma unroll
    for (int q = 0; q < X; ++q) u_out[(size_t)q * ld + i] = (TIO)u.x[q];
#pragma unroll
    for (int m = 0; m < N; ++m) {
        const int off = X + A.off[m];
        if (kNormalisedState) {
#pragma unroll
            for (int q = 0; q < 3; ++q) u.m[m][q] *= A.norm[3 * m + q];
        }
        if constexpr (KEEP0) u.m[m][0] = number_in[m];
        u_out[(size_t)(off + 0) * ld + i] = (TIO)u.m[m][0];
        u_out[(size_t)(off + 1) * ld + i] = (TIO)u.m[m][1];
        if (A.np[m] == 3) u_out[(size_t)(off + 2) * ld + i] = (TIO)u.m[m][2];
    }
    if (g.leader) {
        if (dt_dev) dt_dev[g.ctl] = dt;
        if (t_dev) t_dev[g.ctl] = t;
        if (info_dev) info_dev[g.ctl] = n_acc, info_dev[g.ctl_ld + g.ctl] = n_rej, info_dev[2 * g.ctl_ld + g.ctl] = status;
    }
}

// cloudy_tsit5_adaptive / cloudy_tsit5_adaptive_saveat: the loop on the coalescence right-hand side of the plan -- rhs_normalised
// where the thresholds are all Inf, rhs_physical (ranked) otherwise.
template <int N, int P, int MODE, typename TIO, bool SPEC = false, int BS = kBlock, bool SAVE = false>
__device__ __forceinline__ void tsit5_adaptive_body(const KArgs<N, P> *__restrict__ Ag, const double *__restrict__ nodes, size_t n,
                                                    size_t ld, const TIO *u_in, TIO *u_out, double t_span, AdaptiveOpts o,
                                                    double *dt_dev, double *t_dev, int *info_dev, size_t n_save = 0,
                                                    const double *__restrict__ t_save = nullptr, TIO *__restrict__ u_save = nullptr) {
    constexpr bool kRanked = MODE != MODE_ALLINF;
    // the plan constants through an opaque zero offset per RHS evaluation (see ssprk33_body); none when compiled for the plan
    tsit5_adaptive_loop<N, P, TIO, kRanked, BS, SAVE>(
        *Ag, adaptive::LaneGroup<BS>(n, ld), ld, u_in, u_out, t_span, o, dt_dev, t_dev, info_dev, n_save, t_save, u_save,
        [&](bool live, const double (&state)[N][3], double (&deriv)[N][3]) {
            size_t oz = 0;
            if (!SPEC) asm volatile("" : "+s"(oz));
            if (!kRanked)
                rhs_normalised<N, P, SPEC>(*(Ag + oz), state, deriv);
            else
                rhs_physical<N, P, MODE, SPEC, BS>(*(Ag + oz), nodes, live, state, deriv);
        });
}

}  // namespace cloudy
