// spectra.hpp -- real-order moments and size spectra of every mode of every parcel (cloudy_moments, cloudy_density): the batch forms of
// moment / partial_moment (ParticleDistributions.jl:177-285) and density / normed_density (:323-416) on the (n, theta, k) of
// load_parcel -- one read of the moments and one closure inversion for all orders or all grid points of a parcel.
//
// One parcel per lane, 256 threads; every store runs along the parcels, so a wave writes 512 contiguous bytes of one plane.  What is
// the same for every lane -- the orders with their scale factors, the grid -- lives where uniform data lives: the orders arrive as a
// small struct kernel argument (SGPRs), the grid is indexed at run time and goes through LDS once per workgroup.
//
//   moments  Gamma / Exponential (k = 1): M_q = n theta^q Gamma(q + k) / Gamma(k).  q = m + f with m = floor(q): M_f from
//            log_gamma_ratio(k, f) (f = 0: n itself), then the exact recurrence M_{q+1} = M_q theta (k + q), m times -- an integral
//            order is products alone, and log_gamma_ratio stays on 0 <= v < 1.  Monodisperse: n theta^q the same way.  Lognormal:
//            n exp(q mu + q^2 sigma^2 / 2).  The orders are uniform: every branch on them is.
//            Up to a cutoff x_t: times P(q + k, x_t / theta) (inc_gamma_p), x_t < theta ? 0 : 1, Phi((ln x_t - mu) / sigma - q sigma)
//            (the closed form of standard_nq_body; the reference integrates with quadgk).  Without a cutoff no such factor is formed.
//            Every per-mode value is rounded on its own before the modes are added (per_mode = 0 has the bits of the sum of the
//            per_mode = 1 planes): the products pass through opaque copies, as in moments_inconsistent (reduce_kernels.hpp).
//   density  per mode the constants ln theta, 1 / theta, k - 1 and c = -ln theta - lgamma_pos(k) stay in registers (Lognormal: mu,
//            1 / (2 sigma^2), -ln sigma - ln(2 pi) / 2), and a grid point costs one exp_fin per mode:
//              Gamma / Exponential  exp((k - 1) (ln x - ln theta) - x / theta + c)       (times n: density)
//              Lognormal            exp(-(ln x - mu)^2 / (2 sigma^2) - ln x + c)
//              Monodisperse         the reference's pulse of half width theta / 10: n / (2 theta / 10) inside, 0 outside
//            n multiplies the exponential (a fallback mode has n = 0: no logarithm of it is taken).  Once per workgroup thread t
//            writes x_j / m0 and ln(x_j / m0) for j = t, t + 256, ... into LDS (16 KB at CLOUDY_MAX_GRID), a negative or NaN x_j as
//            NaN in both; after the one barrier no lane takes a logarithm of a grid value.  x = 0 and an invalid x are uniform
//            branches with the values of the reference's expressions there: Inf, 1 / theta or 0 by the sign of k - 1 (never
//            (k - 1) ln 0 at k = 1), NaN for a Lognormal mode, 0 for a Monodisperse one; NaN in every plane of an invalid point.
//
// This header includes kernels.hpp alone and kernels.hpp does not know it: the text of every other plan-time unit stays as it is.
#pragma once
#include "kernels.hpp"

namespace cloudy {

constexpr int kMaxOrders = 8;    // CLOUDY_MAX_ORDERS
constexpr int kMaxGrid = 1024;   // CLOUDY_MAX_GRID
enum { SPECTRA_DENSITY = 0, SPECTRA_NORMED_DENSITY = 1 };   // CLOUDY_DENSITY, CLOUDY_NORMED_DENSITY

// the orders of a cloudy_moments call: a kernel argument.  scale[j] = n0 m0^q[j] (formed on the host); x_t = x_threshold / m0 and
// its logarithm (partial = 0: not read)
struct MomentArgs {
    int32_t n_orders, partial, per_mode, pad;
    double x_t, ln_x_t;
    double q[kMaxOrders], scale[kMaxOrders];
};
// the grid of a cloudy_density call: scale = n0 / m0 (density) or 1 / m0 (normed density)
struct DensityArgs {
    int32_t n_x, kind, per_mode, pad;
    double m0, scale;
};

namespace spectra {
// a value every lane holds alike, moved to the scalar registers
__device__ __forceinline__ double uniform(double v) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(b & 0xffffffffll));
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
// a product rounded on its own, whatever is added to it afterwards (-ffp-contract=fast fuses in the instruction selector)
__device__ __forceinline__ double rounded(double v) {
    asm volatile("" : "+v"(v));
    return v;
}
}  // namespace spectra

template <int N, int P, typename TIO>
__device__ __forceinline__ void spectra_moments_body(const KArgs<N, P> &A, const MomentArgs &a, size_t n, size_t ld,
                                                     const TIO *__restrict__ in, TIO *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double nn[N], th[N], kk[N], lnth[N];
    load_parcel<N, P, TIO>(A, i, ld, in, nn, th, kk);
#pragma unroll
    for (int m = 0; m < N; ++m) lnth[m] = A.dist_type[m] == DIST_LOGNORMAL ? th[m] : log_pos(th[m]);
#pragma unroll 1
    for (int j = 0; j < a.n_orders; ++j) {
        const double q = a.q[j], scale = a.scale[j];
        const double whole = floor(q), f = q - whole;
        const int steps = (int)whole;
        double sum = 0.0;
#pragma unroll
        for (int m = 0; m < N; ++m) {
            const int dtp = A.dist_type[m];
            double mom, part = 1.0;
            if (dtp == DIST_LOGNORMAL) {
                const double sg = kk[m];
                mom = nn[m] * exp_fin(fma(q, th[m], 0.5 * (q * q) * (sg * sg)));
                if (a.partial) part = norm_cdf((a.ln_x_t - th[m]) / sg - q * sg);
            } else {
                const double k = dtp == DIST_GAMMA ? kk[m] : 1.0;
                if (dtp == DIST_MONO) {
                    mom = f == 0.0 ? nn[m] : nn[m] * exp_fin(f * lnth[m]);
#pragma unroll 1
                    for (int s = 0; s < steps; ++s) mom *= th[m];
                    if (a.partial) part = a.x_t < th[m] ? 0.0 : 1.0;
                } else {
                    mom = f == 0.0 ? nn[m] : nn[m] * exp_fin(fma(f, lnth[m], log_gamma_ratio(k, f)));
                    const double kf = k + f;
#pragma unroll 1
                    for (int s = 0; s < steps; ++s) mom *= th[m] * (kf + double(s));
                    if (a.partial) {
                        const double aq = q + k;
                        part = inc_gamma_p(aq, a.x_t / th[m], a.ln_x_t - lnth[m], lgamma_pos(aq + 1.0), nullptr);
                    }
                }
            }
            if (a.partial) mom *= part;
            const double v = spectra::rounded(mom * scale);
            if (a.per_mode) st_stream(out + ((size_t)m * a.n_orders + j) * ld + i, v);
            else sum += v;
        }
        if (!a.per_mode) st_stream(out + (size_t)j * ld + i, sum);
    }
}

template <int N, int P, typename TIO>
__device__ __forceinline__ void spectra_density_body(const KArgs<N, P> &A, const DensityArgs &a, size_t n, size_t ld,
                                                     const TIO *__restrict__ in, const double *__restrict__ x_dev,
                                                     TIO *__restrict__ out) {
    __shared__ double sh_x[kMaxGrid], sh_lx[kMaxGrid];
    const double nan = __builtin_nan("");
    const int n_x = a.n_x < kMaxGrid ? a.n_x : kMaxGrid;
    for (int j = threadIdx.x; j < n_x; j += kBlock) {
        const double x = x_dev[j];
        const bool ok = x >= 0.0;   // (false for NaN)
        const double xn = x / a.m0;
        sh_x[j] = ok ? xn : nan;
        sh_lx[j] = ok ? log(xn) : nan;   // (ln 0 = -Inf: x = 0 takes a branch of its own below)
    }
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double nn[N], th[N], kk[N];
    load_parcel<N, P, TIO>(A, i, ld, in, nn, th, kk);
    // per mode: w = the factor in front of the exponential; c0 .. c3 = (ln theta, 1 / theta, k - 1, c), Lognormal (mu, 1 / (2 sigma^2),
    // unused, c), Monodisperse (theta, theta / 10, unused, the pulse's height over w)
    double w[N], c0[N], c1[N], c2[N], c3[N];
    const bool normed = a.kind == SPECTRA_NORMED_DENSITY;
#pragma unroll
    for (int m = 0; m < N; ++m) {
        const int dtp = A.dist_type[m];
        w[m] = (normed ? 1.0 : nn[m]) * a.scale;
        if (dtp == DIST_LOGNORMAL) {
            const double sg = kk[m];
            c0[m] = th[m];
            c1[m] = 1.0 / (2.0 * (sg * sg));
            c2[m] = 0.0;
            c3[m] = -log_pos(sg) - 0.91893853320467274;
        } else if (dtp == DIST_MONO) {
            c0[m] = th[m];
            c1[m] = th[m] / 10.0;
            c2[m] = 0.0;
            c3[m] = 1.0 / (2.0 * th[m] / 10.0);
        } else {
            const double k = dtp == DIST_GAMMA ? kk[m] : 1.0;
            c0[m] = log_pos(th[m]);
            c1[m] = 1.0 / th[m];
            c2[m] = k - 1.0;
            c3[m] = -c0[m] - (dtp == DIST_GAMMA ? lgamma_pos(k) : 0.0);
        }
    }
    const int M = a.per_mode ? N : 1;
#pragma unroll 1
    for (int j = 0; j < n_x; ++j) {
        const double x = spectra::uniform(sh_x[j]), lx = spectra::uniform(sh_lx[j]);
        double sum = 0.0;
#pragma unroll
        for (int m = 0; m < N; ++m) {
            const int dtp = A.dist_type[m];
            double f;
            if (x > 0.0) {
                if (dtp == DIST_MONO) {
                    f = fabs(x - c0[m]) < c1[m] ? c3[m] : 0.0;
                } else {
                    const double l = lx - c0[m];
                    double e = dtp == DIST_LOGNORMAL ? fma(-(l * l), c1[m], c3[m] - lx) : fma(c2[m], l, fma(-x, c1[m], c3[m]));
                    // (exp_fin takes finite arguments: beyond +-800 the result is 0 or Inf either way; a NaN stays one)
                    e = e < -800.0 ? -800.0 : e;
                    e = e > 800.0 ? 800.0 : e;
                    f = exp_fin(e);
                }
            } else if (x == 0.0) {
                if (dtp == DIST_MONO) f = 0.0;
                else if (dtp == DIST_LOGNORMAL) f = nan;
                else f = c2[m] > 0.0 ? 0.0 : c2[m] < 0.0 ? INFINITY : c2[m] == 0.0 ? exp_fin(c3[m]) : nan;
            } else {
                f = nan;
            }
            const double v = spectra::rounded(w[m] * f);
            if (a.per_mode) st_stream(out + ((size_t)j * M + m) * ld + i, v);
            else sum += v;
        }
        if (!a.per_mode) st_stream(out + (size_t)j * ld + i, sum);
    }
}

}  // namespace cloudy
