/*
 * cloudy_hip.h -- C ABI of libcloudy_hip.so: the MI355X (gfx950) batched collision-coalescence
 * moment-tendency operator for Cloudy.jl.
 *
 * Drop-in boundary.  Each entry point replaces one Julia-level interface of CliMA/Cloudy.jl v0.6.0
 * (file:line relative to the reference checkout) for a batch of independent 0-D parcels; the
 * Julia-side `ccall` binding a maintainer would add is shown in INTEGRATION.md.
 *
 *   cloudy_plan_create            <- CoalescenceData(kernel, NProgMoms, dist_thresholds, norms, ts)
 *                                    src/Sources/Coalescence.jl:55-104  (+ the ODE_parameters NamedTuple
 *                                    test/examples/Analytical/box_gamma_mixture.jl:29-35)
 *   cloudy_coal_rhs               <- rhs!(dm, m, par, t) = rhs_coal!(AnalyticalCoalStyle(), dm, m, par, ts)
 *                                    test/examples/utils/box_model_helpers.jl:22-53
 *   cloudy_get_coal_ints          <- get_coal_ints(::AnalyticalCoalStyle, pdists, coal_data[, ::MovingThreshold])
 *                                    src/Sources/Coalescence.jl:115-185
 *   (coal_style = CLOUDY_NUMERICAL_COAL: the same two entry points are
 *    rhs_coal!(NumericalCoalStyle(), dm, m, par, ts) with par.kernel_func, box_model_helpers.jl:47-48, and
 *    get_coal_ints(::NumericalCoalStyle, pdists, kernel_func), src/Sources/Coalescence.jl:470-489 -- the reference's
 *    nested adaptive quadgk replaced by a fixed Gauss rule (cloudy_plan_desc.quad_order) or, with quad_mode =
 *    CLOUDY_QUAD_CONVERGED, by closed forms + one 1-D rule per mode that reach quadgk's answer to <= 1e-8 of scale --
 *    the GUARANTEED bound, asserted on the device against the golden values; measured <= 5.5e-10)
 *   cloudy_update_dist_from_moments <- update_dist_from_moments(pdist, moments)
 *                                    src/ParticleDistributions/ParticleDistributions.jl:456-476, 512-523
 *   cloudy_finite_2d_integrals    <- get_finite_2d_integrals / moment_source_helper
 *                                    src/Sources/Coalescence.jl:200-244, ParticleDistributions.jl:567-612
 *   cloudy_compute_thresholds     <- compute_thresholds(pdists, percentiles)
 *                                    src/ParticleDistributions/ParticleDistributions.jl:734-761
 *   cloudy_sedimentation_flux     <- get_sedimentation_flux(pdists, vel)   src/Sources/Sedimentation.jl:22-37
 *   cloudy_rainshaft_sources      <- the per-cell body of make_rainshaft_rhs
 *                                    test/examples/utils/rainshaft_helpers.jl:52-78
 *   cloudy_rainshaft_rhs          <- rhs(m, p, t) of make_rainshaft_rhs incl. the flux divergence
 *                                    test/examples/utils/rainshaft_helpers.jl:45-89
 *   cloudy_rainshaft_ssprk33_steps <- solve(ODEProblem(make_rainshaft_rhs(...), m, tspan, p), SSPRK33(), dt = p.dt),
 *                                    test/examples/Analytical/rainshaft_gamma_mixture.jl:59-60
 *   cloudy_standard_N_q           <- get_standard_N_q(pdists, size_cutoff)  ParticleDistributions.jl:634-687
 *   cloudy_moments                <- moment(dist, q) / partial_moment(dist, q, x_threshold) at real q, every mode
 *                                    ParticleDistributions.jl:177-218, 226-285
 *   cloudy_density                <- density(dist, x) / normed_density(dist, x) on a grid of masses, every mode
 *                                    ParticleDistributions.jl:323-416
 *   cloudy_cond_evap              <- rhs_condensation!(dmom, mom, p, s) / get_cond_evap
 *                                    test/examples/utils/box_model_helpers.jl:55-67, src/Sources/Condensation.jl:22-37
 *   cloudy_ssprk33_steps          <- solve(ODEProblem(rhs, m0, tspan, p), SSPRK33(), dt = p.dt) of the drivers,
 *                                    test/examples/Analytical/box_single_gamma.jl:35-36 (OrdinaryDiffEq stepping)
 *   cloudy_tsit5_steps            <- solve(prob, Tsit5(), dt = ..., adaptive = false) (BASELINE configs[0]; OrdinaryDiffEq tableau)
 *   cloudy_box_ssprk33_steps      <- solve(ODEProblem(rhs!, ...), SSPRK33(), dt = ...) with rhs! = rhs_condensation! (or the sum
 *                                    of rhs_coal! and it), test/examples/Analytical/condensation_single_gamma.jl:28,
 *                                    condensation_exp_gamma.jl:31
 *   cloudy_parcel_rhs             <- parcel_model_cloudy(dY, Y, p, t), test/examples/Analytical/parcel_example.jl:15-85, with the
 *                                    distributions updated from the current moments (see the entry point)
 *   cloudy_parcel_ssprk33_steps   <- solve(ODEProblem(parcel_model_cloudy, Yinit, tspan, p), SSPRK33(), dt = const_dt), :104-111
 *   cloudy_rainshaft_cond_rhs     <- rhs(m, p, t) of make_rainshaft_rhs (test/examples/utils/rainshaft_helpers.jl:45-89) plus
 *                                    get_cond_evap of each cell (src/Sources/Condensation.jl:22-37, as rhs_condensation!,
 *                                    test/examples/utils/box_model_helpers.jl:55-67): the three sources of a column
 *   cloudy_rainshaft_cond_ssprk33_steps <- solve(ODEProblem(that rhs, m, tspan, p), SSPRK33(), dt = p.dt), the stepping of
 *                                    test/examples/Analytical/rainshaft_gamma_mixture.jl:59-60 with the third source
 *   cloudy_moment_sums            <- moments_sum diagnostic, test/examples/utils/plotting_helpers.jl:240-252
 *   cloudy_moment_sums_allreduce  <- the same summed over the ranks / GPUs that share a batch (RCCL; the reference is
 *                                    single-process, its global sum is the local one)
 *
 * Data layout (all batched calls): moment-major structure-of-arrays, element (q, parcel) at
 * base[q * ld + parcel], ld >= n_parcels -- exactly Julia's column-major m[parcel, moment]
 * (test/examples/utils/rainshaft_helpers.jl:48-56).  Plane q is the flat moment index of
 * get_dist_moment_ind (src/helper_functions.jl:13-20), 0-based.  Values are in physical units;
 * normalisation by norms happens inside, as in rhs_coal!.
 *
 * Ownership: the caller owns every buffer; a plan owns only its constant block and a small reduction
 * workspace (used by cloudy_moment_sums: do not run that call concurrently on ONE plan from several
 * streams -- cloudy_moment_sums_ws takes the workspace from the caller and is re-entrant; every other batched
 * call only reads the plan and may run concurrently).
 *
 * Devices: a plan belongs to the device it was created on (desc.device, or the caller's current device): its constant
 * block, node tables and plan-time compiled code objects live there.  Every batched call makes that device current
 * for the duration of the call and restores the caller's current device before returning, as does
 * cloudy_plan_create; `stream` and all buffers must belong to the plan's device.  No call allocates, except the
 * host-pointer convenience cloudy_coal_rhs_host.  All device entry points are asynchronous on `stream` (a hipStream_t passed as
 * void*; NULL = the default stream).  Errors: int status, never a C++ exception; the message
 * of the last failure on the calling thread is cloudy_last_error().
 *
 * Plain C: no HIP or torch types appear in any signature.
 */
#ifndef CLOUDY_HIP_H
#define CLOUDY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CLOUDY_HIP_VERSION 100 /* 0.1.0 */

#define CLOUDY_MAX_MODES 8  /* N: number of sub-distributions */
#define CLOUDY_MAX_P 8      /* P = tensor order + 1 */
/* Plans of up to CLOUDY_AOT_MAX_MODES modes and order <= 4 (P <= CLOUDY_AOT_MAX_P; the reference's examples stop at 4
 * modes and order 4, box_gamma_mixture_4modes.jl:23, box_gamma_mixture_hydro.jl:23) have ahead-of-time compiled kernels
 * behind every entry point.  Larger plans (the reference's types bound neither N nor the order, Coalescence.jl:55-104, and
 * get_coal_ints(::NumericalCoalStyle) is generic in the number of modes, :470-489) run kernels compiled for the plan with hiprtc: the RHS / rainshaft / integrator kernels at
 * cloudy_plan_create (CLOUDY_EUNSUPPORTED there when plan-time compilation is off or fails -- there is no other path), the
 * per-mode diagnostics and the parameter-plane entry points (cloudy_update_dist_from_moments, cloudy_get_coal_ints,
 * cloudy_get_finite_2d_integrals, cloudy_compute_thresholds, cloudy_sedimentation_flux, cloudy_cond_evap_rhs,
 * cloudy_standard_N_q) on their first call.  A NumericalCoalStyle plan takes up to CLOUDY_MAX_MODES modes as well (round 5; 15 to
 * 40 s of compilation per kernel for 5 to 8 modes, cached on disk; the order of its "tensor" is 0: P = 1). */
#define CLOUDY_AOT_MAX_MODES 4
#define CLOUDY_AOT_MAX_P 5
#define CLOUDY_MAX_VEL 4    /* terms of the terminal-velocity power series */
#define CLOUDY_MAX_MOMENTS (3 * CLOUDY_MAX_MODES)
#define CLOUDY_MAX_SAVE_TIMES 4096 /* save times of one cloudy_tsit5_adaptive_saveat call */
/* the sources cloudy_box_ssprk33_steps integrates (bits of its `sources` argument) */
#define CLOUDY_SRC_COAL 1 /* collision-coalescence, rhs_coal! */
#define CLOUDY_SRC_COND 2 /* condensation / evaporation, rhs_condensation! */

/* distribution families, ParticleDistributions.jl:66-159.  Parameter planes are (n, theta, k); Monodisperse uses
 * (n, theta), Lognormal keeps (n, mu, sigma) in the same three slots. */
enum { CLOUDY_DIST_EXPONENTIAL = 0, CLOUDY_DIST_GAMMA = 1, CLOUDY_DIST_MONODISPERSE = 2, CLOUDY_DIST_LOGNORMAL = 3 };
/* EquationTypes.jl:20-22 */
enum { CLOUDY_FIXED_THRESHOLD = 0, CLOUDY_MOVING_THRESHOLD = 1 };
enum { CLOUDY_F64 = 0, CLOUDY_F32 = 1, CLOUDY_F32_FAST = 2, CLOUDY_F64_RELAXED = 3 };
/* EquationTypes.jl:15-16 */
enum { CLOUDY_ANALYTICAL_COAL = 0, CLOUDY_NUMERICAL_COAL = 1 };
/* CoalescenceKernelFunction families, KernelFunctions.jl:39-86; parameters in cloudy_plan_desc.kernel_func_params:
 * (coll_coal_rate) | (coll_coal_rate) | (coal_eff) | (x_threshold, coal_rate_below_threshold, coal_rate_above_threshold) */
enum { CLOUDY_KFUNC_CONSTANT = 0, CLOUDY_KFUNC_LINEAR = 1, CLOUDY_KFUNC_HYDRODYNAMIC = 2, CLOUDY_KFUNC_LONG = 3 };
#define CLOUDY_MAX_QUAD 32  /* points of the fixed Gauss rule per distribution */
/* cloudy_plan_desc.quad_mode: how a NumericalCoalStyle plan evaluates the integrals of Coalescence.jl:503-708.
 * FIXED: one quad_order-point Gauss rule per distribution (BASELINE configs[3] as worded: "10-pt Gauss quadrature").
 * CONVERGED: the integrals split along the non-smooth sets of the kernel function, converged to the reference's
 * quadgk(rtol = 1e-8) answer (DESIGN.md 3.6 states the measured error and cost). */
enum { CLOUDY_QUAD_FIXED = 0, CLOUDY_QUAD_CONVERGED = 1 };
/* layout of cloudy_plan_desc.kernel_c */
enum { CLOUDY_KERNEL_SINGLE = 0 /* [P][P] shared by all pairs, Coalescence.jl:89-104 */,
       CLOUDY_KERNEL_MATRIX = 1 /* [N][N][P][P], Coalescence.jl:55-87 */ };

enum {
    CLOUDY_OK = 0,
    CLOUDY_EINVAL = -1,       /* bad argument (the reference throws in a constructor) */
    CLOUDY_ENOTSYMMETRIC = -2,/* check_symmetry failed, KernelTensors.jl:157-171 */
    CLOUDY_EHIP = -3,         /* HIP runtime error (message has hipGetErrorString) */
    CLOUDY_ENOMEM = -4,
    CLOUDY_EUNSUPPORTED = -5, /* valid in the reference, outside this build */
    CLOUDY_ENODEVICE = -6,
    CLOUDY_ECOMM = -7         /* RCCL error (message has ncclGetErrorString) */
};

typedef struct cloudy_plan cloudy_plan;

typedef struct cloudy_plan_desc {
    uint32_t struct_size;                    /* sizeof(cloudy_plan_desc); set by cloudy_plan_desc_init */
    int32_t n_modes;                         /* N = length(pdists) */
    int32_t dist_type[CLOUDY_MAX_MODES];     /* type of p.pdists[i]; NProgMoms[i] = nparams (2 / 3) */
    int32_t tensor_p;                        /* P = order + 1 */
    int32_t kernel_layout;                   /* CLOUDY_KERNEL_SINGLE / _MATRIX */
    int32_t kernel_is_normalized;            /* 0: library applies get_normalized_kernel_tensor(c, norms) */
    const double *kernel_c;                  /* c[a][b] multiplies x^a y^b (KernelTensors.jl:44-52); row-major */
    double dist_thresholds[CLOUDY_MAX_MODES];/* FixedThreshold: mass in physical units (divided by norms[1] inside,
                                                Coalescence.jl:78-84); MovingThreshold: percentiles. +INFINITY ok. */
    int32_t threshold_style;
    double norms[2];                         /* (n0, m0), helper_functions.jl:40-53 */
    double k_range[2];                       /* param_range.k, ParticleDistributions.jl:459; default (eps, 10) */
    int32_t n_bins_per_log_unit;             /* ParticleDistributions.jl:594; default 15 */
    int32_t dtype;                           /* element type of the mom / dmom / flux planes: CLOUDY_F64, or CLOUDY_F32
                                                (float planes in HBM = half the traffic; arithmetic stays fp64 in
                                                registers; (n, theta, k) / F diagnostics planes are always fp64), or
                                                CLOUDY_F32_FAST (float planes AND single-precision arithmetic: in the
                                                per-node Simpson / incomplete-gamma pass of threshold plans -- ~1e-6
                                                relative on the thresholded integrals; and, for plans WITHOUT a
                                                threshold compiled for the plan, in the whole cloudy_coal_rhs kernel
                                                (packed v_pk_fma_f32, four parcels per lane): <= 1e-2 of scale,
                                                99.9 % of parcels <= 1e-4, median 1e-8, and parcels whose closure is
                                                clamped to k = eps may come out Inf / NaN where fp64 arithmetic stays
                                                finite.  Every layout of a batch takes that arithmetic (16-byte
                                                accesses where ld % 4 == 0 and the planes are aligned, scalar ones
                                                otherwise: same bits).  cloudy_ssprk33_steps / cloudy_tsit5_steps of
                                                such a plan run fp64 arithmetic on the float planes (~2e-7): their
                                                right-hand side is more accurate than cloudy_coal_rhs of the same
                                                plan; use CLOUDY_F32 where the two must agree), or
                                                CLOUDY_F64_RELAXED (fp64 planes and arithmetic; the power series and the
                                                continued fraction of the incomplete gamma function of the threshold
                                                plans stop at 1e-11 instead of 1e-17 / 1e-16: <= 1e-9 of scale against
                                                the oracle, an order inside north_star's 1e-8 for this path; opt-in;
                                                plan-time compiled kernels only -- the ahead-of-time kernels, and plans
                                                without a threshold, compute as CLOUDY_F64) */
    int32_t n_vel;                           /* 0 = no sedimentation term */
    double vel[CLOUDY_MAX_VEL][2];           /* p.vel: terminal velocity sum_k vel[k][0] * x^vel[k][1], physical units */
    int32_t device;                          /* HIP device ordinal, -1 = current */
    int32_t specialize;                      /* plan-time compilation (hiprtc) of the cloudy_coal_rhs kernel (and, for
                                                all-Inf thresholds, the cloudy_ssprk33_steps kernel) with the plan as
                                                compile-time constants: 0 = when available (default; the
                                                environment variable CLOUDY_HIP_JIT=0 turns it off), 1 = required
                                                (plan creation fails otherwise), -1 = off */
    /* ---- NumericalCoalStyle plans (make_box_model_rhs(NumericalCoalStyle()), Coalescence.jl:470-708) ----
     * coal_style = CLOUDY_NUMERICAL_COAL: the integrals of the kernel FUNCTION p.kernel_func over the densities, where
     * the reference nests adaptive quadgk(rtol = 1e-8).  quad_mode = CLOUDY_QUAD_CONVERGED (THE DEFAULT: the drop-in
     * answers within north_star's 1e-8 of the reference): the integrals split along the kernel function's non-smooth
     * sets -- closed forms for Q and R, one ADAPTIVE Gauss-Kronrod (7, 15) rule per mode for the weighting_fn split
     * (panels walked from large sizes down, bisected until |K15 - G7| <= 1e-7 of the accumulated value -- every kernel
     * function since round 5: the Long kernel's panel above x_t, where G(s) ~ (s - x_t)^k, is integrated in xi with
     * s - x_t ~ xi^4, its range [x_t, 2 x_t] in a second phase from a per-rule incomplete-beta table -- and ended by a
     * rigorous bound of what is left; quad_order is then only the points per panel of the inner rule a Lognormal mode's
     * self-collision integral needs under the hydrodynamic or Long kernel, default 8).  ERROR: the guaranteed bound is
     * 1e-8 of scale against nested adaptive quadrature of the reference integrals (asserted on the device on the golden
     * cases); measured <= 5.5e-10 there, and <= 1.1e-10 against the same rule at 1e-13 over a thousand random multi-scale
     * mixtures (a statement about the rule's convergence, not about the reference integrals).  Lognormal modes: under the
     * constant / linear kernels the inner integral is a trapezoidal rule of step min(sigma, 1/2) (<= 2e-13 of the density's
     * peak, any sigma); under the hydrodynamic / Long kernels it takes Gauss-Legendre panels of at most 3 sigma (up to 256):
     * <= 1.5e-12 of scale down to sigma = 0.003, 1e-9 ... 2e-6 at sigma = 0.001, growing below
     * (csrc/quad_conv.hpp).  quad_mode = CLOUDY_QUAD_FIXED (explicit opt-in; BASELINE configs[3] "via 10-pt Gauss
     * quadrature"): each integral by one fixed quad_order-point Gauss rule per distribution (generalised Gauss-Laguerre
     * for Gamma / Exponential modes, Gauss-Hermite in ln x for Lognormal modes; tensor product over a pair of modes after
     * the substitution x' = x - y; default 10 points) -- exact for the constant and linear kernels up to the weighting_fn
     * split, a discretisation for the hydrodynamic and Long kernels (1e-4 ... 4e-2 of scale at 10 points), several
     * times faster.  kernel_c, tensor_p,
     * dist_thresholds and threshold_style are ignored (the style has no thresholds: weighting_fn splits the self
     * collisions, Coalescence.jl:624-642).  Monodisperse modes: CLOUDY_EINVAL (no normed_density_func method).
     * Shape parameters: the per-parcel Gauss-Laguerre rules are staged for 0 < k <= max(k_range[1], 1), the range
     * update_dist_from_moments can produce.  (n, theta, k) planes handed to cloudy_get_coal_ints with a Gamma k outside
     * that range give NaN tendencies for the parcel (a batch cannot fail per parcel): widen k_range[1] instead. */
    int32_t coal_style;                      /* CLOUDY_ANALYTICAL_COAL (default) / CLOUDY_NUMERICAL_COAL */
    int32_t kernel_func;                     /* CLOUDY_KFUNC_* */
    int32_t kernel_func_is_normalized;       /* 0: library applies get_normalized_kernel_func(kernel, norms), :124-154 */
    int32_t quad_order;                      /* FIXED: points per distribution; CONVERGED: Gauss-Legendre points per
                                                panel; 2..CLOUDY_MAX_QUAD; 0 (default) = 10 (FIXED) / 8 (CONVERGED) */
    double kernel_func_params[3];            /* physical units unless kernel_func_is_normalized */
    int32_t thresholds_are_normalized;       /* FixedThreshold only: 1 = dist_thresholds are already divided by norms[1],
                                                i.e. the CoalescenceData.dist_thresholds FIELD (Coalescence.jl:78-84) rather
                                                than the constructor argument -- a host that builds the plan from an
                                                existing CoalescenceData passes its fields through unchanged */
    int32_t quad_mode;                       /* NumericalCoalStyle: CLOUDY_QUAD_CONVERGED (default) / CLOUDY_QUAD_FIXED */
} cloudy_plan_desc;

/* fills defaults: k_range = (eps, 10), n_bins_per_log_unit = 15, norms = (1, 1), thresholds = +Inf,
 * dtype = F64, device = -1, coal_style = ANALYTICAL, quad_mode = CONVERGED, quad_order = 0 (the mode's default) */
void cloudy_plan_desc_init(cloudy_plan_desc *desc);

int cloudy_plan_create(const cloudy_plan_desc *desc, cloudy_plan **out);
void cloudy_plan_destroy(cloudy_plan *plan);
/* 1 if cloudy_coal_rhs / cloudy_ssprk33_steps of this plan run kernels compiled for it at plan creation, else 0 with
 * the reason (or the compiler log) in cloudy_plan_jit_log.  Either way the arithmetic is the same (results agree to
 * rounding, bit for bit in most configurations). */
int cloudy_plan_specialized(const cloudy_plan *plan);
const char *cloudy_plan_jit_log(const cloudy_plan *plan);
/* Build check without a GPU: validates `desc`, generates the plan's specialised translation unit(s) and compiles them
 * with hiprtc for `arch` (NULL = "gfx950"); nothing is loaded or launched.  CLOUDY_OK, or CLOUDY_EUNSUPPORTED with the
 * compiler log in cloudy_last_error().  arch = "source-only": every translation unit of the plan is generated and none compiled
 * (the host-side sanitizer run of the tests). */
int cloudy_jit_selfcheck(const cloudy_plan_desc *desc, const char *arch);
/* Layout of cloudy_plan_desc as this library was compiled: for each field, in declaration order, name / byte offset /
 * byte size.  A binding in another language (julia/CloudyHIP.jl, the ctypes mirror) checks its own struct against this
 * before the first cloudy_plan_create.  Returns the number of fields; fills at most `cap` entries of each array (any of
 * which may be NULL).  Names are static strings. */
int cloudy_plan_desc_layout(const char **names, uint32_t *offsets, uint32_t *sizes, int cap);
/* The per-parcel Gauss rule of the NumericalCoalStyle kernels, evaluated on the HOST by the same source the device
 * compiles (quad.hpp: start values from the staged table, two Newton steps, Christoffel weights): nodes u[quad_order]
 * and normalised weights W[quad_order] for the weight u^(k-1) e^-u / Gamma(k), 0 < k <= k_hi.  A diagnostic for tests
 * and hosts (no device involved, nothing batched: this is not a compute path). */
int cloudy_quad_rule_host(int quad_order, double k_hi, double k, double *u, double *W);
int cloudy_plan_nmom(const cloudy_plan *plan);      /* sum(NProgMoms) */
int cloudy_plan_device(const cloudy_plan *plan);    /* HIP device ordinal the plan lives on */
int cloudy_plan_nparams(const cloudy_plan *plan);   /* 3 * N planes of (n, theta, k) */
/* copies of the derived CoalescenceData fields (Coalescence.jl:69-84), for tests and hosts */
int cloudy_plan_get(const cloudy_plan *plan, int32_t *N_mom_max, int32_t *N_2d_ints /*[N]*/,
                    double *thresholds /*[N]*/, double *kernel_c_normalized /*[N][N][P][P]*/,
                    double *mom_norms /*[nmom]*/);

/* dmom = d(mom)/dt by collision-coalescence; mom, dmom: nmom planes, physical units. */
int cloudy_coal_rhs(const cloudy_plan *plan, size_t n_parcels, size_t ld, const void *mom_dev, void *dmom_dev,
                    void *stream);
/* same through host buffers (allocates a staging buffer, copies, synchronises): convenience only */
int cloudy_coal_rhs_host(const cloudy_plan *plan, size_t n_parcels, size_t ld, const void *mom_host,
                         void *dmom_host);

/* n_steps explicit SSPRK33 steps of du/dt = rhs!(u) with fixed dt, the integrator of every reference driver
 * (solve(prob, SSPRK33(), dt = ...), test/examples/Analytical/box_single_gamma.jl:35-36), fused around the RHS:
 * each parcel's moments stay in registers over all stages and steps (one read + one write of the state per call,
 * no per-stage launches).  u_out_dev may equal u_in_dev.  NumericalCoalStyle plans are served as well (the Numerical
 * drivers integrate the same way, test/examples/Numerical/n_particles_gamma.jl:39-40).  Plans without a finite threshold
 * keep the state in normalised units (mom ./ norms) between load and store: the stage values differ from rhs!'s
 * normalise-in-every-call sequence by roundings only. */
int cloudy_ssprk33_steps(const cloudy_plan *plan, size_t n_parcels, size_t ld, const void *u_in_dev, void *u_out_dev,
                         double dt, int n_steps, void *stream);

/* n_steps explicit steps of the Tsit5 tableau (Tsitouras 2011; OrdinaryDiffEq's Tsit5()) with FIXED dt, fused around the
 * RHS like cloudy_ssprk33_steps (state and the six stage derivatives in registers, 6 RHS evaluations per step, FSAL).
 * BASELINE configs[0] names Tsit5 for the single-box Golovin case; no reference driver uses it (all of them call
 * solve(prob, SSPRK33(), dt = ...)), and OrdinaryDiffEq's adaptive step control uses a global error norm over the state,
 * which a batch of independent parcels does not have: this is the tableau applied per parcel with the caller's dt
 * (cloudy_tsit5_adaptive below controls the step per parcel, with a per-parcel norm).
 * Served for every plan cloudy_ssprk33_steps serves (round 4): AnalyticalCoalStyle with thresholds Inf (state kept in
 * normalised units between load and store), fixed or MovingThreshold, and NumericalCoalStyle in either quad_mode; fp64 or
 * float planes (CLOUDY_F32_FAST: CLOUDY_EUNSUPPORTED).  The kernel is compiled for the plan on the first call
 * (cloudy_jit_tsit5_* / cloudy_jit_quad_tsit5_*); without hiprtc the tensor plans run the ahead-of-time kernel and a
 * NumericalCoalStyle plan answers CLOUDY_EUNSUPPORTED. */
int cloudy_tsit5_steps(const cloudy_plan *plan, size_t n_parcels, size_t ld, const void *u_in_dev, void *u_out_dev,
                       double dt, int n_steps, void *stream);

/* Per-parcel ADAPTIVE Tsit5: every parcel is advanced from t = 0 to t = t_span with the 5(4) pair of the Tsit5 tableau under a
 * step-size controller of its own (csrc/adaptive.hpp).  Each parcel of a batch is its own ODE, so each lane carries its own t, dt
 * and error estimate: a batch whose number concentrations span decades is advanced by one model time step without a common dt, and
 * the caller learns what happened to every parcel.  (cloudy_tsit5_steps is the same tableau with one fixed dt for the batch.)
 *   error norm   err_i = h sum_j btilde_j k_j,i; sc_i = abstol + reltol max(|u_i|, |u_new,i|); EEst = sqrt(mean_i (err_i/sc_i)^2) over
 *                the parcel's prognostic moments.  abstol is in the plan's NORMALISED units (mom ./ norms: the units in which every
 *                moment of a plan is O(1)); reltol is relative.
 *   controller   a PI controller with these constants -- beta1 = 7/50, beta2 = 2/25, gamma = 9/10, qmin = 1/5, qmax = 10,
 *                qold_0 = 1e-4: q11 = EEst^beta1, q = clamp(q11 / qold^beta2 / gamma, 1/qmax, 1/qmin).  With h the step tried (h = dt
 *                but for the last step): EEst <= 1 accepts -- t += h, dt <- max(h / q, min(dt, dt / q)), qold <- max(EEst, qold_0);
 *                otherwise the step is rejected -- dt <- h / min(1/qmin, q11 / gamma), an estimate that is not finite divides h by
 *                5.  For h = dt the accept rule is dt / q.  It is specified here and in csrc/adaptive.hpp, not by reference to
 *                another solver: no bit identity with a run of OrdinaryDiffEq's Tsit5() is claimed.
 *   last step    t + dt >= t_span (1 - 4 eps): the step tried is h = t_span - t and t lands on t_span exactly.  The accept rule
 *                above then lets dt shrink as the shorter step's estimate asks but not grow past what that step supports, so the
 *                dt that goes out is a proposal for a full step, not the remainder of the last one.
 *   first step   dt_dev[i] where dt_dev is given and the value positive and finite, else opts->dt_init where positive, else Hairer's
 *                first guess 0.01 ||u||_sc / ||f(u)||_sc (t_span where f = 0); capped at t_span.
 * Outputs, each optional (NULL) but the state: u_out_dev (may equal u_in_dev); dt_dev, one fp64 value per parcel, in/out -- the next
 * proposed dt, so that a host model calling once per model step starts warm; t_dev, one fp64 value per parcel -- the time reached;
 * info_dev, int32 [3][ld] -- the planes accepted steps, rejected steps, status:
 *   0  reached t_span (t_dev[i] == t_span exactly);   1  accepted + rejected reached opts->max_steps;
 *   2  dt fell below 1e-14 t_span or is not finite.
 * A parcel that stops early keeps the state and time it reached.  max_steps is mandatory and bounds the work of a launch.
 * Argument checks precede any device work, the plan last (CLOUDY_EINVAL): opts NULL or of another struct_size; reltol <= 0,
 * abstol < 0, a value of opts that is not finite, dt_init < 0; t_span < 0 or not finite; max_steps outside [1, 1000000];
 * ld < n_parcels; a NULL state with n_parcels > 0; plan NULL.  n_parcels = 0 returns CLOUDY_OK at once; t_span = 0 copies the input
 * to the output with status 0 and zero counts.
 * Served: AnalyticalCoalStyle plans with thresholds Inf (state in normalised units between load and store), fixed or MovingThreshold
 * (the workgroup re-ranks its parcels in every evaluation; a finished parcel's lane sits through the barriers), CLOUDY_F64 /
 * CLOUDY_F64_RELAXED / CLOUDY_F32 planes (state and control in fp64 registers either way), up to CLOUDY_MAX_MODES modes.
 * Deliberate limits (CLOUDY_EUNSUPPORTED; cloudy_tsit5_steps is the alternative): NumericalCoalStyle plans, CLOUDY_F32_FAST planes,
 * and plans without plan-time compilation (specialize = -1, or hiprtc unavailable) -- the kernel is compiled for the plan on the
 * first call (cloudy_jit_adaptive_tsit5_*) and has no ahead-of-time instance. */
typedef struct cloudy_adaptive_opts {
    uint32_t struct_size; /* sizeof(cloudy_adaptive_opts), set by cloudy_adaptive_opts_init */
    double reltol;        /* 1e-6 */
    double abstol;        /* 1e-9, normalised units */
    double dt_init;       /* 0: automatic */
    int32_t max_steps;    /* 10000: accepted + rejected, per parcel */
} cloudy_adaptive_opts;
void cloudy_adaptive_opts_init(cloudy_adaptive_opts *opts);
int cloudy_tsit5_adaptive(const cloudy_plan *plan, size_t n_parcels, size_t ld, const void *u_in_dev, void *u_out_dev,
                          double t_span, const cloudy_adaptive_opts *opts, double *dt_dev, double *t_dev, int32_t *info_dev,
                          void *stream);

/* cloudy_tsit5_adaptive with DENSE OUTPUT: the same integration -- the same kernel body, controller and step sequence per parcel;
 * u_out_dev, dt_dev, t_dev and info_dev have the bits cloudy_tsit5_adaptive gives -- and the state of every parcel at the n_save
 * batch-wide times t_save.  A caller that needs the state at common times (output intervals, coupling sub-steps) gets them from one
 * launch, and no step is clamped at a save time: where one looks does not change the steps taken.
 *   interpolant  the free 4th-order interpolant of the Tsit5 pair over the seven stage derivatives of the accepted step t -> t + h that
 *                holds the save time: u(t + th h) = u + h sum_i b_i(th) k_i, i = 1 .. 7, th = (t_save[j] - t) / h in (0, 1], with
 *                  b1 = -1.0530884977290216 th (th - 1.3299890189751412)(th^2 - 1.4364028541716351 th + 0.7139816917074209)
 *                  b2 =  0.1017 th^2 (th^2 - 2.1966568338249754 th + 1.2949852507374631)
 *                  b3 =  2.490627285651252793 th^2 (th^2 - 2.38535645472061657 th + 1.57803468208092486)
 *                  b4 = -16.54810288924490272 th^2 (th - 1.21712927295533244)(th - 0.61620406037800089)
 *                  b5 =  47.37952196281928122 th^2 (th - 1.203071208372362603)(th - 0.658047292653547382)
 *                  b6 = -34.87065786149660974 th^2 (th - 1.2)(th - 0.666666666666666667)
 *                  b7 =  2.5 th^2 (th - 1)(th - 0.6)
 *                It costs no evaluation of the right-hand side and is not seen by the controller: reltol and abstol bound the error
 *                at the ends of the steps, and inside a step the error of the interpolant (O(h^5), as the local error of the
 *                step) adds to it.
 *   save times   t_save: a HOST pointer to n_save doubles, finite, within [0, t_span], strictly increasing, n_save <=
 *                CLOUDY_MAX_SAVE_TIMES.  The library checks them and uploads them on `stream` into scratch the plan owns (allocated
 *                by the first such call -- not inside a stream capture); calls on several streams are ordered among themselves by an
 *                event.  n_save = 0 (t_save, u_save_dev may be NULL) is cloudy_tsit5_adaptive.
 *   layout       u_save_dev: n_save * planes planes of leading dimension ld in the plan's plane type, planes = cloudy_plan_nmom:
 *                snapshot j, plane p, parcel i at u_save_dev[(j * planes + p) * ld + i], physical units.  It must not overlap
 *                u_in_dev or u_out_dev.  Columns n_parcels .. ld are not written.
 *   NaN rule     a parcel that stops with status 1 or 2 has a quiet NaN in every plane of every snapshot with t_save[j] beyond the
 *                time it reached; its other snapshots hold what it passed.
 *   bit-equal    a snapshot at t_save[j] == 0 holds the bits of u_in_dev; a snapshot at t_save[j] == t_span those of u_out_dev
 *                (of a parcel with status 0).  More generally a save time that is the end of an accepted step gets that step's
 *                u_new, not the interpolant at th = 1.  t_span = 0: every snapshot is the input.
 * Argument checks precede any device work, the plan last (CLOUDY_EINVAL, the message names the argument): n_save above the cap;
 * t_save or u_save_dev NULL with n_save > 0; an entry of t_save that is not finite, below 0 or above t_span; entries that do not
 * strictly increase; then those of cloudy_tsit5_adaptive.  Served and refused (CLOUDY_EUNSUPPORTED, nothing is written) exactly
 * as cloudy_tsit5_adaptive: the second kernel of the same plan-time unit (cloudy_jit_dense_tsit5_*). */
int cloudy_tsit5_adaptive_saveat(const cloudy_plan *plan, size_t n_parcels, size_t ld, const void *u_in_dev, void *u_out_dev,
                                 double t_span, const cloudy_adaptive_opts *opts, double *dt_dev, double *t_dev, int32_t *info_dev,
                                 void *stream, size_t n_save, const double *t_save, void *u_save_dev);

/* n_steps SSPRK33 steps of du/dt = [coal](u) + [cond](u; s, xi) with fixed dt, fused like cloudy_ssprk33_steps: a lane keeps its
 * parcel's state in registers over all stages and steps, the state is read once and written once per call and the parcel's
 * supersaturation is loaded once.  [cond] is rhs_condensation!(dmom, mom, p, s) (test/examples/utils/box_model_helpers.jl:55-67
 * -> get_cond_evap, src/Sources/Condensation.jl:22-37) and s_dev / s / xi mean what they mean in cloudy_cond_evap: s_dev holds
 * one fp64 value per parcel or is NULL to use the scalar `s`; xi = p.xi in physical units (rho_l = 1000).
 *   sources = CLOUDY_SRC_COND: `solve(prob, SSPRK33(), dt = ODE_parameters.dt)` with rhs! = rhs_condensation! of
 *     test/examples/Analytical/condensation_single_gamma.jl:28 and condensation_exp_gamma.jl:31 in one launch; every plan
 *     cloudy_cond_evap serves, NumericalCoalStyle plans included (nothing of the coalescence data is read);
 *   sources = CLOUDY_SRC_COAL | CLOUDY_SRC_COND: both sources from ONE closure inversion per stage; AnalyticalCoalStyle plans
 *     with thresholds Inf, fixed or MovingThreshold, CLOUDY_F64 / CLOUDY_F64_RELAXED / CLOUDY_F32 planes, up to CLOUDY_MAX_MODES
 *     modes; a NumericalCoalStyle plan answers CLOUDY_EUNSUPPORTED (step it stage by stage: cloudy_coal_rhs + cloudy_cond_evap);
 *   sources = CLOUDY_SRC_COAL: forwards to cloudy_ssprk33_steps (the same kernel, the same bits).
 * The kernels with the condensation source are compiled for the plan on the first call that needs them (cloudy_jit_box_*);
 * without plan-time compilation such a call answers CLOUDY_EUNSUPPORTED with the compiler's log.  That holds for
 * CLOUDY_SRC_COND alone as well, a deliberate limit: cloudy_cond_evap has ahead-of-time kernels, this integrator has none (they
 * would be a third family of translation units), so a plan created with specialize = -1 steps condensation stage by stage
 * with cloudy_cond_evap, and steps coalescence alone here or with cloudy_ssprk33_steps.  CLOUDY_F32_FAST:
 * CLOUDY_EUNSUPPORTED.  u_out_dev may equal u_in_dev; n_steps = 0 copies the input to the output. */
int cloudy_box_ssprk33_steps(const cloudy_plan *plan, size_t n_parcels, size_t ld, const void *u_in_dev, void *u_out_dev,
                             int sources, const double *s_dev, double s, double xi, double dt, int n_steps, void *stream);

/* Per-parcel ADAPTIVE Tsit5 of the box with condensation: du/dt = [coal](u) + [cond](u; s, xi) from t = 0 to t = t_span, every
 * parcel under a step-size controller of its own (csrc/adaptive_box.hpp).  The box a host model advances per model step is this
 * sum -- what cloudy_box_ssprk33_steps integrates with one fixed dt -- and condensation is the source whose time scale differs
 * most from parcel to parcel: the supersaturation is a per-parcel input of either sign, and x^(2/3) of an evaporating mode falls
 * linearly in t.  The only change to the mathematics of cloudy_tsit5_adaptive is the right-hand side.
 *   sources, s_dev, s, xi   what they mean in cloudy_box_ssprk33_steps: [cond] is rhs_condensation!(dmom, mom, p, s)
 *                (test/examples/utils/box_model_helpers.jl:55-67 -> get_cond_evap, src/Sources/Condensation.jl:22-37); s_dev holds
 *                one fp64 value per parcel (loaded once per parcel) or is NULL to use the scalar `s`; xi = p.xi in physical units.
 *   t_span .. stream   what they mean in cloudy_tsit5_adaptive: its controller, error norm, first-step rule, last-step rule,
 *                statuses and abstol units, stated there and not again here.
 *   n_save, t_save, u_save_dev   every rule of cloudy_tsit5_adaptive_saveat: a host pointer, its checks, its layout, its NaN rule
 *                and its bit-equal rule; n_save = 0 with NULL pointers means "no snapshots".
 *   sources = CLOUDY_SRC_COAL: forwards to cloudy_tsit5_adaptive / cloudy_tsit5_adaptive_saveat (the same kernel, the same bits,
 *     the same refusals);
 *   sources = CLOUDY_SRC_COND: every plan cloudy_cond_evap serves, NumericalCoalStyle plans included; nothing of the coalescence
 *     data is read, the state is kept in normalised units, a plain per-lane loop without a barrier;
 *   sources = CLOUDY_SRC_COAL | CLOUDY_SRC_COND: AnalyticalCoalStyle plans, both sources from ONE closure inversion per
 *     evaluation.  Thresholds all Inf: a per-lane loop, normalised state.  Fixed or MovingThreshold: physical state, the
 *     workgroup re-ranks its parcels in every evaluation and the loop runs while any of its lanes is active.  A
 *     NumericalCoalStyle plan answers CLOUDY_EUNSUPPORTED (step it stage by stage: cloudy_coal_rhs + cloudy_cond_evap).
 * Behaviour after a mode has evaporated completely is not specified (max_steps bounds the loop whatever happens).
 * Argument checks precede any device work, the plan last (CLOUDY_EINVAL, the message names the argument): those of
 * cloudy_tsit5_adaptive_saveat in its order, then sources outside {COAL, COND, COAL | COND} and xi NaN, then the plan.
 * Plane types as cloudy_box_ssprk33_steps: CLOUDY_F64 / CLOUDY_F64_RELAXED / CLOUDY_F32 (state and control in fp64 registers
 * either way); CLOUDY_F32_FAST: CLOUDY_EUNSUPPORTED.  The kernels are compiled for the plan on the first call that needs them
 * (cloudy_jit_box_adaptive_*, one with and one without snapshots per source set) and have no ahead-of-time instance: without
 * plan-time compilation the call answers CLOUDY_EUNSUPPORTED with the compiler's log.  A refusal writes nothing. */
int cloudy_box_tsit5_adaptive(const cloudy_plan *plan, size_t n_parcels, size_t ld, const void *u_in_dev, void *u_out_dev,
                              int sources, const double *s_dev, double s, double xi, double t_span,
                              const cloudy_adaptive_opts *opts, double *dt_dev, double *t_dev, int32_t *info_dev, void *stream,
                              size_t n_save, const double *t_save, void *u_save_dev);

/* The adiabatic parcel of test/examples/Analytical/parcel_example.jl: Y = (S, p, T, q_v, mom[0..nmom)) -- saturation ratio over
 * liquid water, pressure, temperature, vapour specific humidity and the plan's moments (physical units, the plan's plane order) --
 * rising at speed w.  With the constants below:
 *   R_m(q_t, q_l)  = R_d (1 + (R_v/R_d - 1) q_t - (R_v/R_d) q_l)          cp_m(q_t, q_l) = cp_d + (cp_v - cp_d) q_t + (cp_l - cp_v) q_l
 *   L(T)           = LH_v0 + (cp_v - cp_l)(T - T_0)
 *   p_vs(T)        = press_triple (T/T_triple)^((cp_v-cp_l)/R_v) exp((LH_v0 - (cp_v-cp_l) T_0)/R_v (1/T_triple - 1/T))
 *   xi(T)          = 1 / ( L/(K_therm T) (L/(R_v T) - 1) + R_v T / (D_vapor p_vs) )
 *   rho0 = p / (R_m(q_v, 0) T);  q_l = sum_modes M1_mode / rho0;  R = R_m(q_v + q_l, q_l);  cp = cp_m(q_v + q_l, q_l);  rho = p / (R T)
 *   a1 = L g/(cp T^2 R_v) - g/(R T);  a2 = 1/q_v;  a3 = L^2/(R_v T^2 cp)
 *   dmom = get_cond_evap(update_dist_from_moments(mom), S - 1, xi(T), rho_l);  dq_l = sum_modes dmom[M1_mode] / rho
 *   dS = a1 w S - (a2 + a3) S dq_l;  dp = -p g w/(R T);  dT = -g w/cp + L dq_l/cp;  dq_v = -dq_l
 * (Thermodynamics.jl / CloudMicrophysics.jl, which the driver takes these from, are not part of the reference tree: the closure
 * is stated here in full.)  The driver as written binds `pdists` (:19) before it rebuilds p.pdists (:55-61), so its get_cond_evap
 * sees the INITIAL distributions at every call; these entry points use the distributions updated from the current moments, as
 * every other right-hand side of the reference does.
 * The defaults of cloudy_parcel_params_init are ClimaParams' values as recalled -- ClimaParams is not part of the reference tree,
 * so they could not be verified against it: R_d = 8.3144598/0.02897, R_v = 8.3144598/0.018015, cp_d = R_d 7/2, cp_v = 1859,
 * cp_l = 4181, LH_v0 = 2.5008e6, T_0 = 273.16, press_triple = 611.657, T_triple = 273.16, grav = 9.81, K_therm = 2.4e-2,
 * D_vapor = 2.26e-5, rho_l = 1000. */
typedef struct cloudy_parcel_params {
    uint32_t struct_size; /* sizeof(cloudy_parcel_params), set by cloudy_parcel_params_init */
    double R_d, R_v, cp_d, cp_v, cp_l, LH_v0, T_0, press_triple, T_triple, grav, K_therm, D_vapor, rho_l;
} cloudy_parcel_params;
void cloudy_parcel_params_init(cloudy_parcel_params *params);

/* y: 4 + nmom fp64 planes of leading dimension ld -- planes 0..3 are S, p, T, q_v, plane 4 + q is the plan's moment plane q.
 * w_dev: one updraft speed per parcel (fp64), or NULL to use the scalar `w`.
 *   sources = CLOUDY_SRC_COND: every plan cloudy_cond_evap serves, Monodisperse and NumericalCoalStyle plans included (nothing
 *     of the coalescence data is read);
 *   sources = CLOUDY_SRC_COAL | CLOUDY_SRC_COND: the coalescence tendency added to the moments' (AnalyticalCoalStyle plans
 *     whose thresholds are all Inf), from the same closure inversion.
 * cloudy_parcel_rhs: one evaluation of dY into dy_dev (same layout).  cloudy_parcel_ssprk33_steps: n_steps SSPRK33 steps with
 * fixed dt, fused like cloudy_box_ssprk33_steps -- state in registers over all stages and steps, read once and written once, w
 * loaded once, xi(T) formed per stage on the device; y_out_dev may equal y_in_dev, n_steps = 0 copies, n_parcels = 0 returns
 * CLOUDY_OK at once.
 * Argument checks precede any device work (CLOUDY_EINVAL): params NULL or of another struct_size, a constant that is not
 * positive (NaN included), sources without CLOUDY_SRC_COND, n_steps < 0, dt NaN, ld < n_parcels, plan NULL.
 * Deliberate limits (CLOUDY_EUNSUPPORTED; step such a parcel stage by stage with cloudy_cond_evap / cloudy_coal_rhs and
 * cloudy_parcel_thermo_host): COAL | COND on plans with finite or moving thresholds and on NumericalCoalStyle plans; CLOUDY_F32 /
 * CLOUDY_F32_FAST planes (S - 1 of 1e-3 does not survive a float plane).  CLOUDY_SRC_COAL alone is CLOUDY_EINVAL: it is not a
 * parcel, cloudy_ssprk33_steps exists for it.  The kernels are compiled for the plan on first use (cloudy_jit_parcel_*); without
 * plan-time compilation the calls answer CLOUDY_EUNSUPPORTED with the compiler's log, as cloudy_box_ssprk33_steps does. */
int cloudy_parcel_rhs(const cloudy_plan *plan, size_t n_parcels, size_t ld, const void *y_dev, const double *w_dev, double w,
                      const cloudy_parcel_params *params, int sources, void *dy_dev, void *stream);
int cloudy_parcel_ssprk33_steps(const cloudy_plan *plan, size_t n_parcels, size_t ld, const void *y_in_dev, void *y_out_dev,
                                int sources, const double *w_dev, double w, const cloudy_parcel_params *params, double dt,
                                int n_steps, void *stream);
/* Per-parcel ADAPTIVE Tsit5 of the adiabatic parcel: dY/dt above from t = 0 to t = t_span, every parcel under a step-size
 * controller of its own (csrc/adaptive_thermo.hpp).  The parcel's fastest time scale is the relaxation of the supersaturation,
 * about 1 / (4 pi D_vapor N r) -- 2 s for the driver's N = 2e8, a tenth of that at 2e9 -- and it moves as the droplets grow: a
 * batch whose droplet numbers and updraft speeds span a decade each has no common dt that is both safe and cheap.  It is the
 * loop of cloudy_tsit5_adaptive on the right-hand side of cloudy_parcel_ssprk33_steps (the updated-distribution form, xi(T) formed
 * per evaluation, the moments in normalised units between load and store).
 *   y_in_dev, y_out_dev, sources, w_dev, w, params   what they mean in cloudy_parcel_ssprk33_steps, the layout included: 4 + nmom
 *                fp64 planes of leading dimension ld; y_out_dev may equal y_in_dev.
 *   t_span .. stream   what they mean in cloudy_tsit5_adaptive: tableau, PI controller and its constants, first-step rule,
 *                last-step rule, statuses 0 / 1 / 2, max_steps, dt_dev in/out for a warm start -- stated there, not again here.
 *   error norm   EEst = sqrt(mean_i (err_i / sc_i)^2) over the 4 + nmom prognostic components, sc_i = abstol_i + reltol
 *                max(|y_i|, |y_new,i|).  The moments: abstol_i = abstol in the plan's normalised units (mom ./ norms), as for every
 *                plan whose thresholds are all Inf.  S, p, T, q_v: abstol_i = abstol in their own units.  Consequence: p (~1e5) and
 *                T (~3e2) are controlled relatively, S (~1) to reltol + abstol, and q_v (~1e-2) to max(reltol, abstol / q_v).
 *   n_save, t_save, y_save_dev   every rule of cloudy_tsit5_adaptive_saveat: a host pointer, its checks, its NaN rule, its bit-equal
 *                rules at 0, at t_span and at step ends, the plan-owned save-time scratch; n_save = 0 with NULL pointers means "no
 *                snapshots".  y_save_dev holds snapshot j, plane p, parcel i at [(j * (4 + nmom) + p) * ld + i], fp64, physical
 *                units; it overlaps neither y_in_dev nor y_out_dev; columns n_parcels .. ld are not written.
 *   sources = CLOUDY_SRC_COND: dM0/dt is zero identically -- the number planes of y_out_dev and of every snapshot carry the bits
 *     of the input.
 * n_parcels = 0: CLOUDY_OK at once.  t_span = 0: a copy, status 0, zero counts, every snapshot is the input.
 * Argument checks precede any device work, the plan last (CLOUDY_EINVAL, the message names the argument): those of
 * cloudy_tsit5_adaptive_saveat in its order, then those of cloudy_parcel_ssprk33_steps (params NULL or of another struct_size, a
 * constant that is not positive, sources without CLOUDY_SRC_COND), then the plan.
 * Deliberate limits (CLOUDY_EUNSUPPORTED, nothing written; step such a parcel stage by stage with cloudy_cond_evap /
 * cloudy_coal_rhs and cloudy_parcel_thermo_host): those of cloudy_parcel_ssprk33_steps -- COAL | COND on plans with finite or
 * moving thresholds and on NumericalCoalStyle plans; CLOUDY_F32 / CLOUDY_F32_FAST planes.  The kernels are compiled for the plan on
 * the first call that needs them (cloudy_jit_parcel_adaptive_*, one with and one without snapshots per source set) and have no
 * ahead-of-time instance: without plan-time compilation the call answers CLOUDY_EUNSUPPORTED with the compiler's log. */
int cloudy_parcel_tsit5_adaptive(const cloudy_plan *plan, size_t n_parcels, size_t ld, const void *y_in_dev, void *y_out_dev,
                                 int sources, const double *w_dev, double w, const cloudy_parcel_params *params, double t_span,
                                 const cloudy_adaptive_opts *opts, double *dt_dev, double *t_dev, int32_t *info_dev, void *stream,
                                 size_t n_save, const double *t_save, void *y_save_dev);
/* the closure alone, on the host (the same source as the kernels'): out = (rho, R, cp, L, p_vs, xi, a1, a3) for a state
 * (S, p, T, q_v) and m_liq = the sum of the modes' mass moments in physical units */
int cloudy_parcel_thermo_host(const cloudy_parcel_params *params, double S, double p, double T, double q_v, double m_liq,
                              double out[8]);

/* inner operator on given distributions: params = 3N planes (n, theta, k) per mode, normalised units
 * (k plane ignored for exponential modes); out = nmom planes, normalised units. */
int cloudy_get_coal_ints(const cloudy_plan *plan, size_t n_parcels, size_t ld, const void *params_dev,
                         void *coal_ints_dev, void *stream);

/* Batched validity diagnostic of the closure inversion (round 6): counts_host[4 * mode + c] = the number of parcels whose mode
 *   c = 0: took the fallback distribution (0, 1, 1) (moments at or below eps; ParticleDistributions.jl:461, :473-475, :495, :519);
 *   c = 1: has its shape at the lower clamp (Gamma: k = k_range[0], :459-469; Lognormal: sigma = eps, :499-502);
 *   c = 2: has its shape at the upper clamp (Gamma: k = k_range[1]);
 *   c = 3: fails check_moment_consistency (ParticleDistributions.jl:437-449) -- a negative moment, or a negative second central
 *          moment -- evaluated on the normalised moments the closure sees (box_model_helpers.jl:30-31).
 * The reference can only raise per call or clamp silently; a batch of 1e7 parcels cannot throw per parcel, so the counts are the
 * batch form of both.  mom_dev: the plan's plane type, physical units, as cloudy_coal_rhs.  Synchronises `stream`; counts_host
 * has 4 * n_modes entries (host memory). */
int cloudy_closure_stats(const cloudy_plan *plan, size_t n_parcels, size_t ld, const void *mom_dev, uint64_t *counts_host,
                         void *stream);

/* closure inversion: mom (physical) -> params planes (n, theta, k), normalised units */
int cloudy_update_dist_from_moments(const cloudy_plan *plan, size_t n_parcels, size_t ld, const void *mom_dev,
                                    void *params_dev, void *stream);

/* F[i][p1][p2] of get_finite_2d_integrals: N*M*M planes (M = P+2), row-major (i, p1, p2) */
int cloudy_finite_2d_integrals(const cloudy_plan *plan, size_t n_parcels, size_t ld, const void *params_dev,
                               void *F_dev, void *stream);

/* per-parcel thresholds actually used by the S terms: N planes (last = +Inf) */
int cloudy_compute_thresholds(const cloudy_plan *plan, size_t n_parcels, size_t ld, const void *params_dev,
                              void *thresholds_dev, void *stream);

/* sedimentation flux of every prognostic moment, physical units (plan must have n_vel > 0) */
int cloudy_sedimentation_flux(const cloudy_plan *plan, size_t n_parcels, size_t ld, const void *mom_dev,
                              void *flux_dev, void *stream);

/* condensation / evaporation tendency of every prognostic moment, rhs_condensation!(dmom, mom, p, s)
 * (test/examples/utils/box_model_helpers.jl:55-67 -> get_cond_evap, src/Sources/Condensation.jl:22-37).
 * xi = p.xi in physical units; supersaturation s per parcel (s_dev, fp64, n values) or, if s_dev is NULL, `s`. */
int cloudy_cond_evap(const cloudy_plan *plan, size_t n_parcels, size_t ld, const void *mom_dev, const double *s_dev,
                     double s, double xi, void *dmom_dev, void *stream);

/* cloud / rain diagnostics get_standard_N_q(pdists, size_cutoff) (ParticleDistributions.jl:634-687): 4 planes
 * (N_liq, N_rai, M_liq, M_rai) in physical units; size_cutoff in physical mass units (the examples pass 1e-6 kg). */
int cloudy_standard_N_q(const cloudy_plan *plan, size_t n_parcels, size_t ld, const void *mom_dev, double size_cutoff,
                        void *nq_dev, void *stream);

/* Real-order moments and size spectra of every mode of every parcel, one launch each: what a host model evaluates around a
 * microphysics step (effective radius from M_2/3 and M_1, reflectivity from M_2, fall speed from M_1+1/6, their rain-only forms
 * with a cutoff, the spectra the reference's drivers plot, test/examples/utils/plotting_helpers.jl:104).
 * mom_dev as for cloudy_standard_N_q: the plan's planes, physical units, the plan's plane type; outputs in the plan's plane type
 * and in physical units.  Both calls serve tensor plans and NumericalCoalStyle plans of up to CLOUDY_MAX_MODES modes and every
 * plane type, and run kernels compiled for the plan with hiprtc (no ahead-of-time instance: CLOUDY_EUNSUPPORTED where plan-time
 * compilation is off or failed).  Arguments that need no plan are checked first (CLOUDY_EINVAL, the message names the argument),
 * then the plan; a refused call writes nothing. */
#define CLOUDY_MAX_ORDERS 8
#define CLOUDY_MAX_GRID 1024
enum { CLOUDY_DENSITY = 0, CLOUDY_NORMED_DENSITY = 1 };

/* moment(dist, q) (ParticleDistributions.jl:177-218), or, with a finite x_threshold, partial_moment(dist, q, x_threshold)
 * (:226-285), of every mode of every parcel at n_orders real orders (1 .. CLOUDY_MAX_ORDERS host values, each finite and within
 * [0, 16]).  x_threshold: physical mass, positive; +Inf: the full moment (no incomplete gamma function is evaluated).
 * out_dev: M * n_orders planes of leading dimension ld, M = n_modes if per_mode (1), else 1 (0); plane m * n_orders + j holds
 * mode m, order j; with per_mode = 0 plane j is the sum over the modes in mode order, formed in fp64 from the per-mode values.
 * On the (n, theta, k) of the closure inversion, times n0 m0^q:
 *   Gamma / Exponential (k = 1)  n theta^q Gamma(q + k) / Gamma(k)        up to x_t: times P(q + k, x_t / theta)
 *   Monodisperse                 n theta^q                                 x_t < theta ? 0 : the full moment
 *   Lognormal                    n exp(q mu + q^2 sigma^2 / 2)             times Phi((ln x_t - mu - q sigma^2) / sigma)
 * (the Lognormal partial moment in closed form, as cloudy_standard_N_q: the reference integrates with quadgk, :255-269).  A
 * fallback mode (0, 1, 1) gives 0 at every order.  cloudy_standard_N_q is orders (0, 1) at one cutoff, summed over the modes. */
int cloudy_moments(const cloudy_plan *plan, size_t n_parcels, size_t ld, const void *mom_dev, int n_orders, const double *orders,
                   double x_threshold, int per_mode, void *out_dev, void *stream);

/* density(dist, x) (kind = CLOUDY_DENSITY) or normed_density(dist, x) (CLOUDY_NORMED_DENSITY) (ParticleDistributions.jl:323-416)
 * of every mode of every parcel on a grid of n_x masses (1 .. CLOUDY_MAX_GRID device doubles, physical mass): n0 / m0 (1 / m0) times
 * the normalised (normed) density at x / m0.  out_dev: n_x * M planes, M as above; plane j * M + m holds grid point j, mode m;
 * per_mode = 0 sums the densities of the modes (CLOUDY_NORMED_DENSITY takes per_mode = 1 only).  The formulas are the reference's
 * (:323-388), the Monodisperse density its pulse of half width theta / 10; a plan with a Monodisperse mode has no normed density
 * (CLOUDY_EINVAL, as the reference has no method).  A negative or NaN grid value gives a quiet NaN in every plane of that grid
 * point and nowhere else: the batch form of error("Density can only be evaluated at nonnegative values.").  At x = 0 the value is
 * the one the reference's expressions give: Inf (Gamma, k < 1), n / theta (Exponential; Gamma, k = 1), 0 (Gamma, k > 1;
 * Monodisperse; a fallback Gamma or Exponential mode), NaN (Lognormal). */
int cloudy_density(const cloudy_plan *plan, size_t n_parcels, size_t ld, const void *mom_dev, int kind, size_t n_x,
                   const double *x_dev, int per_mode, void *out_dev, void *stream);

/* coalescence source and sedimentation flux of each cell in one fused pass
 * (negative moments clamped to zero, empty cells skipped) */
int cloudy_rainshaft_sources(const cloudy_plan *plan, size_t n_cells, size_t ld, const void *mom_dev,
                             void *coal_source_dev, void *sedi_flux_dev, void *stream);

/* the full right-hand side of make_rainshaft_rhs (rainshaft_helpers.jl:45-89) for n_columns columns of nz cells
 * (cell index fastest, bottom to top): coalescence source + upwind divergence of the sedimentation flux,
 * rhs[i] = coal[i] - (flux[i+1] - flux[i]) / dz with zero flux above the top cell.  flux_work_dev: nmom planes of
 * scratch (holds the cell fluxes on return).  One launch for columns of up to 1024 cells when the plan's kernels are compiled
 * for it (a workgroup holds whole columns, the flux of the cell above travels through LDS), the cell kernel and a divergence
 * launch otherwise; the same bits on fp64 planes (float planes: the one launch does not round the fluxes in between). */
int cloudy_rainshaft_rhs(const cloudy_plan *plan, size_t nz, size_t n_columns, size_t ld, const void *mom_dev, double dz,
                         void *flux_work_dev, void *rhs_dev, void *stream);

/* n_steps SSPRK33 steps of the rainshaft right-hand side above for n_columns independent columns of nz <= 1024 cells
 * (what `solve(ODEProblem(rhs, m, tspan, p), SSPRK33(), dt = p.dt)` does in rainshaft_single_gamma.jl:52-53,
 * rainshaft_gamma_mixture.jl:59-60), in ONE launch: a workgroup owns whole columns, the state stays in registers over
 * all stages and steps (parked in LDS across the Simpson passes of a thresholded plan) and the upwind flux of the cell above
 * is exchanged through LDS.  As in the reference, every RHS
 * evaluation first clamps negative moments of its argument to zero in place (rainshaft_helpers.jl:52), including the
 * FSAL evaluation on each step's result, so the returned state is clamped.  u_out_dev may equal u_in_dev.
 * A workgroup of 256, 512 or 1024 threads holds floor(threads / nz) whole columns; the kernel compiled for the plan picks the
 * size by nz (512 threads for the reference's 20 cells; results do not depend on it), the ahead-of-time kernel has 256 threads
 * and nz <= 256 (256 < nz <= 1024 without hiprtc: CLOUDY_EUNSUPPORTED).  nz > 1024 (round 5; the reference's cell
 * loop is unbounded in nz, rainshaft_helpers.jl:55-78): the same steps stage by stage on the stream -- cloudy_rainshaft_rhs and
 * one update launch per stage, three stream-ordered scratch arrays of the state's size per call -- not fused, any nz. */
int cloudy_rainshaft_ssprk33_steps(const cloudy_plan *plan, size_t nz, size_t n_columns, size_t ld,
                                   const void *u_in_dev, void *u_out_dev, double dz, double dt, int n_steps,
                                   void *stream);

/* The column right-hand side with all three sources, for columns through air with a supersaturation profile (rain that
 * evaporates below the cloud layer).  One evaluation on n_columns independent columns of nz cells is
 *     clamp m to >= 0                                              (rainshaft_helpers.jl:52)
 *     f = coal_source(m) [skipped for empty cells, :67-72]
 *       + upwind divergence of the sedimentation flux              (as cloudy_rainshaft_rhs, :80-86)
 *       + get_cond_evap(update_dist_from_moments(m), s_cell, xi)   (Condensation.jl:22-37, as cloudy_cond_evap on the clamped m)
 * summed in this order.  The condensation term is formed for every cell from the same closure inversion as the other two (an
 * empty cell's fallback distribution gives zero).  s_dev holds one fp64 supersaturation per cell in the cell order of the state
 * (cell col * nz + iz; always fp64, whatever the plane type), constant over the call, or is NULL to use the scalar `s`; xi and
 * rho_l = 1000 as in cloudy_cond_evap.  flux_work_dev as in cloudy_rainshaft_rhs.  With s = 0 or xi = 0 the result equals
 * cloudy_rainshaft_rhs's.
 * One launch for columns of up to 1024 cells: the kernels are compiled for the plan on the first call that needs them
 * (cloudy_jit_rainshaft_cond_*, one unit per workgroup size of 256 / 512 / 1024 threads, picked as cloudy_rainshaft_rhs picks);
 * there are no ahead-of-time instances, so without plan-time compilation such a call answers CLOUDY_EUNSUPPORTED with the
 * compiler's log.  Where no workgroup can hold a column -- nz > 1024, LDS rows of the plan that fit no workgroup size that
 * holds a column, MovingThreshold plans (which these two entries accept, unlike cloudy_rainshaft_rhs) -- the library runs the
 * unfused form: the cell kernel, the divergence launch, a cloudy_cond_evap launch on a clamped copy and an add, with two scratch
 * arrays of the state's size per call.
 * Refusals: NULL plan, NaN xi, nz < 1, dz <= 0, a plan without terminal-velocity terms: CLOUDY_EINVAL; NumericalCoalStyle plans
 * and CLOUDY_F32_FAST planes: CLOUDY_EUNSUPPORTED (CLOUDY_F64, CLOUDY_F64_RELAXED and CLOUDY_F32 are served). */
int cloudy_rainshaft_cond_rhs(const cloudy_plan *plan, size_t nz, size_t n_columns, size_t ld, const void *mom_dev,
                              const double *s_dev, double s, double xi, double dz, void *flux_work_dev, void *rhs_dev,
                              void *stream);

/* n_steps SSPRK33 steps of that right-hand side with fixed dt: cloudy_rainshaft_ssprk33_steps with the third source.  The
 * clamp is part of every evaluation, the FSAL one included, so the returned state is clamped; OrdinaryDiffEq's update
 * formulas.  One launch for nz <= 1024: the column integrator's body with the condensation term formed after the Simpson
 * passes, beside the sedimentation flux, from the (n, theta, k) of the lane's own cell; the cell's supersaturation is read again
 * in every stage (8 bytes per cell and stage), nothing more is live across the passes.  u_out_dev may equal u_in_dev; n_steps = 0
 * copies the input to the output.  The cases without a fused kernel (see above) are stepped stage by stage inside the library
 * as cloudy_rainshaft_ssprk33_steps steps tall columns, with a cloudy_cond_evap launch per stage added into the tendency (four
 * scratch arrays of the state's size per call).  Refusals as above, and n_steps < 0 or a NaN dt: CLOUDY_EINVAL.  With s = 0 or
 * xi = 0 the result equals cloudy_rainshaft_ssprk33_steps's. */
int cloudy_rainshaft_cond_ssprk33_steps(const cloudy_plan *plan, size_t nz, size_t n_columns, size_t ld,
                                        const void *u_in_dev, void *u_out_dev, const double *s_dev, double s, double xi,
                                        double dz, double dt, int n_steps, void *stream);

/* Per-COLUMN adaptive Tsit5 for the rainshaft columns: every column of nz cells -- one ODE system, its cells couple through the
 * upwind flux -- from t = 0 to t_span under a step-size controller of its own (csrc/adaptive_column.hpp).  The sedimentation CFL
 * limit dz / v(x), the coalescence rate of the cloud slab and evaporation below cloud base differ from column to column; the
 * fixed-step integrators above take one dt for the batch.  Everything shared with cloudy_tsit5_adaptive -- the stages, err and
 * sc, the controller and its constants, the last-step rule, the first-step rule, the statuses 0 / 1 / 2, max_steps -- is stated
 * in its comment and not again here; what follows is what a column changes.
 *   right-hand side   one evaluation of the column right-hand side on a CLAMPED COPY of its argument: sources = CLOUDY_SRC_COAL is
 *                coalescence + sedimentation, what cloudy_rainshaft_rhs computes; CLOUDY_SRC_COAL | CLOUDY_SRC_COND adds get_cond_evap
 *                at the cell's supersaturation, what cloudy_rainshaft_cond_rhs computes, and s_dev (one fp64 value per cell, or
 *                NULL for the scalar `s`), s and xi mean what they mean there.  Any other `sources`: CLOUDY_EINVAL.
 *   clamping     the stage arguments are not mutated.  u is clamped to >= 0 on load and u_new before k7 = f(u_new); the clamped
 *                u_new is what the error scale, the acceptance and the store see: what the reference's in-place clamp
 *                (rainshaft_helpers.jl:52) does to the state under a FSAL method.  The returned state is therefore clamped, as
 *                cloudy_rainshaft_ssprk33_steps returns it.
 *   state units  physical for every plan: abstol_i = abstol norm_i, as the thresholded per-parcel kernels have it.
 *   error norm   per column: EEst = sqrt(sum over the column's nz cells and the planes a mode has of (err / sc)^2 / (nz n_moms));
 *                empty cells count in the mean.  Hairer's first-step guess uses the same two column means.
 *   outputs      one controller state per column: dt_dev [n_columns] (in/out), t_dev [n_columns] and info_dev [3][n_columns]
 *                (accepted, rejected, status) hold one entry per COLUMN; each may be NULL.  A column's result depends neither on
 *                the other columns of the batch nor on the workgroup size.
 * t_span = 0 copies the input to the output with status 0 and zero counts; n_columns = 0 returns CLOUDY_OK at once; u_out_dev
 * may equal u_in_dev.
 * Argument checks precede any device work, the plan last (CLOUDY_EINVAL, the message names the argument): those of
 * cloudy_tsit5_adaptive for opts and t_span, ld < nz * n_columns and NULL buffers; then `sources`, nz < 1, dz <= 0, xi NaN; then
 * the plan, which must carry terminal-velocity terms.
 * Served: AnalyticalCoalStyle plans whose thresholds are all Inf, or FixedThreshold plans; CLOUDY_F64, CLOUDY_F64_RELAXED and
 * CLOUDY_F32 planes (state and control in fp64 registers either way); nz up to 1024, provided a workgroup can hold a column.
 * Deliberate limits, each CLOUDY_EUNSUPPORTED with a message that names cloudy_rainshaft_cond_ssprk33_steps as the alternative,
 * nothing written: MovingThreshold plans; NumericalCoalStyle plans; CLOUDY_F32_FAST planes; nz > 1024, or a plan whose LDS rows
 * fit no workgroup that holds a column; plans without plan-time compilation (the kernels -- cloudy_jit_column_adaptive_*, one
 * unit per workgroup size of 256 / 512 / 1024 threads, picked by the rule of cloudy_rainshaft_rhs -- have no ahead-of-time
 * instance).  The state at the caller's save times: cloudy_rainshaft_tsit5_adaptive_saveat below.  A stage-by-stage form for
 * taller columns is not built. */
int cloudy_rainshaft_tsit5_adaptive(const cloudy_plan *plan, size_t nz, size_t n_columns, size_t ld, const void *u_in_dev,
                                    void *u_out_dev, int sources, const double *s_dev, double s, double xi, double dz,
                                    double t_span, const cloudy_adaptive_opts *opts, double *dt_dev, double *t_dev,
                                    int32_t *info_dev, void *stream);

/* cloudy_rainshaft_tsit5_adaptive with dense output: the same integration -- u_out_dev, dt_dev, t_dev and info_dev have the bits
 * that entry point gives, the workgroup size is picked by the same rule -- and the state of every cell at the batch-wide save
 * times t_save[0 .. n_save), in one launch and with no step clamped to a save time.  The save times, their checks, the
 * interpolant (the free 4th-order one of the pair, no further right-hand-side evaluation), the end points (a snapshot at 0 has the
 * bits of u_in_dev, one at t_span the bits of u_out_dev), t_span = 0 (every snapshot is the input) and the layout
 * u_save_dev[((size_t)j * planes + p) * ld + i], planes = cloudy_plan_nmom, in the plan's plane type, are those of
 * cloudy_tsit5_adaptive_saveat; what a column changes:
 *   i            is a cell index, col * nz + iz; the cells nz * n_columns .. ld of a snapshot plane are not written.
 *   clamping     a snapshot inside a step, u + h sum_i b_i(th) k_i, is clamped to >= 0 on the way out, as the returned state is:
 *                the clamped u_new is what the step ends on and what k7 was evaluated at, and a snapshot just inside a step whose
 *                u_new was clamped would be negative without it where the snapshot at its end is not.
 *   stopped columns   a COLUMN that stops with status 1 or 2 leaves a quiet NaN in every plane of every one of its cells for every
 *                snapshot beyond the time it reached (t_dev[col]); the snapshots it passed stay.
 * u_save_dev must overlap neither u_in_dev nor u_out_dev (not checked).  n_save = 0 (t_save and u_save_dev may be NULL) is
 * cloudy_rainshaft_tsit5_adaptive: the same kernel, the same bits.
 * Argument checks: the save times first (CLOUDY_EINVAL: n_save > CLOUDY_MAX_SAVE_TIMES, NULL t_save or u_save_dev with
 * n_save > 0, a time that is not finite, negative, beyond t_span or not above the one before), then every check of
 * cloudy_rainshaft_tsit5_adaptive in its order, the plan last.  Served and refused exactly as that entry point, each refusal
 * CLOUDY_EUNSUPPORTED in its words with nothing written, u_save_dev included.  The kernels -- cloudy_jit_column_dense_*, the SAVE
 * instances of the same body -- sit in three units of their own, compiled on the first call with save times. */
int cloudy_rainshaft_tsit5_adaptive_saveat(const cloudy_plan *plan, size_t nz, size_t n_columns, size_t ld, const void *u_in_dev,
                                           void *u_out_dev, int sources, const double *s_dev, double s, double xi, double dz,
                                           double t_span, const cloudy_adaptive_opts *opts, double *dt_dev, double *t_dev,
                                           int32_t *info_dev, void *stream, size_t n_save, const double *t_save,
                                           void *u_save_dev);

/* sums_dev[q] = sum over parcels of plane q (fp64 accumulate); `planes` planes are reduced.
 * The multi-GPU conservation check all-reduces these nmom doubles (RCCL), see INTEGRATION.md. */
int cloudy_moment_sums(const cloudy_plan *plan, size_t n_parcels, size_t ld, int planes, const void *arr_dev,
                       double *sums_dev, void *stream);
/* the same with a caller-supplied workspace of cloudy_moment_sums_workspace_bytes(planes) bytes of device memory:
 * re-entrant (any number of streams may reduce with one plan concurrently, each with its own workspace) */
size_t cloudy_moment_sums_workspace_bytes(int planes);
int cloudy_moment_sums_ws(const cloudy_plan *plan, size_t n_parcels, size_t ld, int planes, const void *arr_dev,
                          double *sums_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* ---- multi-GPU: the one collective of the path ----------------------------------------------------------
 * Parcels are independent: ranks (one process per GPU, or one process driving several GPUs) own contiguous parcel ranges
 * and exchange nothing per right-hand side.  The only exchange is the sum over ranks of the nmom plane sums of the
 * conservation diagnostic (moments_sum, plotting_helpers.jl:240-252): ncclAllReduce(sum, ncclDouble, planes values) over
 * RCCL / xGMI, issued on the caller's stream.  RCCL is bound at first use (dlopen librccl.so.1): hosts that never create a
 * communicator do not load it.  CLOUDY_EUNSUPPORTED if RCCL is absent, CLOUDY_ECOMM on an RCCL error.
 *
 * One process per GPU: rank 0 calls cloudy_comm_unique_id, the host hands the 128 bytes to every rank (MPI.bcast, a
 * file, a socket -- the library does no rendezvous of its own), every rank calls cloudy_comm_create (collective).
 * One process, several GPUs: cloudy_comm_create_all, and bracket the per-GPU cloudy_moment_sums_allreduce calls with
 * cloudy_comm_group_start / _end as RCCL requires for one thread driving several communicators. */
#define CLOUDY_COMM_ID_BYTES 128
typedef struct cloudy_comm cloudy_comm;
int cloudy_comm_rccl_version(void);                 /* NCCL_VERSION_CODE of the RCCL bound, 0 if none */
int cloudy_comm_unique_id(void *id_out /*[CLOUDY_COMM_ID_BYTES]*/);
/* device: HIP ordinal the communicator binds to, -1 = current */
int cloudy_comm_create(int world_size, int rank, const void *id /*[CLOUDY_COMM_ID_BYTES]*/, int device, cloudy_comm **out);
/* devices: n_devices ordinals, NULL = 0 .. n_devices-1; comms_out[i] has rank i */
int cloudy_comm_create_all(int n_devices, const int *devices, cloudy_comm **comms_out /*[n_devices]*/);
void cloudy_comm_destroy(cloudy_comm *comm);
int cloudy_comm_rank(const cloudy_comm *comm);
int cloudy_comm_world_size(const cloudy_comm *comm);
int cloudy_comm_device(const cloudy_comm *comm);
int cloudy_comm_group_start(void);
int cloudy_comm_group_end(void);
/* recv_dev[i] = sum over ranks of send_dev[i], i < count; in place allowed; asynchronous on `stream` */
int cloudy_allreduce_sum_f64(cloudy_comm *comm, const double *send_dev, double *recv_dev, size_t count, void *stream);
/* cloudy_moment_sums of this rank's parcels followed by the all-reduce, in place in sums_dev, both on `stream`:
 * sums_dev[q] = sum over ALL ranks' parcels of plane q.  With world_size 1 the result is cloudy_moment_sums' bit for bit. */
int cloudy_moment_sums_allreduce(const cloudy_plan *plan, cloudy_comm *comm, size_t n_parcels, size_t ld, int planes,
                                 const void *arr_dev, double *sums_dev, void *stream);

/* thin device-memory helpers so that a host without a HIP binding can keep state device-resident */
int cloudy_device_count(void);
int cloudy_set_device(int device);
/* "dddd:bb:dd.f" of a device ordinal (hipDeviceGetPCIBusId), len >= 13: bench.py --gpus N records it per rank so that a
 * scaling record shows N distinct devices */
int cloudy_device_pci_bus_id(int device, char *buf, int len);
int cloudy_malloc(void **dev_ptr, size_t bytes);
int cloudy_free(void *dev_ptr);
int cloudy_memcpy_h2d(void *dst_dev, const void *src_host, size_t bytes, void *stream);
int cloudy_memcpy_d2h(void *dst_host, const void *src_dev, size_t bytes, void *stream);
int cloudy_memset(void *dst_dev, int value, size_t bytes, void *stream);
int cloudy_stream_synchronize(void *stream);

/* launch-timing helper used by bench.py: runs `iters` back-to-back cloudy_coal_rhs launches on `stream`
 * bracketed by HIP events recorded on that stream; returns the average milliseconds per launch. */
int cloudy_time_coal_rhs(const cloudy_plan *plan, size_t n_parcels, size_t ld, const void *mom_dev,
                         void *dmom_dev, void *stream, int iters, float *ms_per_launch);

/* generic launch timing with HIP events recorded on `stream` (the stream the kernels are launched on): begin records an
 * event and hands out a timer, end records the second event, waits for it, returns the milliseconds between the two and
 * releases the timer.  bench.py brackets every variant that is not a plain cloudy_coal_rhs loop with these. */
int cloudy_timer_begin(void *stream, void **timer_out);
int cloudy_timer_end(void *timer, void *stream, float *ms_total);

const char *cloudy_last_error(void);
int cloudy_version(void);
/* FNV-1a of the kernel sources inside the library (which = 0: all of them; 1: those of the all-Inf kernels, the headline of
 * bench.py): a committed profile figure is quoted only for the sources it was collected on */
unsigned long long cloudy_source_hash(int which);

#ifdef __cplusplus
}
#endif
#endif /* CLOUDY_HIP_H */
