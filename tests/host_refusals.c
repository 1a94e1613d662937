/* host_refusals.c -- every exit of the host half of libcloudy_hip.so that gives up a plan, an event or a timer, walked by a plain
 * C program that uses include/cloudy_hip.h alone.  tests/test_host_refusals.py links it against the host sanitizer build of the
 * library (libcloudy_hip_asan.so) with the same sanitizers and runs it as an ordinary process: a plan read after it was freed,
 * freed twice or not freed at all is the sanitizers' finding, not this program's.
 *
 * Each refused descriptor goes through cloudy_plan_create and through cloudy_jit_selfcheck(desc, "source-only"): the same status
 * from both, a message, no handle.  Then descriptors that are served: the self-check passes, and without a device
 * cloudy_plan_create answers CLOUDY_ENODEVICE -- the exit that frees a completely built host plan.  Exit status 0: all as stated. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "cloudy_hip.h"

static int failures = 0;

#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            ++failures;                                    \
            fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                  \
            fprintf(stderr, " [%s]\n", #cond);             \
        }                                                  \
    } while (0)

/* symmetric in (a, b) and in (j, k): [2][2][2][2] for CLOUDY_KERNEL_MATRIX */
static double kernel[16];

/* two Gamma modes, order-1 tensor per pair, no thresholds */
static void tensor_desc(cloudy_plan_desc *d) {
    cloudy_plan_desc_init(d);
    d->n_modes = 2;
    d->dist_type[0] = d->dist_type[1] = CLOUDY_DIST_GAMMA;
    d->tensor_p = 2;
    d->kernel_layout = CLOUDY_KERNEL_MATRIX;
    for (int jk = 0; jk < 4; ++jk) {
        const double s = 1.0 + 0.25 * ((jk == 1 || jk == 2) ? 1 : jk);
        kernel[4 * jk + 0] = 1e-7 * s;
        kernel[4 * jk + 1] = kernel[4 * jk + 2] = 5.0 * s;
        kernel[4 * jk + 3] = 0.0;
    }
    d->kernel_c = kernel;
    d->norms[0] = 1e6;
    d->norms[1] = 1e-9;
}

/* two Gamma modes under the hydrodynamic kernel function, fixed 10-point rule */
static void numerical_desc(cloudy_plan_desc *d) {
    cloudy_plan_desc_init(d);
    d->coal_style = CLOUDY_NUMERICAL_COAL;
    d->n_modes = 2;
    d->dist_type[0] = d->dist_type[1] = CLOUDY_DIST_GAMMA;
    d->kernel_func = CLOUDY_KFUNC_HYDRODYNAMIC;
    d->kernel_func_params[0] = 3e2;
    d->quad_order = 10;
    d->quad_mode = CLOUDY_QUAD_FIXED;
    d->norms[0] = 1e6;
    d->norms[1] = 1e-9;
}

/* a descriptor both entry points refuse with `code`; `needle` (or NULL) is part of the message */
static void refused(const char *what, const cloudy_plan_desc *d, int code, const char *needle) {
    cloudy_plan *h = (cloudy_plan *)(void *)&failures; /* (a refusal must clear the caller's handle) */
    const int rc = cloudy_plan_create(d, &h);
    char msg[512];
    snprintf(msg, sizeof msg, "%s", cloudy_last_error());
    CHECK(rc == code, "%s: cloudy_plan_create returned %d, not %d (%s)", what, rc, code, msg);
    CHECK(h == NULL, "%s: a refusal left a handle", what);
    CHECK(msg[0] != 0, "%s: no message", what);
    CHECK(!needle || strstr(msg, needle), "%s: message \"%s\" lacks \"%s\"", what, msg, needle ? needle : "");
    const int rs = cloudy_jit_selfcheck(d, "source-only");
    CHECK(rs == rc, "%s: cloudy_jit_selfcheck returned %d, cloudy_plan_create %d", what, rs, rc);
    CHECK(cloudy_last_error()[0] != 0, "%s: no message from cloudy_jit_selfcheck", what);
    if (rc == CLOUDY_OK && h) cloudy_plan_destroy(h);
}

/* a descriptor that is served: the self-check passes; cloudy_plan_create needs a device */
static void served(const char *what, const cloudy_plan_desc *d) {
    const int rs = cloudy_jit_selfcheck(d, "source-only");
    CHECK(rs == CLOUDY_OK, "%s: cloudy_jit_selfcheck returned %d (%s)", what, rs, cloudy_last_error());
    cloudy_plan *h = (cloudy_plan *)(void *)&failures;
    const int rc = cloudy_plan_create(d, &h);
    if (cloudy_device_count() == 0) {
        CHECK(rc == CLOUDY_ENODEVICE, "%s: cloudy_plan_create without a device returned %d (%s)", what, rc, cloudy_last_error());
        CHECK(h == NULL, "%s: CLOUDY_ENODEVICE left a handle", what);
        CHECK(strstr(cloudy_last_error(), "no HIP device") != NULL, "%s: message \"%s\"", what, cloudy_last_error());
    } else {
        CHECK(rc == CLOUDY_OK && h != NULL, "%s: cloudy_plan_create returned %d (%s)", what, rc, cloudy_last_error());
        if (rc == CLOUDY_OK) cloudy_plan_destroy(h);
    }
}

int main(void) {
    cloudy_plan_desc d;

    tensor_desc(&d); d.n_modes = 0; refused("n_modes 0", &d, CLOUDY_EUNSUPPORTED, "n_modes");
    tensor_desc(&d); d.n_modes = 9; refused("n_modes 9", &d, CLOUDY_EUNSUPPORTED, "n_modes");
    tensor_desc(&d); d.tensor_p = 0; refused("tensor_p 0", &d, CLOUDY_EUNSUPPORTED, "tensor_p");
    tensor_desc(&d); d.tensor_p = 9; refused("tensor_p 9", &d, CLOUDY_EUNSUPPORTED, "tensor_p");
    tensor_desc(&d); d.struct_size = 8; refused("struct_size", &d, CLOUDY_EINVAL, "struct_size");
    tensor_desc(&d); d.dist_type[1] = 7; refused("dist_type", &d, CLOUDY_EINVAL, "dist_type[1] = 7");
    tensor_desc(&d); d.norms[0] = 0.0; refused("zero norm", &d, CLOUDY_EINVAL, "norms must be positive");
    tensor_desc(&d); d.k_range[0] = 5.0; d.k_range[1] = 1.0; refused("inverted k_range", &d, CLOUDY_EINVAL, "k_range");
    tensor_desc(&d); d.n_vel = 5; refused("n_vel 5", &d, CLOUDY_EUNSUPPORTED, "n_vel");
    tensor_desc(&d); d.dtype = 9; refused("dtype", &d, CLOUDY_EINVAL, "dtype");
    tensor_desc(&d); d.kernel_c = NULL; refused("kernel_c NULL", &d, CLOUDY_EINVAL, "kernel_c");
    tensor_desc(&d); d.dist_thresholds[0] = NAN; refused("NaN threshold", &d, CLOUDY_EINVAL, "dist_thresholds[0] is NaN");
    tensor_desc(&d);
    d.threshold_style = CLOUDY_MOVING_THRESHOLD;
    d.dist_thresholds[0] = 1.5;
    d.dist_thresholds[1] = 1.0;
    refused("percentile above 1", &d, CLOUDY_EINVAL, "percentile 0");
    tensor_desc(&d); kernel[1] += 1.0; refused("asymmetric tensor", &d, CLOUDY_ENOTSYMMETRIC, "not symmetric");
    numerical_desc(&d); d.quad_order = 1000; refused("quad_order 1000", &d, CLOUDY_EUNSUPPORTED, "quad_order");
    numerical_desc(&d); d.kernel_func = 11; refused("kernel_func 11", &d, CLOUDY_EINVAL, "kernel_func 11");
    numerical_desc(&d); d.dist_type[1] = CLOUDY_DIST_MONODISPERSE; refused("Monodisperse, numerical", &d, CLOUDY_EINVAL, "Monodisperse");
    /* compute_threshold has no method for a Lognormal mode that is not the last: the message names the mode and its type */
    tensor_desc(&d);
    d.n_modes = 4;
    d.kernel_layout = CLOUDY_KERNEL_SINGLE;
    d.threshold_style = CLOUDY_MOVING_THRESHOLD;
    for (int i = 0; i < 4; ++i) {
        d.dist_type[i] = i == 1 ? CLOUDY_DIST_LOGNORMAL : CLOUDY_DIST_GAMMA;
        d.dist_thresholds[i] = i < 3 ? 0.9 : 1.0;
    }
    refused("Lognormal in a non-last MovingThreshold mode", &d, CLOUDY_EINVAL, "dist_type[1] = 3");

    /* no descriptor at all */
    cloudy_plan *h = NULL;
    CHECK(cloudy_plan_create(NULL, &h) == CLOUDY_EINVAL && h == NULL, "cloudy_plan_create(NULL, &h)");
    CHECK(cloudy_plan_create(NULL, NULL) == CLOUDY_EINVAL, "cloudy_plan_create(NULL, NULL)");
    CHECK(cloudy_jit_selfcheck(NULL, "source-only") == CLOUDY_EINVAL, "cloudy_jit_selfcheck(NULL)");
    cloudy_plan_destroy(NULL);

    /* descriptors that are served: all-Inf and FixedThreshold tensor plans (the second with node tables and velocity terms),
     * a MovingThreshold one, both quadrature modes */
    tensor_desc(&d); served("tensor plan", &d);
    tensor_desc(&d);
    d.dist_thresholds[0] = 5e-10;
    d.n_vel = 2;
    d.vel[0][0] = 50.0; d.vel[0][1] = 1.0 / 6;
    d.vel[1][0] = 25.0; d.vel[1][1] = 1.0 / 3;
    served("FixedThreshold tensor plan", &d);
    tensor_desc(&d);
    d.threshold_style = CLOUDY_MOVING_THRESHOLD;
    d.dist_thresholds[0] = 0.9;
    d.dist_thresholds[1] = 1.0;
    served("MovingThreshold tensor plan", &d);
    numerical_desc(&d); d.n_vel = 1; d.vel[0][0] = 50.0; d.vel[0][1] = 1.0 / 6; served("numerical plan, fixed rule", &d);
    numerical_desc(&d); d.quad_order = 0; d.quad_mode = CLOUDY_QUAD_CONVERGED; served("numerical plan, converged", &d);

    /* timers and the timed loop with arguments they refuse, and -- without a device -- with events that cannot be created */
    void *timer = NULL;
    float ms = -1.f;
    CHECK(cloudy_timer_begin(NULL, NULL) == CLOUDY_EINVAL, "cloudy_timer_begin(NULL, NULL)");
    CHECK(cloudy_timer_end(NULL, NULL, &ms) == CLOUDY_EINVAL && ms == -1.f, "cloudy_timer_end(NULL, ...)");
    CHECK(cloudy_time_coal_rhs(NULL, 1, 1, NULL, NULL, NULL, 0, &ms) == CLOUDY_EINVAL, "cloudy_time_coal_rhs, iters 0");
    CHECK(cloudy_time_coal_rhs(NULL, 1, 1, NULL, NULL, NULL, 3, NULL) == CLOUDY_EINVAL, "cloudy_time_coal_rhs, ms NULL");
    /* (with a device: the events exist and the loop's first call refuses the NULL plan) */
    CHECK(cloudy_time_coal_rhs(NULL, 1, 1, NULL, NULL, NULL, 3, &ms) != CLOUDY_OK && ms == -1.f, "cloudy_time_coal_rhs, plan NULL");
    CHECK(cloudy_last_error()[0] != 0, "cloudy_time_coal_rhs: no message");
    if (cloudy_device_count() == 0) {
        CHECK(cloudy_timer_begin(NULL, &timer) != CLOUDY_OK && timer == NULL, "cloudy_timer_begin without a device");
        CHECK(cloudy_last_error()[0] != 0, "cloudy_timer_begin: no message");
    } else {
        CHECK(cloudy_timer_begin(NULL, &timer) == CLOUDY_OK && timer != NULL, "cloudy_timer_begin");
        CHECK(cloudy_timer_end(timer, NULL, &ms) == CLOUDY_OK && ms >= 0.f, "cloudy_timer_end");
    }

    if (failures) {
        fprintf(stderr, "host_refusals: %d check(s) failed\n", failures);
        return 1;
    }
    printf("host_refusals ok\n");
    return 0;
}
