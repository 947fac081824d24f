// libastro_qopt.so: torch.optim's SGD, RMSprop, Adagrad and Adam on a packed
// float32 parameter buffer, with clip_grad_norm_, a non-finite guard and the
// target network's update (include/astro_qopt.h).
//
// One workgroup of 1,024 threads (16 waves) walks k = t, t + 1024, ...: twice,
// once for the gradient's norm (float64 partials, folded through LDS in the
// order the header states) and once for the update, which reads the gradient
// again from cache.  The norm is a reduction inside the workgroup, so the clip
// coefficient and the guard need no second launch and no grid-wide barrier.
// Neighbouring lanes touch neighbouring floats; a network of 4,934 parameters
// is five passes of the loop, and the call is bound by its launch.
//
// Every float32 operation below rounds on its own (the build's
// -ffp-contract=off; divide and sqrt are correctly rounded): the expressions
// are written in the header's order and astro_amd.optim.step_host mirrors them.
#include "astro_qopt.h"
#include "astro_common.h"

#include <cmath>

namespace {

constexpr int THREADS = ASTRO_QOPT_THREADS;

template <int KIND>
__global__ __launch_bounds__(THREADS) void qopt_kernel(AstroQOpt o, int n, const float *__restrict__ grad,
                                                       float *__restrict__ w, float *__restrict__ s1,
                                                       float *__restrict__ s2, float *__restrict__ target,
                                                       float *__restrict__ norm_out, int32_t *__restrict__ skipped) {
    __shared__ double part[THREADS];
    const int t = threadIdx.x;

    double sum = 0.0;
    for (int k = t; k < n; k += THREADS) {
        const double g = double(grad[k]);
        sum = sum + g * g;
    }
    part[t] = sum;
    __syncthreads();
    for (int h = THREADS / 2; h >= 1; h >>= 1) {
        if (t < h) part[t] = part[t] + part[t + h];
        __syncthreads();
    }
    const double norm = sqrt(part[0]);
    const bool finite = norm <= 1.7976931348623157e308;   // false for a NaN too
    if (t == 0) {
        if (norm_out) *norm_out = float(norm);
        if (!finite && skipped) *skipped = *skipped + 1;
    }
    if (!finite) return;

    const bool clip = o.max_norm > 0.0f;
    float coef = 1.0f;
    if (clip) {
        const double c = double(o.max_norm) / (norm + 1e-6);
        coef = float(c < 1.0 ? c : 1.0);
    }
    const bool decay = o.weight_decay != 0.0f;
    const bool momentum = o.momentum != 0.0f;

    for (int k = t; k < n; k += THREADS) {
        float g = grad[k];
        float x = w[k];
        if (clip) g = coef * g;
        if (decay) g = g + o.weight_decay * x;
        if (KIND == ASTRO_QOPT_SGD) {
            if (momentum) {
                const float b = o.momentum * s1[k] + g;
                s1[k] = b;
                g = o.nesterov ? g + o.momentum * b : b;
            }
            x = x - o.lr * g;
        } else if (KIND == ASTRO_QOPT_RMSPROP) {
            const float v = o.alpha * s1[k] + o.one_minus_alpha * (g * g);
            s1[k] = v;
            x = x - o.lr * (g / (sqrtf(v) + o.eps));
        } else if (KIND == ASTRO_QOPT_ADAGRAD) {
            const float v = s1[k] + g * g;
            s1[k] = v;
            x = x - o.lr * (g / (sqrtf(v) + o.eps));
        } else {
            const float m = o.beta1 * s1[k] + o.one_minus_beta1 * g;
            const float v = o.beta2 * s2[k] + o.one_minus_beta2 * (g * g);
            s1[k] = m;
            s2[k] = v;
            x = x - o.step_size * (m / (sqrtf(v) / o.bc2 + o.eps));
        }
        w[k] = x;
        if (target) {
            const float y = target[k];
            target[k] = o.tau == 1.0f ? x : y + o.tau * (x - y);
        }
    }
}

inline bool bad(float x) { return !(x >= 0.0f) || std::isinf(x); }   // negative, NaN or infinite

}  // namespace

extern "C" {

int astro_qopt_abi_version(void) { return ASTRO_QOPT_ABI_VERSION; }
const char *astro_qopt_last_error(void) { return g_err; }

int astro_qopt_step(const AstroQOpt *opt, int32_t nparams, const float *grad, float *weights, float *state1,
                    float *state2, float *target, float *norm_out, int32_t *skipped, void *stream) {
    if (!opt) return fail(-100, "opt is NULL");
    const AstroQOpt &o = *opt;
    if (o.kind < ASTRO_QOPT_SGD || o.kind > ASTRO_QOPT_ADAM) return fail(-101, "opt.kind %d is unknown", int(o.kind));
    if (nparams < 1 || nparams > ASTRO_QOPT_MAX_PARAMS)
        return fail(-102, "nparams must be in [1, %d], got %d", ASTRO_QOPT_MAX_PARAMS, int(nparams));
    if (!(o.tau > 0.0f && o.tau <= 1.0f)) return fail(-103, "opt.tau must be in (0, 1], got %g", double(o.tau));
    const float all[] = {o.lr, o.weight_decay, o.max_norm, o.momentum, o.alpha, o.one_minus_alpha, o.beta1,
                         o.one_minus_beta1, o.beta2, o.one_minus_beta2, o.step_size, o.bc2, o.eps};
    for (float x : all)
        if (!std::isfinite(x)) return fail(-104, "a hyperparameter of opt is not finite");
    if (bad(o.lr) || bad(o.weight_decay) || bad(o.momentum) || bad(o.eps))
        return fail(-104, "opt.lr, weight_decay, momentum and eps must be >= 0");
    if (o.kind == ASTRO_QOPT_ADAM && !(o.bc2 > 0.0f && o.bc2 <= 1.0f))
        return fail(-104, "opt.bc2 must be in (0, 1], got %g", double(o.bc2));
    if (!grad) return fail(-110, "grad is NULL");
    if (!weights) return fail(-111, "weights is NULL");
    const bool needs1 = o.kind != ASTRO_QOPT_SGD || o.momentum != 0.0f;
    if (needs1 && !state1) return fail(-112, "state1 is NULL (kind %d keeps a state array)", int(o.kind));
    if (o.kind == ASTRO_QOPT_ADAM && !state2) return fail(-113, "state2 is NULL (ADAM's v)");
    if (target == weights) return fail(-114, "target is weights: the target network needs storage of its own");
    if (!aligned(grad, 4) || !aligned(weights, 4) || !aligned(state1, 4) || !aligned(state2, 4) ||
        !aligned(target, 4) || !aligned(norm_out, 4) || !aligned(skipped, 4))
        return fail(-119, "grad, weights, state1, state2, target, norm_out and skipped must be 4-byte aligned");

    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(1), block(THREADS);
    // a state array the kind does not read is not handed to the kernel
    float *s1 = needs1 ? state1 : nullptr, *s2 = o.kind == ASTRO_QOPT_ADAM ? state2 : nullptr;
    switch (o.kind) {
        case ASTRO_QOPT_SGD:
            hipLaunchKernelGGL(qopt_kernel<ASTRO_QOPT_SGD>, grid, block, 0, st, o, int(nparams), grad, weights, s1, s2,
                               target, norm_out, skipped);
            break;
        case ASTRO_QOPT_RMSPROP:
            hipLaunchKernelGGL(qopt_kernel<ASTRO_QOPT_RMSPROP>, grid, block, 0, st, o, int(nparams), grad, weights, s1,
                               s2, target, norm_out, skipped);
            break;
        case ASTRO_QOPT_ADAGRAD:
            hipLaunchKernelGGL(qopt_kernel<ASTRO_QOPT_ADAGRAD>, grid, block, 0, st, o, int(nparams), grad, weights, s1,
                               s2, target, norm_out, skipped);
            break;
        default:
            hipLaunchKernelGGL(qopt_kernel<ASTRO_QOPT_ADAM>, grid, block, 0, st, o, int(nparams), grad, weights, s1, s2,
                               target, norm_out, skipped);
            break;
    }
    return launched("astro_qopt_step");
}

}  // extern "C"
