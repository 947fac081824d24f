/*
 * astro_qopt.h -- C-ABI of libastro_qopt.so, the MI355X (gfx950) optimiser
 * step for a packed float32 parameter buffer (AstroQNet.weights of
 * astro_qnet.h, or any other).
 *
 * The reference's trainer picks its update rule among torch.optim's (astro/rl.py
 * 172-176: Adam, Rprop, RMSprop, Adagrad, SGD).  astro_qopt_step is one of those
 * rules -- SGD with momentum, RMSprop, Adagrad or Adam; Rprop is left out -- on
 * the buffer in place, with gradient-norm clipping (torch.nn.utils
 * clip_grad_norm_), a non-finite guard and the update of a target copy of the
 * buffer, in ONE launch of one workgroup.
 *
 * Conventions: those of astro_qtrain.h.  The caller owns all memory; the call
 * is stream-ordered and asynchronous on `stream`; the library never allocates
 * or synchronises; 0 on success, a negative code on a bad argument (-1..-199,
 * rejected before the device is touched) or a launch failure (-1000 -
 * hipError_t), described by astro_qopt_last_error() for the calling thread.
 *
 * This library is separate from the five others and shares nothing with them:
 * nparams is a plain argument, the network's shape is not known here.
 */
#ifndef ASTRO_QOPT_H
#define ASTRO_QOPT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ASTRO_QOPT_ABI_VERSION 1
#define ASTRO_QOPT_MAX_PARAMS (1 << 20) /* nparams: 1 .. 2^20 */
#define ASTRO_QOPT_THREADS 1024         /* the one workgroup; fixes the norm's summation order */

#define ASTRO_QOPT_SGD 0
#define ASTRO_QOPT_RMSPROP 1
#define ASTRO_QOPT_ADAGRAD 2
#define ASTRO_QOPT_ADAM 3

int astro_qopt_abi_version(void);
const char *astro_qopt_last_error(void);

/* The hyperparameters of one step, all float32 as they stand here.  The host
 * computes every derived scalar in float64 FROM THE FLOAT32 VALUE of the
 * hyperparameter and rounds it ONCE to float32:
 *   one_minus_alpha = 1 - alpha, one_minus_beta1 = 1 - beta1, one_minus_beta2 = 1 - beta2,
 *   step_size = lr / (1 - beta1^t), bc2 = sqrt(1 - beta2^t)     (ADAM; t = 1, 2, ... counts the steps)
 * Fields a kind does not use are ignored (but must be finite). */
typedef struct AstroQOpt {
    int32_t kind;          /* ASTRO_QOPT_* */
    int32_t nesterov;      /* SGD: 0 or 1 */
    float lr;              /* SGD, RMSPROP, ADAGRAD */
    float weight_decay;    /* every kind; 0: none */
    float max_norm;        /* > 0: clip the gradient's norm to it; <= 0: no clipping */
    float momentum;        /* SGD mu; 0: no state */
    float alpha;           /* RMSPROP */
    float one_minus_alpha;
    float beta1;           /* ADAM */
    float one_minus_beta1;
    float beta2;
    float one_minus_beta2;
    float step_size;       /* ADAM */
    float bc2;             /* ADAM, in (0, 1] */
    float eps;             /* RMSPROP, ADAGRAD, ADAM */
    float tau;             /* target update, in (0, 1]; looked at whether or not target is NULL */
} AstroQOpt;

/* One optimiser step.
 *
 * grad:     const float32 [nparams]; never written.
 * weights:  float32 [nparams], updated in place.
 * state1:   float32 [nparams]: SGD's b (needed when momentum != 0), RMSPROP's and
 *           ADAGRAD's v, ADAM's m.  Zeros before the first step.  NULL where the
 *           kind has no state (SGD with momentum == 0: it is then not looked at).
 * state2:   float32 [nparams]: ADAM's v; not looked at by the other kinds.
 * target:   float32 [nparams] or NULL: target[k] = target[k] + tau * (w_new[k] -
 *           target[k]) (three roundings); with tau == 1 the kernel stores w_new[k]
 *           itself, an exact copy.  May not be `weights`.
 * norm_out: device float or NULL: always receives float32(norm).
 * skipped:  device int32 or NULL: *skipped += 1 when the step is skipped (one
 *           thread, plain load and store: the call is stream-ordered).
 * The arrays may not overlap each other.
 *
 * ORDER OF OPERATIONS.  Everything below is float32 and every operation rounds
 * separately (no fused multiply-add; divide and sqrt correctly rounded), except
 * the norm, which is float64.  astro_amd.optim.step_host is this text in numpy.
 *
 *   norm:  thread t of 1024 adds double(grad[k])^2 (exact in double) for k = t,
 *          t + 1024, ... in ascending k to its own double, starting from 0; the
 *          1024 partials s[] are then folded in halves: for h = 512, 256, ..., 1:
 *          s[i] = s[i] + s[i + h] for i < h; norm = sqrt(s[0]) in double.
 *   guard: norm not finite (a NaN or an infinity in grad): nothing but norm_out
 *          and skipped is written.
 *   clip:  max_norm > 0: coef = float32(min(1, double(max_norm) / (norm + 1e-6)))
 *          in double, g = coef * grad[k] (coef == 1 leaves g = grad[k] bit for bit);
 *          else g = grad[k].
 *   decay: weight_decay != 0: g = g + weight_decay * w.
 *   SGD:      momentum != 0: b = momentum * b + g; g = nesterov ? g + momentum * b : b.
 *             w = w - lr * g.
 *   RMSPROP:  v = alpha * v + one_minus_alpha * (g * g);  w = w - lr * (g / (sqrt(v) + eps)).
 *   ADAGRAD:  v = v + g * g;                              w = w - lr * (g / (sqrt(v) + eps)).
 *   ADAM:     m = beta1 * m + one_minus_beta1 * g;  v = beta2 * v + one_minus_beta2 * (g * g);
 *             w = w - step_size * (m / (sqrt(v) / bc2 + eps)).
 *   target (if given), from the w just stored.
 * These are torch.optim's SGD, RMSprop, Adagrad and Adam (defaults otherwise:
 * no dampening, not centered, no lr_decay, no amsgrad, L2 weight decay).
 *
 * Subnormal intermediates follow the build's float32 denormal mode and are not
 * covered by the bit-for-bit statement.  For the same inputs the results are
 * bit-identical from call to call: no atomics, one workgroup, a fixed order.
 *
 * Argument codes, in the order they are checked:
 *   -100 opt is NULL                 -101 opt.kind unknown
 *   -102 nparams < 1 or > ASTRO_QOPT_MAX_PARAMS
 *   -103 opt.tau outside (0, 1]
 *   -104 a hyperparameter is not finite; lr, weight_decay, momentum or eps < 0;
 *        ADAM's bc2 outside (0, 1]
 *   -110 grad is NULL                -111 weights is NULL
 *   -112 state1 is NULL where the kind needs it
 *   -113 state2 is NULL (ADAM)       -114 target == weights
 *   -119 an array, norm_out or skipped is not 4-byte aligned */
int astro_qopt_step(const AstroQOpt *opt, int32_t nparams, const float *grad, float *weights,
                    float *state1, float *state2, float *target, float *norm_out, int32_t *skipped,
                    void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ASTRO_QOPT_H */
