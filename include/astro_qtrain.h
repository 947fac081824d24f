/*
 * astro_qtrain.h -- C-ABI of libastro_qtrain.so, the MI355X (gfx950) training
 * half of the fused Q-network of astro_qnet.h.
 *
 * The reference's learner (astro/rl.py) trains rl.ValueNetwork on batches of
 * to_batch feature tensors:
 *
 *   astro_qforward <- rl.ValueNetwork.forward on a feature tensor (rl.py:75-99,
 *                     137-155), and its max over the outputs: the
 *                     `max_a Q(new_state_f)` of QBotTrainer._step (rl.py:278-291)
 *   astro_qgrad    <- rl.QNetworkTrainer.step's loss and its gradient
 *                     (rl.py:184-188) without the optimiser step
 *
 * on the packed weights astro_qvalues reads (AstroQNet, same layout, same
 * state_dict order), so a trained buffer is the acting kernel's input as it
 * stands.
 *
 * Conventions: those of astro_qnet.h.  The caller owns all memory; every call
 * is stream-ordered and asynchronous on `stream`; the library never allocates
 * or synchronises; 0 on success, a negative code on a bad argument (-1..-199,
 * rejected before the device is touched) or a launch failure (-1000 -
 * hipError_t), described by astro_qtrain_last_error() for the calling thread.
 *
 * This library is separate from libastro_qnet.so and libastro_hip.so and
 * shares only the AstroQNet struct with the former.
 */
#ifndef ASTRO_QTRAIN_H
#define ASTRO_QTRAIN_H

#include <stddef.h>
#include <stdint.h>

#include "astro_qnet.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ASTRO_QTRAIN_ABI_VERSION 1
#define ASTRO_QTRAIN_MAX_ROWS (1 << 24) /* rows of a feature tensor */

int astro_qtrain_abi_version(void);
const char *astro_qtrain_last_error(void);

/* Argument codes (both entry points):
 *   -100 net is NULL                 -101 net.nships not 1 or 2
 *   -102 net.nout outside 1..6       -105 net.weights NULL or not 4-byte aligned
 *   -110 features is NULL            -111 n < 0
 *   -112 rows < 1 or > ASTRO_QTRAIN_MAX_ROWS
 *   -114 q and qmax both NULL        -115 action is NULL
 *   -116 target is NULL              -117 grad is NULL
 *   -118 workspace NULL or smaller than astro_qgrad_workspace_bytes
 *   -119 a float array is not 4-byte aligned, or workspace not 16-byte aligned
 * net, nships, nout, n, rows and the output pointers are checked first, in
 * that order; with n == 0 the input arrays and the workspace are not looked
 * at and may be NULL. */

/* rl.ValueNetwork.forward on a to_batch feature tensor.
 *
 * features: float32 [n][rows][nf], nf = 5 + 5*net->nships, contiguous.  A row
 *           whose column 0 is < 0 is padding and takes no part in the max
 *           pool, wherever it stands among the rows; its other columns are
 *           never read.  (A NaN in column 0 is not < 0: the row is live.)
 * q:        float32 [n][nout], or NULL
 * qmax:     float32 [n], or NULL: the maximum of the sample's nout values of q,
 *           bit for bit.  q and qmax may not both be NULL.
 * n == 0 returns 0 and touches nothing.
 * Every sample needs at least one live row (BatchedEnv.features always has
 * one).  A sample with none reads and writes nothing out of bounds; its
 * values are unspecified.  All arithmetic is float32. */
int astro_qforward(const AstroQNet *net, const float *features, int32_t n, int32_t rows,
                   float *q, float *qmax, void *stream);

/* rl.QNetworkTrainer.step's loss and gradient, without the optimiser:
 *
 *   y_i = Q(features_i)[action_i];  loss_i = (target_i - y_i)^2;  L = mean_i loss_i
 *
 * action:    int8 [n] (the dtype BatchedEnv.qcontrols writes)
 * target:    float32 [n]
 * loss:      float32 [n], or NULL
 * grad:      float32 [nparams]: dL/dw in the packed layout of AstroQNet.weights;
 *            every element is written.
 * workspace: device scratch of at least astro_qgrad_workspace_bytes(net, n)
 *            bytes, 16-byte aligned; its contents on entry are irrelevant and
 *            on return unspecified.
 *
 * Max pool backward: the gradient of a pooled unit goes to the FIRST live row
 * that attains the maximum (np.argmax over the sample's live rows).
 *
 * Determinism: no float atomics.  Every wave keeps its own partial sums and
 * writes them to the workspace; a second kernel of the same call adds the
 * partials in a fixed order in float64 and rounds once.  For the same inputs
 * on the same device, grad and loss are bit-identical from call to call,
 * whatever the workspace held.
 *
 * A sample whose action is out of range (action < 0 or >= nout) gets loss =
 * NaN and adds nothing to grad; it still counts in the mean's n.
 * A sample with no live row: as for astro_qforward.
 * n == 0 returns 0 and writes zeros to grad (loss is not touched).
 *
 * astro_qgrad_workspace_bytes returns 0 for a NULL or invalid net or n <= 0. */
size_t astro_qgrad_workspace_bytes(const AstroQNet *net, int32_t n);
int astro_qgrad(const AstroQNet *net, const float *features, int32_t n, int32_t rows,
                const int8_t *action, const float *target, float *loss, float *grad,
                void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ASTRO_QTRAIN_H */
