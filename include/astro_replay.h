/*
 * astro_replay.h -- C-ABI of libastro_replay.so, the MI355X (gfx950) experience
 * replay of the reference's learner (astro/rl.py, QBotTrainer, rl.py:231-332):
 *
 *   astro_replay_push    <- QBotTrainer.__call__'s _nstep_buffer.append and
 *                           reward()'s flush into n-step experiences
 *                           (rl.py:255, 303-319), for every env at once
 *   astro_replay_sample  <- _step's choice of experiences (rl.py:263-276): the
 *                           unscored ones first, then without replacement with
 *                           probability proportional to the last loss
 *   astro_replay_gather  <- the to_batch of the chosen experiences' state_f and
 *                           new_state_f (rl.py:286-296)
 *   astro_replay_update  <- `xp.loss = float(loss)` (rl.py:298-299)
 *
 * Storage is a time-major ring the caller owns (AstroReplay): tick t lives in
 * row t % ticks.  One feature tensor per (tick, env) serves both ships (ship 1's
 * ego view is the exchange of the two ships' five columns) and every
 * experience's next state (an index to a later row of the same env).
 *
 * Conventions: those of astro_qtrain.h.  The caller owns all memory; every call
 * is stream-ordered and asynchronous on `stream`; the library never allocates
 * or synchronises; 0 on success, a negative code on a bad argument (-1..-199,
 * rejected before the device is touched) or a launch failure (-1000 -
 * hipError_t), described by astro_replay_last_error() for the calling thread.
 *
 * This library is separate from libastro_hip.so, libastro_qnet.so and
 * libastro_qtrain.so and shares nothing with them.
 */
#ifndef ASTRO_REPLAY_H
#define ASTRO_REPLAY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ASTRO_REPLAY_ABI_VERSION 1
#define ASTRO_REPLAY_MAX_ROWS (1 << 16)     /* rows of one feature tensor */
#define ASTRO_REPLAY_MAX_STEPS (1 << 20)    /* n_steps */
#define ASTRO_REPLAY_NEXT_TERMINAL (-1)     /* next: the game ended, there is no next state */
#define ASTRO_REPLAY_NEXT_PENDING (-2)      /* next: the entry's window is still open */

/* The ring.  Every array is device memory, contiguous, S = nships,
 * nf = 5 + 5 * nships.  An experience is one (row, env, ship); its id is
 * (row * n_env + env) * nships + ship, and ticks * n_env * nships must fit an
 * int32. */
typedef struct AstroReplay {
    float *features;     /* [ticks][n_env][rows][nf]: ship 0's ego view (BatchedEnv.features) */
    int8_t *action;      /* [ticks][n_env][S] */
    float *reward;       /* [ticks][n_env][S]: the n-step discounted reward (0 while pending) */
    float *discount;     /* [ticks][n_env]: gamma ** (steps to the next state); 0 while pending */
    int32_t *next;       /* [ticks][n_env]: ring row of the next state, or ASTRO_REPLAY_NEXT_* */
    float *loss;         /* [ticks][n_env][S]: the last loss; +inf = not yet scored */
    int64_t *wstart;     /* [n_env]: the tick at which the env's open window began */
    const double *gpow;  /* [n_steps + 1]: gpow[i] = gamma ** i, computed by the caller in float64 */
    double gamma;        /* the learner's discount, rl.py:241 */
    int32_t n_env;
    int32_t rows;
    int32_t nships;      /* 1 or 2 */
    int32_t ticks;       /* rows of the ring, >= n_steps + 2 */
    int32_t n_steps;     /* rl.py:239 */
    int32_t reserved;    /* 0 */
} AstroReplay;

int astro_replay_abi_version(void);
const char *astro_replay_last_error(void);

/* Argument codes (all entry points):
 *   -100 rb is NULL                  -101 rb.nships not 1 or 2
 *   -102 rb.n_env < 1                -103 rb.rows < 1 or > ASTRO_REPLAY_MAX_ROWS
 *   -104 rb.n_steps < 1 or > ASTRO_REPLAY_MAX_STEPS
 *   -105 rb.ticks < rb.n_steps + 2   -106 ticks * n_env * nships does not fit an int32
 *   -107 rb.gamma is not finite   -108 an array of rb the call uses is NULL
 *   -109 an array of rb the call uses is misaligned (its element size; features 4)
 *   -110 t < 0                       -111 n < 0
 *   -112 control, reward or done is NULL (push)
 *   -113 ids is NULL                 -114 count is NULL (sample)
 *   -115 an output or the loss array is NULL (gather, update)
 *   -118 workspace NULL or smaller than astro_replay_sample_workspace_bytes
 *   -119 an argument array is misaligned (its element size), or workspace not 16-byte aligned
 * rb and its scalars are checked first, in the order above, then t or n, then
 * the call's own pointers; with n == 0 gather and update look at nothing else. */

/* One tick of every env.  `t` is the tick being stored: the number of pushes
 * before this one; its row t % ticks is the ring's head row, whose features
 * the caller has written already (BatchedEnv.features(out=head row)).
 *
 * control: int8 [n_env][S], reward: float32 [n_env][S], done: uint8 [n_env]
 * (nonzero = the game ended on this tick) -- what BatchedEnv.step takes and
 * returns.
 *
 * Per env: action[row] = control, reward[row] = 0, discount[row] = 0,
 * next[row] = PENDING, loss[row] = +inf, L = t - wstart + 1.  When done != 0 or
 * L == n_steps the window closes: for its j-th tick (j = 0 .. L-1, tick
 * k = wstart + j, row k % ticks)
 *   reward[k][s] = float32(double(reward[s]) * gpow[L - 1 - j])
 *   discount[k]  = float32(rb.gamma * gpow[L - 1 - j])
 *   next[k]      = done ? TERMINAL : (t + 1) % ticks
 * and wstart = t + 1.  A wstart outside [max(0, t - n_steps + 1), t] (the
 * caller wrote it) is taken as t.  The features are not touched. */
int astro_replay_push(const AstroReplay *rb, int64_t t, const int8_t *control, const float *reward,
                      const uint8_t *done, void *stream);

/* The selection.  `t` is the number of pushes so far (the head row is t %
 * ticks).  An experience is eligible when its row has been written (row <
 * min(t, ticks)), is not the head row, and its next is neither PENDING nor the
 * head row.  Each eligible experience gets
 *   class  0 if loss == +inf, 1 if loss > 0 and finite, 2 otherwise
 *   z      splitmix64's mix of id * 0x9E3779B97F4A7C15 + (draw + 1) * 0xD1B54A32D192ED03 + seed
 *   E      -log(((z >> 11) + 0.5) * 2^-53) in float64
 *   key    float32(E) for class 0, float32(E / double(loss)) for class 1, 0 for class 2
 * and the min(n, eligible) experiences smallest in (class, key, id) are
 * written to ids[0 .. count) in ascending id order; *count (a device word)
 * receives their number.  ids has room for n; elements from count on are not
 * written.
 *
 * The device's float64 log is within 3 ulp of the exact value, so a key can
 * differ in its last bit from another implementation's.
 *
 * Determinism: integer atomics only, and the output order comes from a scan.
 * For the same ring, t, n, seed and draw the result is bit-identical from call
 * to call, whatever the workspace held.
 *
 * workspace: device scratch of at least astro_replay_sample_workspace_bytes(rb)
 * bytes, 16-byte aligned; unspecified on return.  The query returns 0 for a
 * NULL or invalid rb. */
size_t astro_replay_sample_workspace_bytes(const AstroReplay *rb);
int astro_replay_sample(const AstroReplay *rb, int64_t t, int32_t n, uint64_t seed, uint64_t draw, int32_t *ids,
                        int32_t *count, void *workspace, size_t workspace_bytes, void *stream);

/* The chosen experiences as training tensors.
 *
 * ids:           int32 [n]
 * features:      float32 [n][rows][nf]: the experience's state, in its ship's ego view
 * action:        int8 [n]
 * reward:        float32 [n]
 * discount:      float32 [n]
 * next_features: float32 [n][rows][nf]: the state at row `next`, same view
 * terminal:      uint8 [n]: 1 where next is TERMINAL
 *
 * Of features and next_features, column 0 of every row is exact and every
 * column of a live row (column 0 not < 0) is exact; the other columns of
 * padding rows are not written (astro_qforward and astro_qgrad never read
 * them).  A terminal sample's next_features has column 0 = -1 in every row and
 * nothing else written.  An id outside the ring, or one whose next is
 * PENDING, reads nothing out of bounds: it gives column 0 = -1 throughout
 * (next_features; for an id outside the ring also features), action -1,
 * reward 0, discount 0 and terminal 1 for the former, and the stored values
 * with terminal 0 for the latter.  n == 0 returns 0 and touches nothing. */
int astro_replay_gather(const AstroReplay *rb, const int32_t *ids, int32_t n, float *features, int8_t *action,
                        float *reward, float *discount, float *next_features, uint8_t *terminal, void *stream);

/* rb.loss[ids[i]] = loss[i] for i < n.  An id outside the ring is skipped; an
 * id that occurs twice receives one of its values.  n == 0 returns 0 and
 * touches nothing. */
int astro_replay_update(const AstroReplay *rb, const int32_t *ids, const float *loss, int32_t n, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ASTRO_REPLAY_H */
