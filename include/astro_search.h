/*
 * astro_search.h -- C-ABI of libastro_search.so: the outputs of a branched
 * step plus rollout reduced to one value per (env, control) and a decision.
 *
 * A one-ply search over copies of the game (astro_amd.fork.Lookahead) steps
 * every copy once with its own first control, rolls all copies on for a
 * horizon, and then asks of every branch: when did it end first, what was it
 * worth then, and if it did not end, what does a Q-network think of where it
 * stands?  The reference has no counterpart: its bots decide from one state.
 *
 *   astro_search_values   value[i][a] for the six controls of every env, the
 *                         control to play and (optionally) each branch's first
 *                         done tick, in one launch
 *
 * Conventions: those of astro_fork.h.  The caller owns all memory; the call is
 * stream-ordered and asynchronous on `stream`; the library never allocates or
 * synchronises; 0 on success, a negative code on a bad argument (-1..-199;
 * this header's own are -170..-179) or a launch failure (-1000 - hipError_t),
 * described by astro_search_last_error() for the calling thread.
 *
 * A library of its own: it shares no struct and no symbol with the others.
 */
#ifndef ASTRO_SEARCH_H
#define ASTRO_SEARCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ASTRO_SEARCH_ABI_VERSION 1

#define ASTRO_SEARCH_NCONTROL 6 /* A: a ship's controls, and a leaf row's values */

/* The shape and the inputs (device pointers; none is written).
 *
 * N envs, A = 6 own controls, R replies: M = N * A * R branches, branch
 * m = (i * A + a) * R + o.  S ships; the values are ship `ship`'s.  K ticks.
 *
 * Per branch: t* is the first t < K whose done byte (done0 for t = 0, done[t - 1]
 * after) is non-zero -- 1 a collision, 2 a timeout, any non-zero byte counts.
 *   t* exists       b = gamma[t*] * (that tick's reward of `ship`): one float32
 *                   multiply.  Later done ticks are ignored whatever their
 *                   reward: with auto-reset they belong to the next game.
 *   else, leaf      b = gamma[K] * qmax, qmax = q[0] folded with fmaxf left to
 *                   right over leaf[m][ship][0..5] (astro_qforward's qmax)
 *   else            b = 0.0f
 * Per (env, control): v = b of reply 0; then for o = 1..R-1 in order, v = b_o
 * where b_o < v (the opponent's worst reply; R == 1 compares nothing). */
typedef struct AstroSearch {
    const float *reward0;  /* [M][S]        what the step returned for tick 0 */
    const uint8_t *done0;  /* [M] */
    const float *reward;   /* [K-1][M][S]   what the rollout returned for ticks 1..K-1; NULL allowed with K == 1 */
    const uint8_t *done;   /* [K-1][M]      the same */
    const float *gamma;    /* [K+1]         float32(discount ** t), t = 0..K */
    const float *leaf;     /* [M][S][6] or NULL: Q values of the branch's last state; only `ship`'s rows are read */
    int32_t n_env;         /* N */
    int32_t replies;       /* R: 1 or 6 */
    int32_t nships;        /* S: 1 or 2 */
    int32_t ship;          /* in [0, S) */
    int32_t horizon;       /* K >= 1 */
    int32_t reserved;      /* 0 */
} AstroSearch;

int astro_search_abi_version(void);
const char *astro_search_last_error(void);

/* value: float32 [N][6], every element written.
 * control: int8 [N] or NULL.  With it `own` (int8 [N], each env's default
 * control) is required: control[i] = own[i] unless some value[i][a] is strictly
 * greater than value[i][own[i]], then the first maximal a; an own[i] outside
 * 0..5 gives the first maximal a.
 * first: int32 [M] or NULL: t*, or -1.
 * Nothing else is written.  With K == 1 `reward` and `done` are not read.
 *
 * Argument codes, in the order they are checked (all before the device is touched):
 *   -170 s NULL, -3 n_env < 0, -11 nships not 1 or 2, -171 ship outside [0, nships), -172 horizon < 1,
 *   -173 replies not 1 or 6, -174 n_env * 6 * replies * nships * 6 (a leaf's element count) does not fit an int32,
 *   -175 value NULL, -176 control given without own, (n_env == 0 returns 0,) -177 reward0, done0 or gamma
 *   NULL, -178 reward or done NULL with horizon > 1, -179 a float or int32 array not 4-byte aligned. */
int astro_search_values(const AstroSearch *s, float *value, const int8_t *own, int8_t *control, int32_t *first,
                        void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ASTRO_SEARCH_H */
