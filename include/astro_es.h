/*
 * astro_es.h -- C-ABI of libastro_es.so: an antithetic evolution strategy on a
 * packed float32 parameter buffer (a Q-network's weights, astro_qnet.h).
 *
 * Every learner of the project follows a surrogate's gradient (a TD error, a
 * value regression).  This one follows the outcome of games: a population of
 * perturbed copies of the parameters plays, each copy's games are counted into
 * one fitness, and the fitness differences of the antithetic pairs, weighted
 * by the noise that made them, estimate the fitness's gradient.  The reference
 * has no counterpart.
 *
 *   astro_es_perturb    theta +- sigma * eps for a run of pairs, into rows
 *   astro_es_score      per member of a blocked env batch: wins, losses and
 *                       games without a winner, and one fitness
 *   astro_es_gradient   utilities of the fitness (centred ranks or raw) and
 *                       the gradient estimate for a minimising optimiser
 *
 * Conventions: those of astro_search.h.  The caller owns all memory; the calls
 * are stream-ordered and asynchronous on `stream`; the library never allocates
 * or synchronises; 0 on success, a negative code on a bad argument (-1..-199;
 * this header's own are -180..-189) or a launch failure (-1000 - hipError_t),
 * described by astro_es_last_error() for the calling thread.  Every result is
 * bit-identical from call to call: no float atomics, integer sums only where
 * the order is free.
 *
 * A library of its own: it shares no struct and no symbol with the others.
 *
 * THE NOISE.  For (seed, generation g, pair j, parameter p):
 *   word = the project's random word (splitmix64 of id * 0x9E3779B97F4A7C15 +
 *          (draw + 1) * 0xD1B54A32D192ED03 + seed) with
 *          id = ((uint64_t)j << 32) | p and draw = (uint64_t)g
 *   s    = the sum of the word's four 16-bit fields, 0 .. 262140
 *   eps  = (float)(s - 131070) * 0x1.bb67aep-16f
 * The constant is float32 of sqrt(3 / (2^32 - 1)): a sum of four uniform 16-bit
 * integers has mean 131070 and variance (2^32 - 1) / 3, so eps has mean 0 and
 * variance 1, and |eps| <= 131070 * 0x1.bb67aep-16f (about 3.46).  s - 131070
 * is exact in float32: eps costs one float32 multiply.  The noise is never
 * stored: astro_es_gradient regenerates what astro_es_perturb used.
 */
#ifndef ASTRO_ES_H
#define ASTRO_ES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ASTRO_ES_ABI_VERSION 1

#define ASTRO_ES_MAX_PAIRS 512           /* pairs of one population */
#define ASTRO_ES_MAX_MEMBERS 1024        /* astro_es_score's nmembers: 2 * ASTRO_ES_MAX_PAIRS */
#define ASTRO_ES_MAX_PARAMS (1 << 20)    /* astro_qopt.h's ASTRO_QOPT_MAX_PARAMS */

#define ASTRO_ES_RANKS 0 /* shaping: centred ranks, ties share the average rank */
#define ASTRO_ES_RAW 1   /* shaping: the fitness itself */

/* One population: `pairs` antithetic pairs around a centre of `nparams` floats. */
typedef struct AstroES {
    uint64_t seed;
    int64_t generation; /* g: the draw of the noise; any value */
    int32_t nparams;    /* 1 .. ASTRO_ES_MAX_PARAMS */
    int32_t pairs;      /* 1 .. ASTRO_ES_MAX_PAIRS */
    float sigma;        /* finite and > 0 */
    int32_t reserved;   /* 0 */
} AstroES;

int astro_es_abi_version(void);
const char *astro_es_last_error(void);

/* members: float32 [2 * npairs][nparams].  For i in [0, npairs) and pair j = first_pair + i:
 *   d = sigma * eps_j[p]            one float32 multiply
 *   members[2 i][p]     = theta[p] + d
 *   members[2 i + 1][p] = theta[p] - d
 * each a float32 add of its own (nothing is contracted; astro_qopt_step's rule).  theta (float32 [nparams]) is not
 * written; members may not overlap it.  npairs == 0 does nothing.
 *
 * Argument codes, in the order they are checked (all before the device is touched):
 *   -180 es NULL, -181 nparams outside [1, ASTRO_ES_MAX_PARAMS], -182 pairs outside [1, ASTRO_ES_MAX_PAIRS],
 *   -183 sigma not finite or not > 0, -184 first_pair < 0, npairs < 0 or first_pair + npairs > pairs,
 *   (npairs == 0 returns 0,) -185 theta or members NULL, -186 members overlaps theta, -189 theta or members not
 *   4-byte aligned. */
int astro_es_perturb(const AstroES *es, const float *theta, int32_t first_pair, int32_t npairs, float *members,
                     void *stream);

/* winner: int8 [n_env][games], ticks: int32 [n_env][games], as astro_actor.h's AstroEpisodes keeps them.  Member k
 * of K = nmembers owns the envs [k * n_env / K, (k + 1) * n_env / K) (the products in 64 bits): the blocks of
 * astro_amd.league.Pool.versus.  A block may be empty.
 *
 * Per game of a member's envs, from the seat `ship`: winner == ship is a win (W), -1 a game without a winner (D),
 * -2 a game not played, which is not counted, and any other value a loss (L).  lost = the sum of
 * min(ticks, timeout_tick) over the lost games (how long the member survived).
 *   counts     int32 [K][3] or NULL: W, L, D
 *   lost_ticks int64 [K] or NULL: lost
 *   fitness    float32 [K]: (float)((((double)(W - L) + draw * (double)D)
 *                                    + survive * ((double)lost / (double)timeout_tick)) / (double)(W + L + D)),
 *              float64 operations in that order, rounded once; NaN (0x7fc00000) when W + L + D == 0
 * The sums are integers: the order of the reduction does not matter.  Every element of the outputs given is written,
 * with n_env == 0 too.
 *
 * Argument codes, in the order they are checked:
 *   -3 n_env < 0, -187 games < 1, n_env * games beyond an int32, nmembers outside [1, ASTRO_ES_MAX_MEMBERS] or
 *   timeout_tick < 1, -11 ship not 0 or 1 (a game has one or two ships), -183 draw or survive not finite,
 *   -185 fitness NULL, or winner or ticks NULL with n_env > 0, -189 ticks, counts or fitness not 4-byte, or
 *   lost_ticks not 8-byte aligned. */
int astro_es_score(const int8_t *winner, const int32_t *ticks, int32_t n_env, int32_t games, int32_t nmembers,
                   int32_t ship, double draw, double survive, int32_t timeout_tick, int32_t *counts,
                   int64_t *lost_ticks, float *fitness, void *stream);

/* fitness: float32 [K], K = 2 * pairs; members 2 j and 2 j + 1 are pair j's + and - (astro_es_perturb's rows).
 * Utilities u, float32 [K] (written to `utilities` if it is not NULL):
 *   ASTRO_ES_RANKS  u_k = (float)(2 * #{j : f_j < f_k} + #{j != k : f_j == f_k}) / (float)(2 * (K - 1)) - 0.5f
 *                   (one float32 divide, one float32 subtract; with pairs == 1 the divisor is 2)
 *   ASTRO_ES_RAW    u_k = f_k
 *   either          if any f is not finite, every u is 0 (and so is the gradient)
 * grad: float32 [nparams], every element written:
 *   a = 0.0; for j = 0 .. pairs - 1 in order: a = a + (double)(u[2 j] - u[2 j + 1]) * (double)eps_j[p]
 *   grad[p] = (float)(-a / ((2.0 * (double)pairs) * (double)sigma))
 * with the difference of the two utilities taken in float32.  The sign is for an optimiser that minimises
 * (astro_qopt_step): stepping along -grad ascends the fitness.
 *
 * Argument codes, in the order they are checked:
 *   -180 es NULL, -181 nparams, -182 pairs, -183 sigma (as astro_es_perturb), -188 shaping unknown,
 *   -185 fitness or grad NULL, -189 fitness, utilities or grad not 4-byte aligned. */
int astro_es_gradient(const AstroES *es, const float *fitness, int32_t shaping, float *utilities, float *grad,
                      void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ASTRO_ES_H */
