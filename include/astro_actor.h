/*
 * astro_actor.h -- C-ABI of libastro_actor.so, the MI355X (gfx950) acting side of
 * the reference's trainer (astro/rl.py) around astro_step:
 *
 *   astro_explore   <- rl.EpsilonGreedy (rl.py:10-29) as QBotTrainer uses it
 *                      (rl.py:235-238, 253-254): the two-state sticky exploration
 *                      of every ship of every env, in place on a control array
 *   astro_episodes  <- the per-game bookkeeping rl.train logs (rl.py:352-369) and
 *                      core.play returns (core.py:377-410): winner and length of
 *                      every finished game, from what astro_step returns
 *
 * Conventions: those of astro_replay.h.  The caller owns all memory; every call
 * is stream-ordered and asynchronous on `stream`; the library never allocates
 * or synchronises; 0 on success, a negative code on a bad argument (-1..-199,
 * rejected before the device is touched) or a launch failure (-1000 -
 * hipError_t), described by astro_actor_last_error() for the calling thread.
 *
 * This library is separate from the other four.  It shares only the structs of
 * astro_step.h (AstroParams for nships, AstroState for n_env and the header
 * array), as astro_qnet.h does.
 *
 * What differs from the reference's EpsilonGreedy: numpy's random stream is not
 * reproduced (the words are the project's splitmix64 of ship id, draw and
 * seed), and the time between two ticks is the constant config.dt where the
 * reference subtracts two accumulated floats (a last-place difference in a
 * probability).
 */
#ifndef ASTRO_ACTOR_H
#define ASTRO_ACTOR_H

#include <stddef.h>
#include <stdint.h>

#include "astro_step.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ASTRO_ACTOR_ABI_VERSION 1
#define ASTRO_EXPLORE_ONE (1ull << 53)   /* a threshold of 1.0: the state never moves */
#define ASTRO_EXPLORE_MAX_RANDOM 6       /* the controls are 0..5 */

/* The exploration state and its constants.
 *
 * stay_out = ceil(exp(-dt / t_in) * 2^53) and stay_in = ceil(exp(-dt / t_out) *
 * 2^53), computed once by the caller in float64: the probability, in units of
 * 2^-53, that a ship without (with) a random policy keeps that state over one
 * tick.  t = inf gives 2^53 (never moves), t -> 0 gives 0 (always moves). */
typedef struct AstroExplore {
    int8_t *policy;      /* device [n_env][nships]: -1 = none held, else the held control 0..nrandom-1 */
    uint64_t stay_out;   /* <= 2^53 */
    uint64_t stay_in;    /* <= 2^53 */
    uint64_t seed;
    int64_t env_offset;  /* global id of env 0 (shards) */
    int32_t nrandom;     /* 1..6: an entered control is uniform on 0..nrandom-1 (rl.py:24: 5) */
    int32_t reserved;    /* 0 */
} AstroExplore;

/* The bookkeeping of every env's games.  Every array is device memory. */
typedef struct AstroEpisodes {
    int32_t *length;     /* [n_env]: ticks of the open game so far */
    int32_t *got;        /* [n_env]: games finished */
    int8_t *winner;      /* [n_env][games]: game g's winning ship, -1 = none (draw or timeout) */
    int32_t *ticks;      /* [n_env][games]: game g's length in ticks */
    int32_t *wins;       /* [n_env][nships]: games won by each ship, recorded or not */
    int32_t *finished;   /* [n_env]: games finished, recorded or not (= got) */
    int64_t *tick_sum;   /* [n_env]: the sum of their lengths */
    int32_t n_env;
    int32_t nships;      /* 1 or 2 */
    int32_t games;       /* >= 1: games recorded per env */
    int32_t reserved;    /* 0 */
} AstroEpisodes;

int astro_actor_abi_version(void);
const char *astro_actor_last_error(void);

/* Argument codes:
 *   -100 p, s or ex is NULL (explore); ep is NULL (episodes)
 *   -101 nships not 1 or 2           -102 n_env < 1
 *   -103 ex.nrandom outside 1..6     -104 ex.stay_out or ex.stay_in above 2^53
 *   -105 ep.games < 1                -106 n_env * nships or n_env * games does not fit an int32
 *   -108 s.hdr, ex.policy or an array of ep is NULL
 *   -109 s.hdr or an array of ep is misaligned (its element size; hdr 16)
 *   -112 control is NULL (explore); reward or done is NULL (episodes)
 *   -119 reward is not 4-byte aligned
 * in that order. */

/* rl.EpsilonGreedy.__call__ for every ship, then the override of rl.py:254.
 *
 * p is read for nships, s for n_env and hdr (each env's tick counter,
 * hdr[4 * i] & 0x3fffff).  control: device int8 [n_env][nships].
 *
 * Ship s of env i has the global id g = (ex.env_offset + i) * nships + s.
 *   tick == 0: no transition (in the reference dt = state.t - self._t <= 0 on a
 *     game's first tick and exp(-dt / t) >= 1 is never below rand()): a held
 *     policy carries over from the previous game.
 *   otherwise k = z(g) >> 11, where z(x) is splitmix64's mix of
 *     x * 0x9E3779B97F4A7C15 + (draw + 1) * 0xD1B54A32D192ED03 + seed (mod 2^64):
 *       policy < 0:  if k >= stay_out, policy = ((z(g + 2^63) >> 32) * nrandom) >> 32
 *       else:        if k >= stay_in, policy = -1
 *     (at most one transition per call, the reference's elif).
 * Then control = policy where policy >= 0; the other controls are not touched.
 * Integer arithmetic only: a restatement in any language agrees bit for bit. */
int astro_explore(const AstroParams *p, const AstroState *s, const AstroExplore *ex, int64_t draw, int8_t *control,
                  void *stream);

/* One tick of bookkeeping.  reward: float32 [n_env][nships], done: uint8 [n_env]
 * (nonzero = the game ended on this tick) -- what astro_step returned.
 *
 * Per env: length += 1.  When done != 0: w = the first ship whose reward is the
 * maximum if that maximum is >= 1, else -1 (core.py:409); if got < games,
 * winner[got] = w and ticks[got] = length; if w >= 0, wins[w] += 1;
 * finished += 1; tick_sum += length; got += 1; length = 0. */
int astro_episodes(const AstroEpisodes *ep, const float *reward, const uint8_t *done, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ASTRO_ACTOR_H */
