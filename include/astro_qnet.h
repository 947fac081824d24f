/*
 * astro_qnet.h -- C-ABI of libastro_qnet.so, the MI355X (gfx950) fused
 * Q-network policy over the batched state of astro_step.h.
 *
 * The reference's learned policy (astro/rl.py) evaluates, for every ship and
 * every tick, a small network on the features of the ship's ego view:
 *
 *   astro_qvalues  <- rl.ValueNetwork.forward(get_features(roll_ships(state, s)))
 *                     (rl.py:36-72, 137-155) for every env and ship, then
 *                     rl.QBot.__call__'s argmax (rl.py:195-209), optionally
 *                     mixed with a uniform random control (epsilon-greedy)
 *
 * in ONE kernel that reads the AstroState arrays directly: each live object
 * row's features are built in registers, the per-row layers and the head run
 * on the f32-input MFMA, and only q / control are written.  The feature
 * tensor astro_features would write is never materialised.
 *
 * Conventions: those of astro_step.h.  The caller owns all memory; the call
 * is stream-ordered and asynchronous on `stream`; the library never
 * allocates or synchronises; 0 on success, a negative code on a bad argument
 * (-1..-199) or a launch failure (-1000 - hipError_t), described by
 * astro_qnet_last_error() for the calling thread.
 *
 * This library is separate from libastro_hip.so and shares only the structs
 * of astro_step.h (AstroParams, AstroState, AstroPolicy) with it.
 */
#ifndef ASTRO_QNET_H
#define ASTRO_QNET_H

#include <stdint.h>

#include "astro_step.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ASTRO_QNET_ABI_VERSION 1
#define ASTRO_QNET_HIDDEN 32          /* rl.py:140: nh, d = 32, 2 */
#define ASTRO_QNET_MAX_OUT 6          /* the six controls of core.step */

/* The network: f0 (nf -> 32), f.0, f.1 (32 -> 32) on every object row with
 * softsign between, a max over the env's live rows, v.0, v.1 (32 -> 32) with
 * softsign after each, v0 (32 -> nout) and tanh. */
typedef struct AstroQNet {
    const float *weights;  /* device; float32, state_dict order, torch's [out][in] rows:
                              f0.weight[32][nf] f0.bias[32]  f.0.weight[32][32] f.0.bias[32]  f.1.*  v.0.*  v.1.*
                              v0.weight[nout][32] v0.bias[nout];  nf = 5 + 5*nships
                              (32*nf + 32 + 4*(32*32 + 32) + 33*nout floats, 4-byte aligned) */
    int32_t nships;        /* must equal AstroParams.nships */
    int32_t nout;          /* 1..6 */
} AstroQNet;

int astro_qnet_abi_version(void);
const char *astro_qnet_last_error(void);

/* Q values and controls of every ship of every env on the current state.
 *
 * Ship s of env i sees its ego view (core.roll_ships: its own ship first).
 * The network's input rows are exactly the float32 values astro_features
 * writes for that view: row r < nplanets is planet r, then the live bullets;
 * column 0 is 0 (planet) or 1 (bullet); then every ship's (x, y, dx, dy,
 * norm_angle(b)/pi) -- the bearing in float32 at a game's first tick, in
 * float64 then cast after; then the object's (x, y, dx, dy).  Counts are
 * clamped as astro_features clamps them (1 <= nplanets <= p_pad, nbullets <=
 * b_cap); slots past the counts are never read.  All arithmetic is float32.
 *
 * q:       float [n_env][nships][nout], or NULL
 * control: int8  [n_env][nships], or NULL: the first maximal index of the
 *          kernel's own q (np.argmax).  With `explore` non-NULL and z the
 *          splitmix64 word ASTRO_POLICY_RANDOM draws for (explore->env_offset
 *          + i, s, explore->tick0, explore->seed): when uint32(z) <
 *          epsilon * 2^32 the control is that draw's own uniform control
 *          ((z >> 32) * 6) >> 32 instead -- epsilon = 1 reproduces
 *          astro_controls with ASTRO_POLICY_RANDOM exactly, for any sharding.
 * explore: NULL (greedy) or an AstroPolicy whose seed / tick0 / env_offset
 *          are used; epsilon in [0, 1].
 * q and control may not both be NULL. */
int astro_qvalues(const AstroParams *p, const AstroState *s, const AstroQNet *net, float *q,
                  int8_t *control, const AstroPolicy *explore, double epsilon, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ASTRO_QNET_H */
