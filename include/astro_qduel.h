/*
 * astro_qduel.h -- C-ABI of libastro_qduel.so: astro_qnet.h's fused Q-network
 * policy with one network PER SHIP, or none.
 *
 * astro_qvalues evaluates one network for every ship of every env.  This
 * library's one entry point takes a network for each ship, so that two
 * different networks can play each other (core.play(config, bots) with two
 * learned bots, util.p_better / find_better's comparison, self-play against a
 * frozen snapshot), and lets a ship go without: a ship that a scripted policy
 * plays costs nothing.
 *
 * Conventions: those of astro_step.h and astro_qnet.h.  The caller owns all
 * memory; the call is stream-ordered and asynchronous on `stream`; the library
 * never allocates or synchronises; 0 on success, a negative code on a bad
 * argument (-1..-199) or a launch failure (-1000 - hipError_t), described by
 * astro_qduel_last_error() for the calling thread.
 *
 * A library of its own: it shares the structs of astro_step.h and astro_qnet.h
 * with the others and no symbol.
 */
#ifndef ASTRO_QDUEL_H
#define ASTRO_QDUEL_H

#include <stdint.h>

#include "astro_qnet.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ASTRO_QDUEL_ABI_VERSION 1

int astro_qduel_abi_version(void);
const char *astro_qduel_last_error(void);

/* astro_qvalues with one network per ship.  nets[s] == NULL: ship s is not evaluated and its
 * entries of q and control are not written (not even read).  For nships == 1 only nets[0] is used.
 * All non-NULL nets: nships == p->nships, equal nout.  max_blocks: 0 = the library's default cap,
 * > 0 = at most that many workgroups (tuning, and so a test can reach a wave's second and third
 * chunk with a few hundred envs).  Everything else -- q / control layout, the ego view, clamped
 * counts, float32 arithmetic, the first-maximum rule, the coin keyed by (env_offset + i, s, tick0,
 * seed) -- is astro_qvalues' contract word for word, and so is every bit of what is written: ship
 * s's q and control equal those of astro_qvalues with *nets[s].
 *
 * A workgroup serves one ship; with two networks and an odd max_blocks > 1 one workgroup fewer is
 * launched, and with max_blocks == 1 the one workgroup serves the ships one after the other.
 *
 * Argument codes, in the order they are checked (all before the device is touched):
 *   -10 params NULL, -2 state NULL, -120 nets NULL, -11 nships, -13 p_pad, -15 b_cap,
 *   -121 every net is NULL, -101 a net's nships, -102 a net's nout, -122 the nets differ in nout,
 *   -103 q and control both NULL, -104 epsilon, -123 max_blocks < 0, -3 n_env < 0,
 *   (n_env == 0 returns 0,) -105 a net's weights, -4 a state array is NULL, -5 state alignment,
 *   -6 state_f64, -106 q alignment. */
int astro_qvalues_ships(const AstroParams *p, const AstroState *s, const AstroQNet *const nets[2],
                        float *q, int8_t *control, const AstroPolicy *explore, double epsilon,
                        int32_t max_blocks, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ASTRO_QDUEL_H */
