/*
 * astro_qpool.h -- C-ABI of libastro_qpool.so: astro_qnet.h's fused Q-network
 * policy with a POOL of networks, each playing one ship of a block of envs.
 *
 * astro_qvalues evaluates one network for every ship of every env and
 * astro_qvalues_ships (astro_qduel.h) one network per ship.  This library's
 * one entry point takes up to ASTRO_QPOOL_MAX_NETS networks and a table of
 * spans -- "ship s of the envs [lo, hi) is played by nets[k]" -- so that a
 * learner can meet a pool of opponents of different ages, or every pairing of
 * a tournament can be played, in ONE launch per tick.
 *
 * Conventions: those of astro_step.h and astro_qnet.h.  The caller owns all
 * memory; the call is stream-ordered and asynchronous on `stream`; the library
 * never allocates or synchronises; 0 on success, a negative code on a bad
 * argument (-1..-199) or a launch failure (-1000 - hipError_t), described by
 * astro_qpool_last_error() for the calling thread.  `nets` and `spans` are
 * HOST arrays, read before the call returns: the kernel receives the weight
 * pointers and the span table by value.
 *
 * A library of its own: it shares the structs of astro_step.h and astro_qnet.h
 * with the others and no symbol.
 */
#ifndef ASTRO_QPOOL_H
#define ASTRO_QPOOL_H

#include <stdint.h>

#include "astro_qnet.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ASTRO_QPOOL_ABI_VERSION 1
#define ASTRO_QPOOL_MAX_NETS 32
#define ASTRO_QPOOL_MAX_SPANS 64

typedef struct AstroQSpan {
    int32_t ship;   /* 0 .. nships-1 */
    int32_t net;    /* index into nets[], or -1: the span is skipped */
    int32_t lo, hi; /* envs [lo, hi), 0 <= lo <= hi <= n_env; lo == hi is allowed */
} AstroQSpan;

int astro_qpool_abi_version(void);
const char *astro_qpool_last_error(void);

/* astro_qvalues with a network per span.  For every span with net >= 0, ship span.ship of every
 * env in [lo, hi) gets the q rows and the control entry that astro_qvalues with nets[span.net]
 * writes for that ship of that env, bit for bit: q / control layout, the ego view, clamped counts,
 * float32 arithmetic, the first-maximum rule and the coin keyed by (env_offset + i, ship, tick0,
 * seed) are astro_qvalues' contract word for word.  Nothing else is read or written: a (ship, env)
 * that no span with a network covers keeps its bits in q and control, and its state is not loaded.
 *
 * The spans of one ship must not overlap (empty spans overlap nothing; a skipped span counts).  A
 * network is USED if a span names it; the used networks must have nships == p->nships and equal
 * nout; the others are not looked at.  max_blocks: 0 = the library's default cap, > 0 = at most
 * that many workgroups.  A workgroup stages one network's weights and serves 32-env chunks of a
 * span, counted from lo; when the cap allows, every non-empty span has workgroups of its own, in
 * proportion to its chunks; otherwise (max_blocks below the number of non-empty spans) a workgroup
 * serves several spans one after the other and restages when the network changes.
 *
 * Argument codes, in the order they are checked (all before the device is touched):
 *   -10 params NULL, -2 state NULL, -120 nets NULL, -130 spans NULL, -11 nships, -13 p_pad,
 *   -15 b_cap, -131 nnets not in [1, ASTRO_QPOOL_MAX_NETS], -132 nspans not in
 *   [1, ASTRO_QPOOL_MAX_SPANS], -3 n_env < 0, -133 a span's ship, -134 a span's net index,
 *   -135 a span's bounds, -136 two spans of one ship overlap, -101 a used net's nships,
 *   -102 a used net's nout, -122 the used nets differ in nout, -103 q and control both NULL,
 *   -104 epsilon, -123 max_blocks < 0, (no span with a network and an env: returns 0 and launches
 *   nothing,) -105 a used net's weights, -4 a state array is NULL, -5 state alignment,
 *   -6 state_f64, -106 q alignment. */
int astro_qvalues_pool(const AstroParams *p, const AstroState *s, const AstroQNet *nets, int32_t nnets,
                       const AstroQSpan *spans, int32_t nspans, float *q, int8_t *control,
                       const AstroPolicy *explore, double epsilon, int32_t max_blocks, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ASTRO_QPOOL_H */
