/*
 * astro_fork.h -- C-ABI of libastro_fork.so: env state copied between slots
 * on the device, within one batch or from one batch to another.
 *
 * A batched simulator's clone_state / restore_state.  The reference has no
 * counterpart to replace: its State is a Python value, copied by assignment,
 * and its generate_configs stream (core.py:77-83) a generator nobody forks.
 * Here an env is a slot of seven arrays in four layouts (astro_step.h
 * AstroState), and the only other way to move one is BatchedEnv.to_host /
 * load_host through numpy, which keeps the destination's seed stream by design.
 *
 *   astro_fork   for every j < m, env dst_ids[j] of `dst` becomes env
 *                src_ids[j] of `src`: its current game, its future games, or
 *                both
 *
 * Conventions: those of astro_step.h and astro_trace.h.  The caller owns all
 * memory; the call is stream-ordered and asynchronous on `stream`; the library
 * never allocates or synchronises; 0 on success, a negative code on a bad
 * argument (-1..-199; this header's own are -160..-169) or a launch failure
 * (-1000 - hipError_t), described by astro_fork_last_error() for the calling
 * thread.
 *
 * A library of its own: it shares the structs of astro_step.h with the others
 * and no symbol.
 */
#ifndef ASTRO_FORK_H
#define ASTRO_FORK_H

#include <stdint.h>

#include "astro_step.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ASTRO_FORK_ABI_VERSION 1

/* `what`: either or both, not 0.
 *
 * ASTRO_FORK_GAME    the current game: every ship row and bearing; all p_pad
 *                    planet slots as they stand; hdr words 0 and 1 as they
 *                    stand (word 0 whole, not masked to the tick);
 *                    stream[4 i + 3], the current game's seed; and the LIVE
 *                    bullet rows [0, nbullets), nbullets from the source's hdr
 *                    word 1 clamped to b_cap.  Bullet rows at or past nbullets
 *                    of the destination are not written.
 * ASTRO_FORK_STREAM  the future games: hdr words 2 and 3 (the pending seed, its
 *                    key_valid / undrawn bits and key[397]); stream[4 i + 0..2],
 *                    the generate_configs cursor; all 624 words of the env's
 *                    stream_ring.
 *
 * With both, the destination env steps bit for bit like the source from then
 * on, through every auto-reset.  With GAME alone it keeps its own stream and
 * pending game (BatchedEnv.load_host's contract).  The split is the header's
 * own ownership rule: words 0-1 are the step wave's, words 2-3 belong to
 * whoever checks the pending seed.
 *
 * Everything else is neither read nor written: envs that no pair names,
 * AstroState.errors, statistics, reward and done buffers, dead bullet rows.
 * Copies are bit for bit. */
enum { ASTRO_FORK_GAME = 1, ASTRO_FORK_STREAM = 2 };

int astro_fork_abi_version(void);
const char *astro_fork_last_error(void);

/* src_ids / dst_ids: device arrays of m int32, or NULL for the identity (id j).
 * A pair with either id outside its state's [0, n_env) is skipped whole.  src
 * and dst share p (nships, p_pad, b_cap; nothing else of p is read) and
 * state_f64; their n_env may differ; they may be the same arrays.
 *
 * Precondition (the ids live on the device: the caller checks it, as
 * astro_amd.fork.check_ids does): the destination ids of a call are distinct,
 * and when src and dst are the same arrays no destination id is another pair's
 * source id.  A pair with src_ids[j] == dst_ids[j] on the same arrays is a
 * no-op.  Where a call violates this, the named destination envs are
 * unspecified; nothing is accessed out of bounds.
 *
 * Argument codes, in the order they are checked (all before the device is touched):
 *   -10 params NULL, -2 src NULL, -160 dst NULL, -11 nships, -13 p_pad, -15 b_cap, -161 m < 0,
 *   (m == 0 returns 0,) -162 what is 0 or has unknown bits, -6 a state_f64 not 0 or 1,
 *   -163 src and dst differ in state_f64, -3 an n_env < 0, (either n_env == 0 returns 0,)
 *   -4 a needed array of src is NULL, -164 a needed array of dst is NULL (ships, ships_b, planets,
 *   hdr, stream always; bullets only with GAME; stream_ring only with STREAM), -5 src alignment,
 *   -165 dst alignment (ships, planets, bullets, hdr, stream, stream_ring to 16 bytes, ships_b to
 *   its element), -166 an id array not 4-byte aligned. */
int astro_fork(const AstroParams *p, const AstroState *src, const AstroState *dst, const int32_t *src_ids,
               const int32_t *dst_ids, int32_t m, int32_t what, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ASTRO_FORK_H */
