/*
 * astro_seats.h -- C-ABI of libastro_seats.so: astro_controls (astro_step.h)
 * with a table of SEATS, each a scripted bot with its own arguments playing
 * one ship of a block of envs.
 *
 * astro_controls runs one bot per ship for every env, and ScriptBot's two
 * arguments travel in AstroPolicy as one script_r2 / script_threshold pair for
 * the whole launch.  This library's one entry point takes up to ASTRO_SEATS_MAX
 * seats -- "ship s of the envs [lo, hi) is played by this bot with these
 * arguments" -- so that two ScriptBots with different arguments can meet in one
 * env, a learner can meet a ladder of scripted opponents next to a pool of
 * networks (astro_qpool.h), or a scripted bot can be a member of a tournament,
 * in ONE launch per tick.
 *
 * Conventions: those of astro_step.h and astro_qpool.h.  The caller owns all
 * memory; the call is stream-ordered and asynchronous on `stream`; the library
 * never allocates or synchronises; 0 on success, a negative code on a bad
 * argument (-1..-199) or a launch failure (-1000 - hipError_t), described by
 * astro_seats_last_error() for the calling thread.  `seats` is a HOST array,
 * read before the call returns: the kernel receives the seat table by value.
 *
 * A library of its own: it shares the structs of astro_step.h with the others
 * and no symbol.
 */
#ifndef ASTRO_SEATS_H
#define ASTRO_SEATS_H

#include <stdint.h>

#include "astro_step.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ASTRO_SEATS_ABI_VERSION 1
#define ASTRO_SEATS_MAX 64

typedef struct AstroSeat {
    int32_t ship;            /* 0 .. nships-1 */
    int32_t bot;             /* a bot code of astro_step.h (0 nothing, 1 script, 2 random), or -1: skipped */
    int32_t lo, hi;          /* envs [lo, hi), 0 <= lo <= hi <= n_env; lo == hi allowed */
    double script_r2;        /* script bots: as AstroPolicy.script_r2 */
    double script_threshold; /* script bots: as AstroPolicy.script_threshold */
} AstroSeat;                 /* 32 bytes */

int astro_seats_abi_version(void);
const char *astro_seats_last_error(void);

/* astro_controls with a bot, and a ScriptBot's arguments, per seat.  For every seat with bot >= 0,
 * ship seat.ship of every env in [lo, hi) gets in control[env][ship] (int8 [n_env][nships]) the byte
 * that astro_controls writes there, bit for bit, when it is called with ASTRO_POLICY_BOTS, that bot
 * for that ship, and an AstroPolicy equal to `base` except for the seat's script_r2 /
 * script_threshold.  `base` supplies seed, tick0, env_offset (the random bot's draw is keyed by the
 * global ship id and the tick, as astro_controls') and the four config constants (ship_thrust,
 * ship_rspeed, bullet_speed, ship_radius); its kind, bots, script_r2 and script_threshold are
 * ignored.  Nothing else is read or written: a (ship, env) that no seat with a bot covers keeps its
 * byte, and an env with no covered ship is not loaded.
 *
 * The seats of one ship must not overlap (empty seats overlap nothing; a skipped seat counts).  The
 * kernel is one lane per env over the envs between the lowest lo and the highest hi of the seats
 * with a bot and an env; each lane finds its ships' seats by a scan of the table.
 *
 * Argument codes, in the order they are checked (all before the device is touched):
 *   -10 params NULL, -2 state NULL, -140 base NULL, -141 seats NULL, -11 nships, -13 p_pad,
 *   -15 b_cap, -142 nseats not in [1, ASTRO_SEATS_MAX], -3 n_env < 0, -143 a seat's ship,
 *   -144 a seat's bot, -145 a seat's bounds, -146 two seats of one ship overlap, -147 control NULL,
 *   (no seat with a bot and an env: returns 0 and launches nothing,) -4 a state array is NULL,
 *   -5 state alignment, -6 state_f64. */
int astro_controls_seats(const AstroParams *p, const AstroState *s, const AstroPolicy *base,
                         const AstroSeat *seats, int32_t nseats, int8_t *control, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ASTRO_SEATS_H */
