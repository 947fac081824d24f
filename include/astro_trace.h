/*
 * astro_trace.h -- C-ABI of libastro_trace.so: whole games of a few chosen
 * envs of a batch, recorded on the device.
 *
 * The reference's trainer saves a validation game with core.save_log
 * (rl.py:352-355): per tick the state the bots saw, their controls, the step's
 * reward and QBot.data, dict(q=...) (rl.py:195-209), which the viewer paints
 * (static/astro.js:129-143).  Here a tick of a batch is two launches -- the
 * policy and astro_step -- and its state never leaves the device.  This
 * library gathers what a Tick is made of, for m chosen envs, into a small ring
 * the caller owns and copies to the host whenever it synchronises anyway:
 *
 *   astro_trace_state   BEFORE the step: the envs' states as the policy saw
 *                       them, the controls the step will take, the Q values
 *   astro_trace_result  AFTER the step: its reward and done
 *
 * Two calls because Tick.state is the state before the step (core.py:393-404),
 * and with auto-reset the state after a finishing step is the next game's.
 *
 * Conventions: those of astro_step.h and astro_qnet.h.  The caller owns all
 * memory; the calls are stream-ordered and asynchronous on `stream`; the
 * library never allocates or synchronises; 0 on success, a negative code on a
 * bad argument (-1..-199) or a launch failure (-1000 - hipError_t), described
 * by astro_trace_last_error() for the calling thread.
 *
 * A library of its own: it shares the structs of astro_step.h with the others
 * and no symbol.
 */
#ifndef ASTRO_TRACE_H
#define ASTRO_TRACE_H

#include <stdint.h>

#include "astro_step.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ASTRO_TRACE_ABI_VERSION 1
#define ASTRO_TRACE_MAX_OUT 6   /* a Q-network's outputs (astro_qnet.h ASTRO_QNET_MAX_OUT) */

/* A ring of `ticks` slots for `m` chosen envs (device pointers).  Slot-major,
 * then ENV-major -- unlike the env arrays, which are ship- and planet-major --
 * so one env's record of a tick is contiguous and a slot is one block.  T is
 * the env state's element type, float or double as AstroState.state_f64 says. */
typedef struct AstroTrace {
    const int32_t *ids; /* [m] the chosen envs' indices; an id outside [0, n_env) records nothing */
    void *ships;        /* T [ticks][m][nships][4]  x, y, dx, dy */
    void *ships_b;      /* T [ticks][m][nships]     bearing */
    void *planets;      /* T [ticks][m][p_pad][4]   rows >= nplanets are written as zero */
    void *bullets;      /* T [ticks][m][b_cap][4]   rows >= nbullets are written as zero */
    int32_t *hdr;       /* [ticks][m][4]: tick, the env's hdr word 1 as it stands (nplanets | flags << 8 |
                           nbullets << 16), the current game's seed (stream[4 i + 3]), 0 */
    int8_t *control;    /* [ticks][m][nships] */
    float *q;           /* [ticks][m][nships][nout], or NULL with nout 0 */
    float *reward;      /* [ticks][m][nships] */
    uint8_t *done;      /* [ticks][m] */
    int32_t m;          /* >= 1 */
    int32_t ticks;      /* >= 1 */
    int32_t nout;       /* 0 .. ASTRO_TRACE_MAX_OUT */
    int32_t reserved;
} AstroTrace;

int astro_trace_abi_version(void);
const char *astro_trace_last_error(void);

/* Before the step: for every j < m with e = ids[j] in [0, n_env), slot `slot` of the ring receives
 * env e's ships, bearings, planets, bullets and header words, control[e] of the int8 [n_env][nships]
 * tensor the step will take and, when trace->q is set, q[e] of a float [n_env][nships][nout] tensor.
 * Live rows (planets below nplanets, bullets below nbullets, both clamped to p_pad / b_cap) are
 * copied bit for bit; dead rows are written as zero, so what a slot holds depends on the run alone,
 * not on what the ring held.  Envs that ids does not name are neither read nor written, and nothing
 * of the env state is written at all.
 *
 * Argument codes, in the order they are checked (all before the device is touched):
 *   -10 params NULL, -2 state NULL, -140 trace NULL, -11 nships, -13 p_pad, -15 b_cap, -141 m < 1,
 *   -142 ticks < 1, -143 nout outside 0..6, -144 slot outside [0, ticks), -3 n_env < 0,
 *   -146 trace->q set with nout 0 or NULL with nout > 0, -145 q given without trace->q or trace->q
 *   without q, -147 control NULL, (n_env == 0 returns 0,) -148 a trace array is NULL, -4 a state array
 *   (ships, ships_b, planets, bullets, hdr, stream) is NULL, -6 state_f64, -5 state alignment,
 *   -149 trace alignment, -150 q alignment. */
int astro_trace_state(const AstroParams *p, const AstroState *s, const AstroTrace *trace, int32_t slot,
                      const int8_t *control, const float *q, void *stream);

/* After the step: reward[e] (float [n_env][nships]) and done[e] (uint8 [n_env]) of the step's
 * outputs into the same slot, for the same envs.
 *
 * Argument codes, in the order they are checked:
 *   -140 trace NULL, -11 nships not 1 or 2, -141 m < 1, -142 ticks < 1, -144 slot outside [0, ticks),
 *   -3 n_env < 0, -151 reward or done NULL, (n_env == 0 returns 0,) -148 trace->ids, reward or done
 *   is NULL, -149 trace alignment, -152 reward alignment. */
int astro_trace_result(const AstroTrace *trace, int32_t slot, const float *reward, const uint8_t *done,
                       int32_t n_env, int32_t nships, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ASTRO_TRACE_H */
