// libastro_trace.so: the state, controls, Q values, reward and done of a few
// chosen envs, gathered into a ring on the device (include/astro_trace.h).
//
// state   one wave per chosen env.  The wave reads its env's header row once
//         (one 16-byte load, every lane the same address) and the game's seed,
//         then its lanes cover the env's (x, y, dx, dy) elements -- 16 bytes
//         as float, 32 as double, moved as one or two 16-byte words so that no
//         float instruction touches the bits: lanes 0 .. S-1 the ships (with
//         the bearing, the control and, over S * nout lanes, the Q values),
//         lanes 32 .. 32 + p_pad - 1 the planets, and all 64 lanes the bullet
//         row, in trips of 64.  The env arrays are strided by n_env for ships
//         and planets (a gather: one element per 16 N bytes) and contiguous
//         for the bullet row; every write is contiguous, env-major.  A dead
//         row -- a planet past nplanets, a bullet past nbullets -- is not
//         read: the lane stores zeros.  An id outside [0, n_env) ends its wave
//         before it touches anything.
//
// result  one lane per chosen env: S floats and a byte.
//
// No LDS, no atomics, no communication between waves; every branch that ends
// a wave is wave-uniform.  At 4,096 envs of the c3 shape a tick's record is
// about 2.5 MB: both kernels are bound by the launch, not by the bytes.
#include "astro_common.h"
#include "astro_step.h"
#include "astro_trace.h"

namespace {

constexpr int BLOCK = 256;            // four waves: four chosen envs per workgroup
constexpr int WAVES = BLOCK / 64;
constexpr int PLANET_LANE0 = 32;      // p_pad <= 16: lanes 32 .. 47

// One (x, y, dx, dy) element, W 16-byte words (W 1: float, 2: double), from src[a] to dst[b] in
// units of elements; a dead element is not read and stored as zeros.  (Plain uint4 values: a
// struct of them would be promoted to LDS.)
template <int W>
__device__ __forceinline__ void copy_elem(const void *src, size_t a, void *dst, size_t b, bool live) {
    const uint4 *s = static_cast<const uint4 *>(src) + a * W;
    uint4 *d = static_cast<uint4 *>(dst) + b * W;
    uint4 v0 = make_uint4(0, 0, 0, 0), v1 = v0;
    if (live) {
        v0 = s[0];
        if (W == 2) v1 = s[1];
    }
    d[0] = v0;
    if (W == 2) d[1] = v1;
}

template <int W, int S>
__global__ __launch_bounds__(BLOCK) void trace_state_kernel(AstroState st, AstroTrace tr, int p_pad, int b_cap, int slot,
                                                            const int8_t *__restrict__ control,
                                                            const float *__restrict__ q) {
    using B = std::conditional_t<W == 1, uint32_t, uint64_t>;   // a bearing's bits
    const int l = threadIdx.x & 63;
    const int j = int(blockIdx.x) * WAVES + (threadIdx.x >> 6);   // wave-uniform
    if (j >= tr.m) return;
    const int e = tr.ids[j];
    if (e < 0 || e >= st.n_env) return;                          // wave-uniform: a bad id records nothing
    const size_t n = size_t(st.n_env), i = size_t(e);
    const size_t rec = size_t(slot) * size_t(tr.m) + size_t(j);  // slot < ticks, j < m: inside the ring

    const int4 h = reinterpret_cast<const int4 *>(st.hdr)[i];
    const uint32_t seed = st.stream[4 * i + 3];
    const int np = min(h.y & 0xff, p_pad);
    const int nb = min((h.y >> 16) & 0xffff, b_cap);
    if (l == 0)
        reinterpret_cast<int4 *>(tr.hdr)[rec] = make_int4(int(uint32_t(h.x) & TICK_MASK), h.y, int(seed), 0);

    if (l < S) {
        copy_elem<W>(st.ships, size_t(l) * n + i, tr.ships, rec * S + l, true);
        static_cast<B *>(tr.ships_b)[rec * S + l] = static_cast<const B *>(st.ships_b)[size_t(l) * n + i];
        tr.control[rec * S + l] = control[i * S + l];
    }
    if (l < S * tr.nout) {   // (nout 0: no lane)
        const size_t row = size_t(S) * size_t(tr.nout);
        tr.q[rec * row + l] = q[i * row + l];
    }
    if (l >= PLANET_LANE0 && l < PLANET_LANE0 + p_pad) {
        const int k = l - PLANET_LANE0;
        copy_elem<W>(st.planets, size_t(k) * n + i, tr.planets, rec * size_t(p_pad) + k, k < np);
    }
    for (int k = l; k < b_cap; k += 64)
        copy_elem<W>(st.bullets, i * size_t(b_cap) + k, tr.bullets, rec * size_t(b_cap) + k, k < nb);
}

template <int S>
__global__ __launch_bounds__(BLOCK) void trace_result_kernel(AstroTrace tr, int slot, const float *__restrict__ reward,
                                                             const uint8_t *__restrict__ done, int n_env) {
    const int j = int(blockIdx.x) * BLOCK + threadIdx.x;
    if (j >= tr.m) return;
    const int e = tr.ids[j];
    if (e < 0 || e >= n_env) return;
    const size_t rec = size_t(slot) * size_t(tr.m) + size_t(j);
#pragma unroll
    for (int s = 0; s < S; ++s) tr.reward[rec * S + s] = reward[size_t(e) * S + s];
    tr.done[rec] = done[e];
}

// the ring's own scalars: -141 m, -142 ticks, (-143 nout,) -144 slot
int check_ring(const AstroTrace *t, int32_t slot, bool with_nout) {
    if (t->m < 1) return fail(-141, "trace.m must be >= 1, got %d", int(t->m));
    if (t->ticks < 1) return fail(-142, "trace.ticks must be >= 1, got %d", int(t->ticks));
    if (with_nout && (t->nout < 0 || t->nout > ASTRO_TRACE_MAX_OUT))
        return fail(-143, "trace.nout must be in [0, %d], got %d", ASTRO_TRACE_MAX_OUT, int(t->nout));
    if (slot < 0 || slot >= t->ticks) return fail(-144, "slot must be in [0, %d), got %d", int(t->ticks), int(slot));
    return 0;
}

}  // namespace

extern "C" {

int astro_trace_abi_version(void) { return ASTRO_TRACE_ABI_VERSION; }

const char *astro_trace_last_error(void) { return g_err; }

int astro_trace_state(const AstroParams *p, const AstroState *s, const AstroTrace *t, int32_t slot,
                      const int8_t *control, const float *q, void *stream) {
    if (!p) return fail(-10, "params is NULL");
    if (!s) return fail(-2, "state is NULL");
    if (!t) return fail(-140, "trace is NULL");
    if (p->nships != 1 && p->nships != 2) return fail(-11, "nships must be 1 or 2, got %d", int(p->nships));
    if (p->p_pad < 1 || p->p_pad > 16) return fail(-13, "p_pad must be in [1, 16], got %d", int(p->p_pad));
    if (p->b_cap < 1 || p->b_cap > 65535) return fail(-15, "b_cap must be in [1, 65535], got %d", int(p->b_cap));
    if (int rc = check_ring(t, slot, true)) return rc;
    if (s->n_env < 0) return fail(-3, "n_env < 0");
    if ((t->q != nullptr) != (t->nout > 0))
        return fail(-146, "trace.q must be set with nout > 0 and NULL with nout 0 (nout %d)", int(t->nout));
    if ((q != nullptr) != (t->q != nullptr))
        return fail(-145, q ? "q given but trace.q is NULL" : "trace.q is set but q is NULL");
    if (!control) return fail(-147, "control is NULL");
    if (s->n_env == 0) return 0;
    if (!t->ids || !t->ships || !t->ships_b || !t->planets || !t->bullets || !t->hdr || !t->control || !t->reward ||
        !t->done)
        return fail(-148, "a trace array is NULL");
    if (!s->ships || !s->ships_b || !s->planets || !s->bullets || !s->hdr || !s->stream)
        return fail(-4, "a state array (ships, ships_b, planets, bullets, hdr, stream) is NULL");
    if (s->state_f64 != 0 && s->state_f64 != 1) return fail(-6, "state_f64 must be 0 or 1, got %d", int(s->state_f64));
    const unsigned el = s->state_f64 ? 8 : 4;
    if (!aligned(s->ships, 16) || !aligned(s->planets, 16) || !aligned(s->bullets, 16) || !aligned(s->hdr, 16) ||
        !aligned(s->stream, 4) || !aligned(s->ships_b, el))
        return fail(-5, "state arrays must be 16-byte aligned (ships_b: to its element, stream: to 4 bytes)");
    if (!aligned(t->ships, 16) || !aligned(t->planets, 16) || !aligned(t->bullets, 16) || !aligned(t->hdr, 16) ||
        !aligned(t->ships_b, el) || !aligned(t->ids, 4) || !aligned(t->reward, 4) || !aligned(t->q, 4))
        return fail(-149, "trace arrays must be 16-byte aligned (ships_b: to its element; ids, q, reward: to 4 bytes)");
    if (!aligned(q, 4)) return fail(-150, "q must be 4-byte aligned");

    hipStream_t hs = static_cast<hipStream_t>(stream);
    const dim3 grid(blocks_for(t->m, WAVES)), block(BLOCK);
    with_nships(p->nships, [&](auto S) {
        if (s->state_f64)
            hipLaunchKernelGGL((trace_state_kernel<2, S()>), grid, block, 0, hs, *s, *t, int(p->p_pad), int(p->b_cap),
                               int(slot), control, q);
        else
            hipLaunchKernelGGL((trace_state_kernel<1, S()>), grid, block, 0, hs, *s, *t, int(p->p_pad), int(p->b_cap),
                               int(slot), control, q);
    });
    return launched("astro_trace_state");
}

int astro_trace_result(const AstroTrace *t, int32_t slot, const float *reward, const uint8_t *done, int32_t n_env,
                       int32_t nships, void *stream) {
    if (!t) return fail(-140, "trace is NULL");
    if (nships != 1 && nships != 2) return fail(-11, "nships must be 1 or 2, got %d", int(nships));
    if (int rc = check_ring(t, slot, false)) return rc;
    if (n_env < 0) return fail(-3, "n_env < 0");
    if (!reward || !done) return fail(-151, "reward or done is NULL");
    if (n_env == 0) return 0;
    if (!t->ids || !t->reward || !t->done) return fail(-148, "a trace array (ids, reward, done) is NULL");
    if (!aligned(t->ids, 4) || !aligned(t->reward, 4))
        return fail(-149, "trace.ids and trace.reward must be 4-byte aligned");
    if (!aligned(reward, 4)) return fail(-152, "reward must be 4-byte aligned");

    hipStream_t hs = static_cast<hipStream_t>(stream);
    const dim3 grid(blocks_for(t->m, BLOCK)), block(BLOCK);
    with_nships(nships, [&](auto S) {
        hipLaunchKernelGGL(trace_result_kernel<S()>, grid, block, 0, hs, *t, int(slot), reward, done, int(n_env));
    });
    return launched("astro_trace_result");
}

}  // extern "C"
