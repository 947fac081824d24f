// libastro_fork.so: env state copied between slots on the device
// (include/astro_fork.h).
//
// fork    sixteen lanes per pair, four pairs per wave, sixteen per workgroup.
//         A group's lanes load the pair's two ids (every lane the same
//         address), check them, and then cover the pieces of the env, each
//         moved as 16-byte words so that no float instruction touches the
//         bits:
//           lane 0        the hdr row (16 B) and the stream row (16 B): one
//                         16-byte store each with GAME | STREAM, else the
//                         half (hdr) or the words (stream) that `what` owns
//           lanes < S     a ship's (x, y, dx, dy) and its bearing
//           lanes < p_pad a planet slot's (x, y, dx, dy)
//           all 16        the stream ring, 156 words of 16 bytes: nine whole
//                         trips and a tail of twelve lanes, every load
//                         issued before the first store;
//                         then the live bullet rows, nbullets * W words,
//                         in trips of 16 until the row is done -- any count
//                         up to b_cap
//         Ships and planets are strided by n_env on both sides (a gather and
//         a scatter: one element per 16 N bytes); the ring and the bullet row
//         are contiguous, so a group's trip is 256 contiguous bytes and a
//         wave's four such runs.  A whole-batch identity fork therefore reads
//         and writes every array in address order.
//
// No LDS, no atomics, no communication between lanes: a pair whose id is out
// of range, or that names one env of the same arrays twice, ends its sixteen
// lanes before they touch anything.  At the c3 shape a pair is about 2.9 KB
// with the stream and about 0.3 KB without.
#include "astro_common.h"
#include "astro_fork.h"
#include "astro_step.h"

namespace {

constexpr int BLOCK = 256;
constexpr int GROUP = 16;                 // lanes per pair: p_pad <= 16 planet slots, one lane each
constexpr int PAIRS = BLOCK / GROUP;      // pairs per workgroup
constexpr int RING16 = 624 / 4;           // an env's stream ring in 16-byte words
constexpr int RING_FULL = RING16 / GROUP;  // nine whole trips of a group ...
constexpr int RING_TAIL = RING16 % GROUP;  // ... and twelve words more

// sixteen bytes as the compiler's own vector: an array of these stays in registers (HIP's uint4 is a
// struct, and an array of it went to scratch)
typedef uint32_t word16 __attribute__((ext_vector_type(4)));

// W: 16-byte words per (x, y, dx, dy) element (1 float, 2 double)
template <int W>
__global__ __launch_bounds__(BLOCK) void fork_kernel(AstroState src, AstroState dst, const int32_t *__restrict__ src_ids,
                                                     const int32_t *__restrict__ dst_ids, int m, int what, int S,
                                                     int p_pad, int b_cap) {
    using B = std::conditional_t<W == 1, uint32_t, uint64_t>;   // a bearing's bits
    const int q = threadIdx.x & (GROUP - 1);
    const int64_t j = int64_t(blockIdx.x) * PAIRS + (threadIdx.x / GROUP);
    if (j >= m) return;
    const int se = src_ids ? src_ids[j] : int(j);
    const int de = dst_ids ? dst_ids[j] : int(j);
    if (se < 0 || se >= src.n_env || de < 0 || de >= dst.n_env) return;   // the pair is skipped whole
    if (se == de && src.hdr == dst.hdr) return;                          // an env onto itself
    const size_t ns = size_t(src.n_env), nd = size_t(dst.n_env), a = size_t(se), b = size_t(de);
    const bool game = (what & ASTRO_FORK_GAME) != 0, future = (what & ASTRO_FORK_STREAM) != 0;

    // every lane of the group reads the source's header: word 1 has the bullet count
    const word16 h = reinterpret_cast<const word16 *>(src.hdr)[a];
    if (q == 0) {
        const word16 c = reinterpret_cast<const word16 *>(src.stream)[a];
        uint32_t *dh = reinterpret_cast<uint32_t *>(dst.hdr) + 4 * b;
        uint32_t *dc = dst.stream + 4 * b;
        if (game && future) {
            *reinterpret_cast<word16 *>(dh) = h;
            *reinterpret_cast<word16 *>(dc) = c;
        } else if (game) {
            *reinterpret_cast<uint2 *>(dh) = make_uint2(h[0], h[1]);
            dc[3] = c[3];
        } else {
            *reinterpret_cast<uint2 *>(dh + 2) = make_uint2(h[2], h[3]);
            *reinterpret_cast<uint2 *>(dc) = make_uint2(c[0], c[1]);
            dc[2] = c[2];
        }
    }

    if (future) {
        const word16 *rs = reinterpret_cast<const word16 *>(src.stream_ring) + a * RING16;
        word16 *rd = reinterpret_cast<word16 *>(dst.stream_ring) + b * RING16;
        // (whole trips unconditionally and the tail in a value of its own, so the array stays in registers)
        word16 v[RING_FULL];
#pragma unroll
        for (int t = 0; t < RING_FULL; ++t) v[t] = rs[q + GROUP * t];
        word16 tail = {0u, 0u, 0u, 0u};
        if (q < RING_TAIL) tail = rs[q + GROUP * RING_FULL];
#pragma unroll
        for (int t = 0; t < RING_FULL; ++t) rd[q + GROUP * t] = v[t];
        if (q < RING_TAIL) rd[q + GROUP * RING_FULL] = tail;
    }
    if (!game) return;

    if (q < S) {
        const word16 *s = reinterpret_cast<const word16 *>(src.ships) + (size_t(q) * ns + a) * W;
        word16 *d = reinterpret_cast<word16 *>(dst.ships) + (size_t(q) * nd + b) * W;
#pragma unroll
        for (int w = 0; w < W; ++w) d[w] = s[w];
        static_cast<B *>(dst.ships_b)[size_t(q) * nd + b] = static_cast<const B *>(src.ships_b)[size_t(q) * ns + a];
    }
    if (q < p_pad) {
        const word16 *s = reinterpret_cast<const word16 *>(src.planets) + (size_t(q) * ns + a) * W;
        word16 *d = reinterpret_cast<word16 *>(dst.planets) + (size_t(q) * nd + b) * W;
#pragma unroll
        for (int w = 0; w < W; ++w) d[w] = s[w];
    }
    // the live rows [0, nbullets): nbullets <= b_cap rows of W words, inside both envs' rows
    const int nb = min(int((h[1] >> 16) & 0xffffu), b_cap);
    const word16 *s = reinterpret_cast<const word16 *>(src.bullets) + a * size_t(b_cap) * W;
    word16 *d = reinterpret_cast<word16 *>(dst.bullets) + b * size_t(b_cap) * W;
    for (int k = q; k < nb * W; k += GROUP) d[k] = s[k];
}

// -4 / -164: the arrays `what` needs
bool has_arrays(const AstroState *s, int32_t what) {
    if (!s->ships || !s->ships_b || !s->planets || !s->hdr || !s->stream) return false;
    if ((what & ASTRO_FORK_GAME) && !s->bullets) return false;
    if ((what & ASTRO_FORK_STREAM) && !s->stream_ring) return false;
    return true;
}

// -5 / -165 (a NULL array that `what` does not need is aligned)
bool state_aligned(const AstroState *s) {
    return aligned(s->ships, 16) && aligned(s->planets, 16) && aligned(s->bullets, 16) && aligned(s->hdr, 16) &&
           aligned(s->stream, 16) && aligned(s->stream_ring, 16) && aligned(s->ships_b, s->state_f64 ? 8 : 4);
}

}  // namespace

extern "C" {

int astro_fork_abi_version(void) { return ASTRO_FORK_ABI_VERSION; }

const char *astro_fork_last_error(void) { return g_err; }

int astro_fork(const AstroParams *p, const AstroState *src, const AstroState *dst, const int32_t *src_ids,
               const int32_t *dst_ids, int32_t m, int32_t what, void *stream) {
    if (!p) return fail(-10, "params is NULL");
    if (!src) return fail(-2, "src state is NULL");
    if (!dst) return fail(-160, "dst state is NULL");
    if (p->nships != 1 && p->nships != 2) return fail(-11, "nships must be 1 or 2, got %d", int(p->nships));
    if (p->p_pad < 1 || p->p_pad > 16) return fail(-13, "p_pad must be in [1, 16], got %d", int(p->p_pad));
    if (p->b_cap < 1 || p->b_cap > 65535) return fail(-15, "b_cap must be in [1, 65535], got %d", int(p->b_cap));
    if (m < 0) return fail(-161, "m must be >= 0, got %d", int(m));
    if (m == 0) return 0;
    if (what == 0 || (what & ~(ASTRO_FORK_GAME | ASTRO_FORK_STREAM)))
        return fail(-162, "what must be ASTRO_FORK_GAME, ASTRO_FORK_STREAM or both, got %d", int(what));
    if ((src->state_f64 != 0 && src->state_f64 != 1) || (dst->state_f64 != 0 && dst->state_f64 != 1))
        return fail(-6, "state_f64 must be 0 or 1, got %d and %d", int(src->state_f64), int(dst->state_f64));
    if (src->state_f64 != dst->state_f64) return fail(-163, "src and dst differ in state_f64");
    if (src->n_env < 0 || dst->n_env < 0) return fail(-3, "n_env < 0");
    if (src->n_env == 0 || dst->n_env == 0) return 0;
    if (!has_arrays(src, what)) return fail(-4, "an array of src that this fork needs is NULL");
    if (!has_arrays(dst, what)) return fail(-164, "an array of dst that this fork needs is NULL");
    if (!state_aligned(src))
        return fail(-5, "src arrays must be 16-byte aligned (ships_b: to its element)");
    if (!state_aligned(dst))
        return fail(-165, "dst arrays must be 16-byte aligned (ships_b: to its element)");
    if (!aligned(src_ids, 4) || !aligned(dst_ids, 4)) return fail(-166, "the id arrays must be 4-byte aligned");

    hipStream_t hs = static_cast<hipStream_t>(stream);
    const dim3 grid(blocks_for(m, PAIRS)), block(BLOCK);
    if (src->state_f64)
        hipLaunchKernelGGL(fork_kernel<2>, grid, block, 0, hs, *src, *dst, src_ids, dst_ids, int(m), int(what),
                           int(p->nships), int(p->p_pad), int(p->b_cap));
    else
        hipLaunchKernelGGL(fork_kernel<1>, grid, block, 0, hs, *src, *dst, src_ids, dst_ids, int(m), int(what),
                           int(p->nships), int(p->p_pad), int(p->b_cap));
    return launched("astro_fork");
}

}  // extern "C"
