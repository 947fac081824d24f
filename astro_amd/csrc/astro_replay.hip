// libastro_replay.so: the experience replay of rl.QBotTrainer (rl.py:231-332) on
// a time-major device ring (include/astro_replay.h).
//
// push     one lane per env: the head row's bookkeeping, and on the lanes whose
//          window closes a loop over the window's ticks (at most n_steps) that
//          writes the n-step reward, discount and next row.  For one tick the
//          stores of neighbouring envs are neighbours in memory.
//
// sample   a radix select over v = class << 32 | bits(key), 34 bits, then an
//          ordered compaction:
//            init    zero the three histograms
//            keys    every id's class and key once, into the workspace, and the
//                    histogram of v's top 12 bits (LDS counters, integer atomics)
//            select  one workgroup scans the histogram for the bin that holds
//                    the n-th smallest and keeps the rank inside it
//            hist    the next 11 bits of the ids that match the prefix; select;
//                    the last 11 bits; select: the threshold T and the number r
//                    of ids equal to T to take
//            count   per tile of 1,024 ids (one wave) the ids below T and equal to T
//            scan    one workgroup: exclusive sums over the tiles
//            compact per tile again: id i is taken when v < T, or v == T and
//                    fewer than r equal ids precede it; its place is (ids below
//                    T before i) + min(equal ids before i, r), so the output is
//                    in ascending id order and no atomic decides an order.
//          With n >= eligible the first select marks the call done: T = 2^34
//          takes every eligible id and the two histogram passes return at once.
//
// gather   one wave per sample, lanes along the [rows][nf] image: column 0 is
//          read per element, live rows are copied (ship 1: the two ships'
//          columns exchanged), of padding rows only column 0 is stored.
//
// update   a scatter of float32.
#include <algorithm>
#include <cmath>

#include "astro_common.h"
#include "astro_replay.h"

namespace {

constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / 64;
constexpr int ITEMS = 16;                  // ids per lane and tile
constexpr int TILE = 64 * ITEMS;           // ids per wave in count / compact
constexpr int BINS = 4096;                 // 12 bits first (2 of class, 10 of key), then 11 and 11
constexpr int D1_SHIFT = 22, D2_SHIFT = 11, D_MASK = 2047;
constexpr int SCAN_BLOCK = 1024;
constexpr int MAX_GRID = 2048;
constexpr uint64_t V_ALL = 1ull << 34;     // above every v: take every eligible id
constexpr uint64_t V_NONE = 1ull << 35;    // the v of an id that is not a candidate

// the selection's state, at the start of the workspace
struct Sel {
    uint64_t threshold;   // T
    uint64_t prefix;      // the digits decided so far
    int32_t remaining;    // rank of the wanted element among those that match the prefix, from 1
    int32_t take_eq;      // r
    int32_t done;         // every pass after this one has nothing to do
    int32_t pad;
};

struct Layout {
    size_t hist, tiles, keys, cls, total;
    int ntiles;
};

__host__ __device__ inline size_t align16(size_t x) { return (x + 15) & ~size_t(15); }

Layout layout_of(int64_t m) {
    Layout l;
    l.ntiles = int((m + TILE - 1) / TILE);
    l.hist = align16(sizeof(Sel));
    l.tiles = l.hist + size_t(3) * BINS * sizeof(uint32_t);
    l.keys = align16(l.tiles + size_t(l.ntiles) * sizeof(uint64_t));
    l.cls = align16(l.keys + size_t(m) * sizeof(uint32_t));
    l.total = align16(l.cls + size_t(m));
    return l;
}

// exclusive sum of x over the workgroup's SCAN_BLOCK threads in thread order; *total: the sum
__device__ uint64_t block_scan(uint64_t x, uint64_t *s, uint64_t *total) {
    const int tid = threadIdx.x;
    s[tid] = x;
    __syncthreads();
    for (int d = 1; d < SCAN_BLOCK; d <<= 1) {
        const uint64_t y = tid >= d ? s[tid - d] : 0;
        __syncthreads();
        s[tid] += y;
        __syncthreads();
    }
    const uint64_t incl = s[tid];
    *total = s[SCAN_BLOCK - 1];
    __syncthreads();
    return incl - x;
}

// ---------------------------------------------------------------------------
// push

template <int S>
__global__ __launch_bounds__(BLOCK) void replay_push_kernel(AstroReplay rb, int64_t t, const int8_t *__restrict__ control,
                                                            const float *__restrict__ reward,
                                                            const uint8_t *__restrict__ done) {
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    const int N = rb.n_env;
    if (e >= N) return;
    const int head = int(t % rb.ticks);
    const size_t he = size_t(head) * N + e;
    float rnow[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        rnow[s] = reward[size_t(e) * S + s];
        rb.action[he * S + s] = control[size_t(e) * S + s];
        rb.reward[he * S + s] = 0.0f;
        rb.loss[he * S + s] = INFINITY;
    }
    rb.discount[he] = 0.0f;
    rb.next[he] = ASTRO_REPLAY_NEXT_PENDING;
    int64_t w = rb.wstart[e];
    if (w < 0 || w > t || w < t - rb.n_steps + 1) w = t;
    const int L = int(t - w) + 1;
    const bool d = done[e] != 0;
    if (!d && L < rb.n_steps) return;
    const int nx = d ? ASTRO_REPLAY_NEXT_TERMINAL : int((t + 1) % rb.ticks);
    int row = int(w % rb.ticks);
    for (int j = 0; j < L; ++j) {
        const double g = rb.gpow[L - 1 - j];
        const size_t re = size_t(row) * N + e;
#pragma unroll
        for (int s = 0; s < S; ++s) rb.reward[re * S + s] = float(double(rnow[s]) * g);
        rb.discount[re] = float(rb.gamma * g);
        rb.next[re] = nx;
        if (++row == rb.ticks) row = 0;
    }
    rb.wstart[e] = t + 1;
}

// ---------------------------------------------------------------------------
// sample

__global__ __launch_bounds__(BLOCK) void replay_init_kernel(uint32_t *hist) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < 3 * BINS) hist[i] = 0;
}

template <int S>
__global__ __launch_bounds__(BLOCK) void replay_keys_kernel(const float *__restrict__ loss, const int32_t *__restrict__ next,
                                                            int N, int m, int written, int head, uint64_t seed,
                                                            uint64_t drawmix, uint32_t *__restrict__ keys,
                                                            uint8_t *__restrict__ cls, uint32_t *__restrict__ hist) {
    __shared__ uint32_t h[BINS];
    for (int b = threadIdx.x; b < BINS; b += BLOCK) h[b] = 0;
    __syncthreads();
    // (row, j) of id = row * per_row + j, advanced by the grid's stride without a division per id
    const int per_row = N * S;
    const int64_t stride = int64_t(gridDim.x) * BLOCK;
    const int row_step = int(stride / per_row), j_step = int(stride - int64_t(row_step) * per_row);
    const int64_t first = int64_t(blockIdx.x) * BLOCK + threadIdx.x;
    int row = int(first / per_row), j = int(first - int64_t(row) * per_row);
    for (int64_t i = first; i < m; i += stride, row += row_step, j += j_step) {
        if (j >= per_row) {
            j -= per_row;
            ++row;
        }
        const int id = int(i);
        const int env = j / S;
        uint32_t c = 3, key = 0;
        if (row < written && row != head) {
            const int nx = next[size_t(row) * N + env];
            if (nx != ASTRO_REPLAY_NEXT_PENDING && nx != head) {
                const float l = loss[id];
                const uint64_t z = random_word(uint64_t(id), drawmix + seed);
                const double u = (double(z >> 11) + 0.5) * 0x1p-53;
                const double E = -log(u);
                if (l == INFINITY) {
                    c = 0;
                    key = __float_as_uint(float(E));
                } else if (l > 0.0f && l < INFINITY) {
                    c = 1;
                    key = __float_as_uint(float(E / double(l)));
                } else {
                    c = 2;
                }
                key &= 0x7FFFFFFFu;   // (-log(1.0) is -0.0)
                atomicAdd(&h[(c << 10) | (key >> D1_SHIFT)], 1u);
            }
        }
        keys[id] = key;
        cls[id] = uint8_t(c);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < BINS; b += BLOCK)
        if (h[b]) atomicAdd(&hist[b], h[b]);
}

__device__ __forceinline__ uint64_t value_of(const uint32_t *keys, const uint8_t *cls, int64_t id, int m) {
    if (id >= m) return V_NONE;
    const uint32_t c = cls[id];
    return c > 2 ? V_NONE : (uint64_t(c) << 32) | keys[id];
}

// PASS 1: bits 21..11 of the ids whose bits 33..22 are the prefix; PASS 2: bits 10..0 under a 23-bit prefix
template <int PASS>
__global__ __launch_bounds__(BLOCK) void replay_hist_kernel(const Sel *__restrict__ sel, const uint32_t *__restrict__ keys,
                                                            const uint8_t *__restrict__ cls, int m,
                                                            uint32_t *__restrict__ hist) {
    if (sel->done) return;
    __shared__ uint32_t h[D_MASK + 1];
    for (int b = threadIdx.x; b <= D_MASK; b += BLOCK) h[b] = 0;
    __syncthreads();
    const uint64_t prefix = sel->prefix;
    constexpr int SHIFT = PASS == 1 ? D2_SHIFT : 0;
    for (int64_t i = int64_t(blockIdx.x) * BLOCK + threadIdx.x; i < m; i += int64_t(gridDim.x) * BLOCK) {
        const uint64_t v = value_of(keys, cls, i, m);
        if (v != V_NONE && (v >> (SHIFT + 11)) == prefix) atomicAdd(&h[(v >> SHIFT) & D_MASK], 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b <= D_MASK; b += BLOCK)
        if (h[b]) atomicAdd(&hist[b], h[b]);
}

// one workgroup: the bin of `hist` that holds the wanted rank
template <int PASS>
__global__ __launch_bounds__(SCAN_BLOCK) void replay_select_kernel(Sel *sel, const uint32_t *__restrict__ hist, int n,
                                                                   int32_t *count) {
    __shared__ uint64_t s[SCAN_BLOCK];
    if (PASS > 0 && sel->done) return;
    constexpr int NB = PASS == 0 ? BINS : D_MASK + 1;
    constexpr int PER = NB / SCAN_BLOCK;
    const int tid = threadIdx.x;
    const int64_t r0 = PASS == 0 ? 0 : sel->remaining;
    const uint64_t prefix0 = PASS == 0 ? 0 : sel->prefix;
    uint32_t hv[PER];
    uint64_t sum = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        hv[i] = hist[tid * PER + i];
        sum += hv[i];
    }
    uint64_t total;
    int64_t run = int64_t(block_scan(sum, s, &total));
    int64_t r = r0;
    if (PASS == 0) {
        const int64_t eligible = int64_t(total);
        const int64_t take = n < eligible ? n : eligible;
        if (take == eligible || take == 0) {   // everything, or nothing
            if (tid == 0) {
                *count = int32_t(take);
                sel->threshold = take == 0 ? 0 : V_ALL;
                sel->prefix = 0;
                sel->remaining = 0;
                sel->take_eq = 0;
                sel->done = 1;
                sel->pad = 0;
            }
            return;
        }
        if (tid == 0) *count = int32_t(take);
        r = take;
    }
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        if (run < r && r <= run + int64_t(hv[i])) {
            const uint64_t prefix = (prefix0 << (PASS == 0 ? 0 : 11)) | uint64_t(tid * PER + i);
            sel->prefix = prefix;
            sel->remaining = int32_t(r - run);
            sel->take_eq = int32_t(r - run);
            sel->threshold = prefix;   // the whole value after the last pass
            sel->done = PASS == 2 ? 1 : 0;
            sel->pad = 0;
        }
        run += int64_t(hv[i]);
    }
}

// per tile: ids below T in the low word, ids equal to T in the high word
__global__ __launch_bounds__(BLOCK) void replay_count_kernel(const Sel *__restrict__ sel, const uint32_t *__restrict__ keys,
                                                             const uint8_t *__restrict__ cls, int m, int ntiles,
                                                             uint64_t *__restrict__ tiles) {
    const int lane = threadIdx.x & 63;
    const int tile = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (tile >= ntiles) return;
    const uint64_t T = sel->threshold;
    uint32_t lt = 0, eq = 0;
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const uint64_t v = value_of(keys, cls, int64_t(tile) * TILE + it * 64 + lane, m);
        lt += __popcll(__ballot(v < T));
        eq += __popcll(__ballot(v == T));
    }
    if (lane == 0) tiles[tile] = uint64_t(lt) | (uint64_t(eq) << 32);
}

// one workgroup: the tiles' counts become the counts before each tile, in place
__global__ __launch_bounds__(SCAN_BLOCK) void replay_scan_kernel(uint64_t *tiles, int ntiles) {
    __shared__ uint64_t s[SCAN_BLOCK];
    const int per = (ntiles + SCAN_BLOCK - 1) / SCAN_BLOCK;
    const int a = min(ntiles, int(threadIdx.x) * per), b = min(ntiles, a + per);
    uint64_t sum = 0, c[8];
    int i = a;
    for (; i + 8 <= b; i += 8) {      // eight loads in flight: one workgroup, so latency is all there is
#pragma unroll
        for (int k = 0; k < 8; ++k) c[k] = tiles[i + k];
#pragma unroll
        for (int k = 0; k < 8; ++k) sum += c[k];
    }
    for (; i < b; ++i) sum += tiles[i];
    uint64_t total;
    uint64_t run = block_scan(sum, s, &total);
    for (i = a; i + 8 <= b; i += 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) c[k] = tiles[i + k];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            tiles[i + k] = run;
            run += c[k];
        }
    }
    for (; i < b; ++i) {
        const uint64_t ci = tiles[i];
        tiles[i] = run;
        run += ci;
    }
}

__global__ __launch_bounds__(BLOCK) void replay_compact_kernel(const Sel *__restrict__ sel, const uint32_t *__restrict__ keys,
                                                               const uint8_t *__restrict__ cls, int m, int ntiles,
                                                               const uint64_t *__restrict__ tiles, int n,
                                                               int32_t *__restrict__ ids) {
    const int lane = threadIdx.x & 63;
    const int tile = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (tile >= ntiles) return;
    const uint64_t T = sel->threshold;
    const int64_t r = sel->take_eq;
    const uint64_t before = tiles[tile];
    int64_t lt = int64_t(before & 0xFFFFFFFFu), eq = int64_t(before >> 32);
    const uint64_t below = (1ull << lane) - 1;
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const int64_t id = int64_t(tile) * TILE + it * 64 + lane;
        const uint64_t v = value_of(keys, cls, id, m);
        const uint64_t mlt = __ballot(v < T), meq = __ballot(v == T);
        const int64_t lt_b = lt + __popcll(mlt & below), eq_b = eq + __popcll(meq & below);
        const bool take = v < T || (v == T && eq_b < r);
        const int64_t pos = lt_b + (eq_b < r ? eq_b : r);
        if (take && pos >= 0 && pos < n) ids[pos] = int32_t(id);
        lt += __popcll(mlt);
        eq += __popcll(meq);
    }
}

// ---------------------------------------------------------------------------
// gather, update

// the column of ship 0's view that column c of ship `ship`'s view shows (qnet.swap_ego)
template <int S>
__device__ __forceinline__ int source_column(int c, int ship) {
    if (S == 2 && ship == 1 && c >= 1 && c < 11) return c < 6 ? c + 5 : c - 5;
    return c;
}

template <int S>
__global__ __launch_bounds__(BLOCK) void replay_gather_kernel(AstroReplay rb, const int32_t *__restrict__ ids, int n,
                                                              float *__restrict__ features, int8_t *__restrict__ action,
                                                              float *__restrict__ reward, float *__restrict__ discount,
                                                              float *__restrict__ next_features,
                                                              uint8_t *__restrict__ terminal) {
    constexpr int NF = 5 + 5 * S;
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= n) return;
    const int N = rb.n_env, rows = rb.rows, elems = rows * NF;
    const int64_t m = int64_t(rb.ticks) * N * S;
    const int id = ids[i];
    const bool valid = id >= 0 && id < m;
    int ship = 0, nx = ASTRO_REPLAY_NEXT_TERMINAL;
    size_t re = 0;
    if (valid) {
        re = size_t(id / S);
        ship = id - int(re) * S;
        nx = rb.next[re];
    }
    if (nx >= rb.ticks) nx = ASTRO_REPLAY_NEXT_PENDING;   // (never stored: a row the ring does not have)
    if (lane == 0) {
        action[i] = valid ? rb.action[id] : int8_t(-1);
        reward[i] = valid ? rb.reward[id] : 0.0f;
        discount[i] = valid ? rb.discount[re] : 0.0f;
        terminal[i] = (!valid || nx == ASTRO_REPLAY_NEXT_TERMINAL) ? 1 : 0;
    }
    float *out = features + size_t(i) * elems;
    float *nout = next_features + size_t(i) * elems;
    const float *src = valid ? rb.features + re * elems : nullptr;
    const int env = valid ? int(re % size_t(N)) : 0;
    const float *nsrc = nx >= 0 ? rb.features + (size_t(nx) * N + env) * elems : nullptr;
    for (int e = lane; e < elems; e += 64) {
        const int row = e / NF, c = e - row * NF;
        const int sc = source_column<S>(c, ship);
        if (src) {
            const float type = src[row * NF];
            if (c == 0 || !(type < 0.0f)) out[e] = src[row * NF + sc];
        } else if (c == 0) {
            out[e] = -1.0f;
        }
        if (nsrc) {
            const float type = nsrc[row * NF];
            if (c == 0 || !(type < 0.0f)) nout[e] = nsrc[row * NF + sc];
        } else if (c == 0) {
            nout[e] = -1.0f;
        }
    }
}

__global__ __launch_bounds__(BLOCK) void replay_update_kernel(float *__restrict__ ring_loss, int64_t m,
                                                              const int32_t *__restrict__ ids,
                                                              const float *__restrict__ loss, int n) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int id = ids[i];
    if (id >= 0 && id < m) ring_loss[id] = loss[i];
}

// ---------------------------------------------------------------------------
// host side

int check_scalars(const AstroReplay *rb) {
    if (!rb) return fail(-100, "rb is NULL");
    if (rb->nships != 1 && rb->nships != 2) return fail(-101, "rb.nships must be 1 or 2, got %d", int(rb->nships));
    if (rb->n_env < 1) return fail(-102, "rb.n_env must be >= 1, got %d", int(rb->n_env));
    if (rb->rows < 1 || rb->rows > ASTRO_REPLAY_MAX_ROWS)
        return fail(-103, "rb.rows must be in [1, %d], got %d", ASTRO_REPLAY_MAX_ROWS, int(rb->rows));
    if (rb->n_steps < 1 || rb->n_steps > ASTRO_REPLAY_MAX_STEPS)
        return fail(-104, "rb.n_steps must be in [1, %d], got %d", ASTRO_REPLAY_MAX_STEPS, int(rb->n_steps));
    if (int64_t(rb->ticks) < int64_t(rb->n_steps) + 2)
        return fail(-105, "rb.ticks must be >= n_steps + 2 = %d, got %d", int(rb->n_steps) + 2, int(rb->ticks));
    if (int64_t(rb->ticks) * rb->n_env * rb->nships > INT32_MAX)
        return fail(-106, "ticks * n_env * nships = %lld ids do not fit an int32",
                    (long long)(int64_t(rb->ticks) * rb->n_env * rb->nships));
    if (!std::isfinite(rb->gamma)) return fail(-107, "rb.gamma is not finite");
    return 0;
}

int64_t ids_of(const AstroReplay &rb) { return int64_t(rb.ticks) * rb.n_env * rb.nships; }

}  // namespace

extern "C" {

int astro_replay_abi_version(void) { return ASTRO_REPLAY_ABI_VERSION; }

const char *astro_replay_last_error(void) { return g_err; }

int astro_replay_push(const AstroReplay *rb, int64_t t, const int8_t *control, const float *reward,
                      const uint8_t *done, void *stream) {
    if (int rc = check_scalars(rb)) return rc;
    if (!rb->action || !rb->reward || !rb->discount || !rb->next || !rb->loss || !rb->wstart || !rb->gpow)
        return fail(-108, "rb.action, reward, discount, next, loss, wstart and gpow must not be NULL");
    if (!aligned(rb->reward, 4) || !aligned(rb->discount, 4) || !aligned(rb->next, 4) || !aligned(rb->loss, 4) ||
        !aligned(rb->wstart, 8) || !aligned(rb->gpow, 8))
        return fail(-109, "an array of rb is not aligned to its element size");
    if (t < 0) return fail(-110, "t < 0");
    if (!control || !reward || !done) return fail(-112, "control, reward or done is NULL");
    if (!aligned(reward, 4)) return fail(-119, "reward must be 4-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(blocks_for(rb->n_env, BLOCK)), block(BLOCK);
    with_nships(rb->nships, [&](auto S) {
        hipLaunchKernelGGL(replay_push_kernel<S()>, grid, block, 0, st, *rb, t, control, reward, done);
    });
    return launched("astro_replay_push");
}

size_t astro_replay_sample_workspace_bytes(const AstroReplay *rb) {
    if (!rb || rb->nships < 1 || rb->nships > 2 || rb->n_env < 1 || rb->ticks < 1 || ids_of(*rb) > INT32_MAX) return 0;
    return layout_of(ids_of(*rb)).total;
}

int astro_replay_sample(const AstroReplay *rb, int64_t t, int32_t n, uint64_t seed, uint64_t draw, int32_t *ids,
                        int32_t *count, void *workspace, size_t workspace_bytes, void *stream) {
    if (int rc = check_scalars(rb)) return rc;
    if (!rb->next || !rb->loss) return fail(-108, "rb.next and rb.loss must not be NULL");
    if (!aligned(rb->next, 4) || !aligned(rb->loss, 4)) return fail(-109, "rb.next and rb.loss must be 4-byte aligned");
    if (t < 0) return fail(-110, "t < 0");
    if (n < 0) return fail(-111, "n < 0");
    if (!ids && n > 0) return fail(-113, "ids is NULL");
    if (!count) return fail(-114, "count is NULL");
    const int64_t m64 = ids_of(*rb);
    const Layout l = layout_of(m64);
    if (!workspace || workspace_bytes < l.total)
        return fail(-118, "workspace of %zu bytes, astro_replay_sample_workspace_bytes is %zu",
                    workspace ? workspace_bytes : size_t(0), l.total);
    if (!aligned(ids, 4) || !aligned(count, 4)) return fail(-119, "ids and count must be 4-byte aligned");
    if (!aligned(workspace, 16)) return fail(-119, "workspace must be 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int m = int(m64);
    char *ws = static_cast<char *>(workspace);
    Sel *sel = reinterpret_cast<Sel *>(ws);
    uint32_t *hist = reinterpret_cast<uint32_t *>(ws + l.hist);
    uint64_t *tiles = reinterpret_cast<uint64_t *>(ws + l.tiles);
    uint32_t *keys = reinterpret_cast<uint32_t *>(ws + l.keys);
    uint8_t *cls = reinterpret_cast<uint8_t *>(ws + l.cls);
    const int written = int(t < rb->ticks ? t : rb->ticks), head = int(t % rb->ticks);
    const uint64_t drawmix = draw_mix(draw, 0);   // (the kernel adds the seed)
    const dim3 block(BLOCK), wide(std::min(blocks_for(m, BLOCK), unsigned(MAX_GRID)));
    const dim3 per_tile(blocks_for(l.ntiles, WAVES));

    hipLaunchKernelGGL(replay_init_kernel, dim3(blocks_for(3 * BINS, BLOCK)), block, 0, st, hist);
    with_nships(rb->nships, [&](auto S) {
        hipLaunchKernelGGL(replay_keys_kernel<S()>, wide, block, 0, st, rb->loss, rb->next, int(rb->n_env), m, written, head,
                           seed, drawmix, keys, cls, hist);
    });
    hipLaunchKernelGGL(replay_select_kernel<0>, dim3(1), dim3(SCAN_BLOCK), 0, st, sel, hist, int(n), count);
    hipLaunchKernelGGL(replay_hist_kernel<1>, wide, block, 0, st, sel, keys, cls, m, hist + BINS);
    hipLaunchKernelGGL(replay_select_kernel<1>, dim3(1), dim3(SCAN_BLOCK), 0, st, sel, hist + BINS, int(n), count);
    hipLaunchKernelGGL(replay_hist_kernel<2>, wide, block, 0, st, sel, keys, cls, m, hist + 2 * BINS);
    hipLaunchKernelGGL(replay_select_kernel<2>, dim3(1), dim3(SCAN_BLOCK), 0, st, sel, hist + 2 * BINS, int(n), count);
    hipLaunchKernelGGL(replay_count_kernel, per_tile, block, 0, st, sel, keys, cls, m, l.ntiles, tiles);
    hipLaunchKernelGGL(replay_scan_kernel, dim3(1), dim3(SCAN_BLOCK), 0, st, tiles, l.ntiles);
    hipLaunchKernelGGL(replay_compact_kernel, per_tile, block, 0, st, sel, keys, cls, m, l.ntiles, tiles, int(n), ids);
    return launched("astro_replay_sample");
}

int astro_replay_gather(const AstroReplay *rb, const int32_t *ids, int32_t n, float *features, int8_t *action,
                        float *reward, float *discount, float *next_features, uint8_t *terminal, void *stream) {
    if (int rc = check_scalars(rb)) return rc;
    if (n < 0) return fail(-111, "n < 0");
    if (n == 0) return 0;
    if (!rb->features || !rb->action || !rb->reward || !rb->discount || !rb->next)
        return fail(-108, "rb.features, action, reward, discount and next must not be NULL");
    if (!aligned(rb->features, 4) || !aligned(rb->reward, 4) || !aligned(rb->discount, 4) || !aligned(rb->next, 4))
        return fail(-109, "an array of rb is not 4-byte aligned");
    if (!ids) return fail(-113, "ids is NULL");
    if (!features || !action || !reward || !discount || !next_features || !terminal)
        return fail(-115, "an output array is NULL");
    if (!aligned(ids, 4) || !aligned(features, 4) || !aligned(reward, 4) || !aligned(discount, 4) ||
        !aligned(next_features, 4))
        return fail(-119, "ids, features, reward, discount and next_features must be 4-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(blocks_for(n, WAVES)), block(BLOCK);
    with_nships(rb->nships, [&](auto S) {
        hipLaunchKernelGGL(replay_gather_kernel<S()>, grid, block, 0, st, *rb, ids, int(n), features, action, reward,
                           discount, next_features, terminal);
    });
    return launched("astro_replay_gather");
}

int astro_replay_update(const AstroReplay *rb, const int32_t *ids, const float *loss, int32_t n, void *stream) {
    if (int rc = check_scalars(rb)) return rc;
    if (n < 0) return fail(-111, "n < 0");
    if (n == 0) return 0;
    if (!rb->loss) return fail(-108, "rb.loss must not be NULL");
    if (!aligned(rb->loss, 4)) return fail(-109, "rb.loss is not 4-byte aligned");
    if (!ids) return fail(-113, "ids is NULL");
    if (!loss) return fail(-115, "loss is NULL");
    if (!aligned(ids, 4) || !aligned(loss, 4)) return fail(-119, "ids and loss must be 4-byte aligned");
    hipLaunchKernelGGL(replay_update_kernel, dim3(blocks_for(n, BLOCK)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream),
                       rb->loss, ids_of(*rb), ids, loss, int(n));
    return launched("astro_replay_update");
}

}  // extern "C"
