// libastro_qpool.so: astro_qvalues (csrc/astro_qnet.hip) with a pool of
// networks, each playing one ship of a block of envs (include/astro_qpool.h).
//
// Layout.  astro_qvalues_ships (csrc/astro_qduel.hip) is ship-major: a
// workgroup stages ONE network's weights and walks chunks of 32 consecutive
// envs of one ship.  Here the unit is a SPAN -- ship s of the envs [lo, hi),
// played by network k -- and the rest is that kernel: a workgroup stages the
// weights of a span's network and serves chunks of that span; a chunk is 32
// consecutive envs counted from lo (not aligned to 32), the last one of a span
// partial, so astro_qduel_kernel's `i < N` is `i < hi` here.  A (ship, env)
// outside every span with a network belongs to no chunk: nothing of it is read
// or written.  The three phases A (features, counts, prefix sum, the ship part
// of f0), B (object rows as MFMA tiles, max per segment) and C (the head, tanh,
// argmax, exploration, stores) are astro_qduel_kernel's line for line.
//
// Who serves what is decided on the host and reaches the kernel by value (the
// active spans, at most 1 KiB, and 32 weight pointers fit the kernarg segment):
// the spans with a network and at least one env, sorted by network, and either
//   * own workgroups: span k has the workgroups first[k] .. first[k + 1] - 1,
//     at least one, in proportion to its chunks (the cap allowing), or
//   * shared workgroups (fewer workgroups than active spans, e.g. max_blocks =
//     1): workgroup g serves the spans [g nact / G, (g + 1) nact / G) one after
//     the other and restages the weights when the network changes.
// Every loop bound and every branch around a __syncthreads() depends on
// blockIdx and the kernel arguments only, so it is workgroup-uniform; there is
// no communication between workgroups, no spin wait and no atomic.
//
// Bit identity with astro_qvalues: astro_qduel.hip's argument.  Every value a
// column of a tile holds depends on that column's own inputs only, each row's
// chain of operations is astro_qvalues' (the same fmaf order for the ship part
// of f0, the same MFMA sequence and k order, the same softsign, the same
// tanhf), and the pool takes a segment's rows in the same order.  Which other
// segments share a tile -- here: where a chunk begins -- changes nothing.
//
// The device helpers that the Q-network sources need and astro_common.h does
// not have (Store, softsign, layer, Explore, WaveLds) are restated here, so
// the other libraries are what they were.
#include <algorithm>

#include "astro_common.h"
#include "astro_qpool.h"

namespace {

constexpr int NH = ASTRO_QNET_HIDDEN;
constexpr int QN_WAVES = 4;
constexpr int QN_BLOCK = 64 * QN_WAVES;
constexpr int SEGS = 32;          // envs per chunk = columns of the head's tile
constexpr int LD = NH + 1;        // LDS row stride of a [32][32] float image (bank-conflict-free columns)
constexpr int MAX_BLOCKS = 512;   // two workgroups per CU on 256 CUs
constexpr int MAX_NETS = ASTRO_QPOOL_MAX_NETS;
constexpr int MAX_SPANS = ASTRO_QPOOL_MAX_SPANS;

template <typename T> struct Store;
template <> struct Store<float> { using V = float4; };
template <> struct Store<double> { using V = double4; };

// a / (1 + |a|): the denominator is in [1, inf), so v_rcp_f32 (1 ulp) is safe
__device__ __forceinline__ float softsign(float a) { return a * __builtin_amdgcn_rcpf(1.0f + fabsf(a)); }

// acc += W x over the 32 inputs held as x's 16 registers (w: the lane's permuted weight columns)
__device__ __forceinline__ f32x16 layer(const float (&w)[16], const f32x16 &x, f32x16 acc) {
#pragma unroll
    for (int j = 0; j < 16; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[j], x[j], acc, 0, 0, 0);
    return acc;
}

struct Explore {
    int32_t on;
    uint64_t seed;
    int64_t tick0;
    int64_t env_offset;
    uint64_t threshold;   // uint64(epsilon * 2^32)
};

// The launch's work, by value: the active spans (a network, at least one env;
// checked on the host: 0 <= ship < nships, 0 <= lo < hi <= n_env, net a used
// network) and how the workgroups share them
struct Work {
    const float *w[MAX_NETS];
    int32_t ship[MAX_SPANS], net[MAX_SPANS], lo[MAX_SPANS], hi[MAX_SPANS];
    int32_t first[MAX_SPANS + 1];   // own workgroups: span k's first workgroup; first[nact] = the grid
    int32_t nact;                   // 1 .. MAX_SPANS
    int32_t shared;                 // 1: fewer workgroups than active spans
};

// Per-wave LDS (floats / ints)
struct WaveLds {
    float ego[SEGS][LD];     // f0's per-segment part: bias + ship columns
    float pool[SEGS][LD];    // max over the segment's rows after f.1
    float tile[SEGS][LD];    // phase A: the chunk's ship features, 8 floats per (env, ship); phase B: a tile's D
    int segoff[SEGS + 1];    // first item of each segment, and the chunk's total
    int cnp[SEGS], cnb[SEGS];   // per env of the chunk: planets, bullets (clamped)
};
static_assert(SEGS * 2 * 8 <= SEGS * LD, "phase A's ship features fit the tile");

// Raw weights as staged for the registers' load: [5][32][LD] for f.0, f.1, v.0, v.1, v0
constexpr int STAGE_FLOATS = 5 * NH * LD;
constexpr int WAVE_FLOATS = int(sizeof(WaveLds) / 4);
constexpr int UNION_FLOATS = STAGE_FLOATS > QN_WAVES * WAVE_FLOATS ? STAGE_FLOATS : QN_WAVES * WAVE_FLOATS;

template <typename T, int S>
__global__ __launch_bounds__(QN_BLOCK, 2) void astro_qpool_kernel(AstroParams p, AstroState st, Work work, int nout,
                                                               float *__restrict__ q_out,
                                                               int8_t *__restrict__ ctl_out, Explore ex) {
    using V = typename Store<T>::V;
    constexpr int NF = 5 + 5 * S;
    constexpr int OBJ = 1 + 5 * S;         // first object column
    __shared__ float s_w0[NH][16];         // f0.weight, row stride 16
    __shared__ float s_b[6][NH];           // f0, f.0, f.1, v.0, v.1, v0 biases (v0's padded with 0)
    __shared__ __attribute__((aligned(16))) float s_union[UNION_FLOATS];

    const int t = threadIdx.x;
    const int l = t & 63, wv = t >> 6;
    const int c = l & 31, h = l >> 5;
    const size_t NN = size_t(st.n_env);

    // This workgroup's spans [k0, k1), and its place (mine of nblk) among the
    // workgroups of a span: all of it from blockIdx and the arguments alone
    int k0, k1, mine = 0, nblk = 1;
    if (work.shared) {
        k0 = int(blockIdx.x) * work.nact / int(gridDim.x);
        k1 = (int(blockIdx.x) + 1) * work.nact / int(gridDim.x);
    } else {
        k0 = 0;
        for (int d = MAX_SPANS / 2; d >= 1; d >>= 1)   // the last k with first[k] <= blockIdx
            if (k0 + d < work.nact && work.first[k0 + d] <= int(blockIdx.x)) k0 += d;
        k1 = k0 + 1;
        mine = int(blockIdx.x) - work.first[k0];
        nblk = work.first[k0 + 1] - work.first[k0];
    }

    float w0r[3], wf0[16], wf1[16], wv0[16], wv1[16], wq[16];
    int staged = -1;
    WaveLds &W = *reinterpret_cast<WaveLds *>(s_union + wv * WAVE_FLOATS);
    const float ninf = -__builtin_huge_valf();

    for (int k = k0; k < k1; ++k) {
    const int net = work.net[k];
    const int ship = S == 1 ? 0 : work.ship[k];
    const int lo = work.lo[k], hi = work.hi[k];

    // ---- stage the weights (whole workgroup), then each lane's operand registers ----
    if (net != staged) {
        staged = net;
        {
            const float *w = work.w[net];
            for (int kk = t; kk < NH * NF; kk += QN_BLOCK) s_w0[kk / NF][kk % NF] = w[kk];
            w += NH * NF;
            for (int kk = t; kk < NH; kk += QN_BLOCK) s_b[0][kk] = w[kk];
            w += NH;
            for (int L = 0; L < 4; ++L) {
                for (int kk = t; kk < NH * NH; kk += QN_BLOCK) s_union[(L * NH + (kk >> 5)) * LD + (kk & 31)] = w[kk];
                w += NH * NH;
                for (int kk = t; kk < NH; kk += QN_BLOCK) s_b[1 + L][kk] = w[kk];
                w += NH;
            }
            for (int kk = t; kk < NH * NH; kk += QN_BLOCK)
                s_union[(4 * NH + (kk >> 5)) * LD + (kk & 31)] = (kk >> 5) < nout ? w[kk] : 0.0f;
            w += nout * NH;
            for (int kk = t; kk < NH; kk += QN_BLOCK) s_b[5][kk] = kk < nout ? w[kk] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int k3 = 0; k3 < 3; ++k3) {   // f0's object part: k = (type, x, y, dx, dy, 0)
            const int kk = 2 * k3 + h;
            w0r[k3] = kk == 0 ? s_w0[c][0] : (kk < 5 ? s_w0[c][OBJ + kk - 1] : 0.0f);
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int o = out_of(j, h);
            wf0[j] = s_union[(0 * NH + c) * LD + o];
            wf1[j] = s_union[(1 * NH + c) * LD + o];
            wv0[j] = s_union[(2 * NH + c) * LD + 2 * j + h];   // the pooled vector arrives in natural order
            wv1[j] = s_union[(3 * NH + c) * LD + o];
            wq[j] = s_union[(4 * NH + c) * LD + o];
        }
        __syncthreads();   // the staging area becomes the waves' own buffers
    }

    const int nchunks = (hi - lo + SEGS - 1) / SEGS;
    for (int chunk = mine * QN_WAVES + wv; chunk < nchunks; chunk += nblk * QN_WAVES) {
        const int e0 = lo + chunk * SEGS;   // < hi
        const int left = hi - e0;           // the chunk's envs are e0 + (0 .. min(left, 32) - 1)

        // ---- phase A: both ships' features, counts, prefix sum, per-segment part of f0 ----
        int rows = 0;
        if (l < SEGS * S) {
            const int le = l & 31, s = l >> 5;   // lane half = ship
            float f0 = 0.f, f1 = 0.f, f2 = 0.f, f3 = 0.f, f4 = 0.f;
            if (le < left) {
                const int i = e0 + le;
                const int4 hd = reinterpret_cast<const int4 *>(st.hdr)[i];
                if (s == 0) {
                    int np = hd.y & 0xff;
                    np = np < 1 ? 1 : (np > p.p_pad ? p.p_pad : np);
                    const int nb = min(int(uint32_t(hd.y) >> 16), p.b_cap);
                    rows = np + nb;
                    W.cnp[le] = np;
                    W.cnb[le] = nb;
                }
                const bool t0 = (uint32_t(hd.x) & TICK_MASK) == 0;
                const V v = reinterpret_cast<const V *>(st.ships)[size_t(s) * NN + i];
                const T b = reinterpret_cast<const T *>(st.ships_b)[size_t(s) * NN + i];
                f0 = float(v.x);
                f1 = float(v.y);
                f2 = float(v.z);
                f3 = float(v.w);
                f4 = t0 ? norm_angle_over_pi<float>(float(b)) : float(norm_angle_over_pi<double>(double(b)));
            }
            float *sf = &W.tile[0][0] + (le * S + s) * 8;
            sf[0] = f0;
            sf[1] = f1;
            sf[2] = f2;
            sf[3] = f3;
            sf[4] = f4;
        }
        {   // inclusive scan of rows over lanes 0..31 (lanes 32..63 hold 0)
            int incl = rows;
#pragma unroll
            for (int d = 1; d < 32; d <<= 1) {
                const int up = __shfl_up(incl, d, 64);
                if (l >= d) incl += up;
            }
            if (l < SEGS) W.segoff[l] = incl - rows;
            if (l == SEGS - 1) W.segoff[SEGS] = incl;
        }
        wave_fence();
        if (l < SEGS) {
            float f[5 * S];
#pragma unroll
            for (int j = 0; j < S; ++j) {
                const int sh = (ship + j) % S;   // core.roll_ships: the ego's own ship first
                const float *sf = &W.tile[0][0] + (l * S + sh) * 8;
#pragma unroll
                for (int kk = 0; kk < 5; ++kk) f[5 * j + kk] = sf[kk];
            }
            for (int o = 0; o < NH; ++o) {
                float acc = s_b[0][o];
#pragma unroll
                for (int kk = 0; kk < 5 * S; ++kk) acc = fmaf(s_w0[o][1 + kk], f[kk], acc);
                W.ego[l][o] = acc;
            }
        }
        wave_fence();
        const int total = __builtin_amdgcn_readfirstlane(W.segoff[SEGS]);

        // ---- phase B: the chunk's object rows, 32 per tile ----
        // A tile's rows are fetched one tile ahead, so their memory latency
        // runs under the previous tile's MFMAs.
        struct Rows {
            int g;          // the column's segment (the env within the chunk), -1 past the chunk's items
            float ty, ox, oy, odx, ody;
        };
        auto fetch = [&](int base) {
            Rows rw{-1, 0.f, 0.f, 0.f, 0.f, 0.f};
            const int item = base + c;
            if (item < total) {
                int g = 0;
#pragma unroll
                for (int d = 16; d >= 1; d >>= 1)
                    if (W.segoff[g + d] <= item) g += d;
                const int i = e0 + g;
                const int r = item - W.segoff[g], np = W.cnp[g];
                // a segment with items is an env below hi (the others have rows = 0), and
                // r < np + nb <= p_pad + b_cap by the prefix sum: both reads are inside the env's slots
                const V o = r < np ? reinterpret_cast<const V *>(st.planets)[size_t(r) * NN + i]
                                   : reinterpret_cast<const V *>(st.bullets)[size_t(i) * size_t(p.b_cap) + (r - np)];
                rw.g = g;
                rw.ty = r < np ? 0.0f : 1.0f;
                rw.ox = float(o.x);
                rw.oy = float(o.y);
                rw.odx = float(o.z);
                rw.ody = float(o.w);
            }
            return rw;
        };
        // the segment being pooled and its maximum so far run across tiles
        // (wave-uniform segment, one output per lane: both halves alike)
        int cur = -1;
        float m = ninf;
        Rows next = fetch(0);
        for (int base = 0; base < total; base += 32) {
            const Rows rw = next;
            if (base + 32 < total) next = fetch(base + 32);
            f32x16 acc;
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[j] = rw.g >= 0 ? W.ego[rw.g < 0 ? 0 : rw.g][out_of(j, h)] : 0.0f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w0r[0], h ? rw.ox : rw.ty, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w0r[1], h ? rw.odx : rw.oy, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w0r[2], h ? 0.0f : rw.ody, acc, 0, 0, 0);
            f32x16 x;
#pragma unroll
            for (int j = 0; j < 16; ++j) x[j] = softsign(acc[j]);
            acc = layer(wf0, x, bias_of(s_b[1], h));
#pragma unroll
            for (int j = 0; j < 16; ++j) x[j] = softsign(acc[j]);
            acc = layer(wf1, x, bias_of(s_b[2], h));
#pragma unroll
            for (int j = 0; j < 16; ++j) W.tile[c][out_of(j, h)] = acc[j];
            wave_fence();
            // max per segment: every lane walks the tile's 32 columns for
            // output c; a finished segment's maximum is stored, the last
            // one's carries into the next tile
            float v[32];
#pragma unroll
            for (int cc = 0; cc < 32; ++cc) v[cc] = W.tile[cc][c];
#pragma unroll
            for (int cc = 0; cc < 32; ++cc) {
                const int sg = __builtin_amdgcn_readlane(rw.g, cc);
                if (sg != cur) {
                    if (cur >= 0) W.pool[cur][c] = m;
                    cur = sg;
                    m = v[cc];
                } else {
                    m = fmaxf(m, v[cc]);
                }
            }
            wave_fence();
        }
        if (cur >= 0) W.pool[cur][c] = m;
        wave_fence();

        // ---- phase C: the head on the chunk's 32 pooled vectors (column c = env e0 + c) ----
        {
            const bool valid = c < left;
            f32x16 x;
#pragma unroll
            for (int j = 0; j < 16; ++j) x[j] = valid ? W.pool[c][2 * j + h] : 0.0f;
            f32x16 acc = layer(wv0, x, bias_of(s_b[3], h));
#pragma unroll
            for (int j = 0; j < 16; ++j) x[j] = softsign(acc[j]);
            acc = layer(wv1, x, bias_of(s_b[4], h));
#pragma unroll
            for (int j = 0; j < 16; ++j) x[j] = softsign(acc[j]);
            acc = layer(wq, x, bias_of(s_b[5], h));
            // outputs 0..3 are registers 0..3 of half 0, outputs 4, 5 registers 0, 1 of half 1
            float qv[6];
#pragma unroll
            for (int j = 0; j < 4; ++j) qv[j] = tanhf(acc[j]);
            qv[4] = __shfl_down(qv[0], 32, 64);
            qv[5] = __shfl_down(qv[1], 32, 64);
            if (valid && h == 0) {
                const int i = e0 + c;                              // lo <= i < hi <= n_env
                const size_t sid = size_t(i) * S + size_t(ship);   // < n_env * nships: inside q and control
                if (q_out) {
                    float *qo = q_out + sid * size_t(nout);
#pragma unroll
                    for (int o = 0; o < 6; ++o)
                        if (o < nout) qo[o] = qv[o];
                }
                if (ctl_out) {
                    int best = 0;
                    float bq = qv[0];
#pragma unroll
                    for (int o = 1; o < 6; ++o)
                        if (o < nout && qv[o] > bq) {
                            bq = qv[o];
                            best = o;
                        }
                    if (ex.on) {
                        const uint64_t id = uint64_t(ex.env_offset + i) * uint64_t(S) + uint64_t(ship);
                        const uint64_t z = random_word(id, ex.tick0, ex.seed);
                        if (uint64_t(uint32_t(z)) < ex.threshold) best = int(((z >> 32) * 6ull) >> 32);
                    }
                    ctl_out[sid] = int8_t(best);
                }
            }
        }
        wave_fence();
    }
    __syncthreads();   // every wave is done with its buffers before the next network is staged over them
    }
}

// ---------------------------------------------------------------------------
// host side

// The workgroups of the launch: fills work.first / work.shared, returns the grid.
// u[k]: the workgroups of span k that find a chunk of their own.
int share_out(Work &work, int max_blocks) {
    const int cap = max_blocks > 0 ? max_blocks : MAX_BLOCKS;
    const int nact = work.nact;
    if (cap < nact) {   // fewer workgroups than spans: each serves several, one after the other
        work.shared = 1;
        return cap;
    }
    int64_t u[MAX_SPANS], total = 0;
    for (int k = 0; k < nact; ++k) {
        const int64_t chunks = (int64_t(work.hi[k]) - work.lo[k] + SEGS - 1) / SEGS;
        u[k] = (chunks + QN_WAVES - 1) / QN_WAVES;
        total += u[k];
    }
    // one workgroup each, the rest of the cap in proportion to what is left of every span
    const int64_t rest = cap - nact;
    int grid = 0;
    for (int k = 0; k < nact; ++k) {
        work.first[k] = grid;
        grid += int(total <= cap ? u[k] : 1 + (u[k] - 1) * rest / (total - nact));
    }
    work.first[nact] = grid;
    work.shared = 0;
    return grid;
}

template <typename T, int S>
int launch(const AstroParams &p, const AstroState &s, const Work &work, int grid, int nout, float *q, int8_t *control,
           const Explore &ex, hipStream_t stream) {
    hipLaunchKernelGGL((astro_qpool_kernel<T, S>), dim3(unsigned(grid)), dim3(QN_BLOCK), 0, stream, p, s, work, nout, q,
                       control, ex);
    return launched("astro_qvalues_pool");
}

}  // namespace

extern "C" {

int astro_qpool_abi_version(void) { return ASTRO_QPOOL_ABI_VERSION; }

const char *astro_qpool_last_error(void) { return g_err; }

int astro_qvalues_pool(const AstroParams *p, const AstroState *s, const AstroQNet *nets, int32_t nnets,
                       const AstroQSpan *spans, int32_t nspans, float *q, int8_t *control, const AstroPolicy *explore,
                       double epsilon, int32_t max_blocks, void *stream) {
    if (!p) return fail(-10, "params is NULL");
    if (!s) return fail(-2, "state is NULL");
    if (!nets) return fail(-120, "nets is NULL");
    if (!spans) return fail(-130, "spans is NULL");
    if (p->nships != 1 && p->nships != 2) return fail(-11, "nships must be 1 or 2");
    if (p->p_pad < 1 || p->p_pad > 16) return fail(-13, "p_pad must be in [1, 16]");
    if (p->b_cap < 1 || p->b_cap > 65535) return fail(-15, "b_cap must be in [1, 65535]");
    if (nnets < 1 || nnets > MAX_NETS) return fail(-131, "nnets must be in [1, %d], got %d", MAX_NETS, int(nnets));
    if (nspans < 1 || nspans > MAX_SPANS)
        return fail(-132, "nspans must be in [1, %d], got %d", MAX_SPANS, int(nspans));
    if (s->n_env < 0) return fail(-3, "n_env < 0");
    for (int k = 0; k < nspans; ++k)
        if (spans[k].ship < 0 || spans[k].ship >= p->nships)
            return fail(-133, "spans[%d].ship must be in [0, %d), got %d", k, int(p->nships), int(spans[k].ship));
    for (int k = 0; k < nspans; ++k)
        if (spans[k].net < -1 || spans[k].net >= nnets)
            return fail(-134, "spans[%d].net must be -1 or in [0, %d), got %d", k, int(nnets), int(spans[k].net));
    for (int k = 0; k < nspans; ++k)
        if (spans[k].lo < 0 || spans[k].lo > spans[k].hi || spans[k].hi > s->n_env)
            return fail(-135, "spans[%d] must have 0 <= lo <= hi <= n_env (%d), got [%d, %d)", k, int(s->n_env),
                        int(spans[k].lo), int(spans[k].hi));
    for (int a = 0; a < nspans; ++a)
        for (int b = a + 1; b < nspans; ++b)
            if (spans[a].ship == spans[b].ship && spans[a].lo < spans[a].hi && spans[b].lo < spans[b].hi &&
                spans[a].lo < spans[b].hi && spans[b].lo < spans[a].hi)
                return fail(-136, "spans[%d] and spans[%d] of ship %d overlap", a, b, int(spans[a].ship));
    bool used[MAX_NETS] = {};
    int one = -1;   // a used network: its nout is everyone's
    for (int k = 0; k < nspans; ++k)
        if (spans[k].net >= 0) {
            used[spans[k].net] = true;
            if (one < 0 || spans[k].net < one) one = spans[k].net;
        }
    for (int n = 0; n < nnets; ++n)
        if (used[n] && nets[n].nships != p->nships)
            return fail(-101, "nets[%d].nships (%d) must equal params.nships (%d)", n, int(nets[n].nships),
                        int(p->nships));
    for (int n = 0; n < nnets; ++n)
        if (used[n] && (nets[n].nout < 1 || nets[n].nout > ASTRO_QNET_MAX_OUT))
            return fail(-102, "nets[%d].nout must be in [1, %d], got %d", n, ASTRO_QNET_MAX_OUT, int(nets[n].nout));
    for (int n = 0; n < nnets; ++n)
        if (used[n] && nets[n].nout != nets[one].nout)
            return fail(-122, "the nets differ in nout (nets[%d]: %d, nets[%d]: %d)", one, int(nets[one].nout), n,
                        int(nets[n].nout));
    if (!q && !control) return fail(-103, "q and control are both NULL");
    if (!(epsilon >= 0.0 && epsilon <= 1.0)) return fail(-104, "epsilon must be in [0, 1], got %g", epsilon);
    if (max_blocks < 0) return fail(-123, "max_blocks must be >= 0, got %d", int(max_blocks));

    // the active spans, sorted by network (a shared workgroup restages as rarely as it can)
    Work work{};
    int order[MAX_SPANS];
    for (int k = 0; k < nspans; ++k)
        if (spans[k].net >= 0 && spans[k].lo < spans[k].hi) order[work.nact++] = k;
    if (work.nact == 0) return 0;
    std::stable_sort(order, order + work.nact, [&](int a, int b) { return spans[a].net < spans[b].net; });
    for (int k = 0; k < work.nact; ++k) {
        const AstroQSpan &sp = spans[order[k]];
        work.ship[k] = sp.ship;
        work.net[k] = sp.net;
        work.lo[k] = sp.lo;
        work.hi[k] = sp.hi;
    }
    for (int n = 0; n < nnets; ++n)
        if (used[n]) {
            if (!nets[n].weights || !aligned(nets[n].weights, 4))
                return fail(-105, "nets[%d].weights must be a 4-byte aligned device pointer", n);
            work.w[n] = nets[n].weights;
        }
    if (!s->ships || !s->ships_b || !s->planets || !s->bullets || !s->hdr) return fail(-4, "a state array is NULL");
    if (!aligned(s->ships, 16) || !aligned(s->planets, 16) || !aligned(s->bullets, 16) || !aligned(s->hdr, 16))
        return fail(-5, "ships/planets/bullets/hdr must be 16-byte aligned");
    if (s->state_f64 != 0 && s->state_f64 != 1) return fail(-6, "state_f64 must be 0 or 1");
    if (q && !aligned(q, 4)) return fail(-106, "q must be 4-byte aligned");

    Explore ex{};
    if (explore) {
        ex.on = 1;
        ex.seed = explore->seed;
        ex.tick0 = explore->tick0;
        ex.env_offset = explore->env_offset;
        ex.threshold = uint64_t(epsilon * 4294967296.0);
    }
    const int grid = share_out(work, max_blocks);
    const int nout = int(nets[one].nout);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (s->state_f64)
        return p->nships == 1 ? launch<double, 1>(*p, *s, work, grid, nout, q, control, ex, st)
                              : launch<double, 2>(*p, *s, work, grid, nout, q, control, ex, st);
    return p->nships == 1 ? launch<float, 1>(*p, *s, work, grid, nout, q, control, ex, st)
                          : launch<float, 2>(*p, *s, work, grid, nout, q, control, ex, st);
}

}  // extern "C"
