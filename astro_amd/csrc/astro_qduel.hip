// libastro_qduel.so: astro_qvalues (csrc/astro_qnet.hip) with one network per
// ship, or none (include/astro_qduel.h).
//
// Layout.  astro_qvalues mixes the segments of both ships into one 32-column
// tile and keeps ONE network's five 32x32 layers as per-lane MFMA operand
// registers, so it cannot serve two weight sets.  Here the work is ship-major:
// a workgroup stages the weights of ONE ship's network and serves that ship
// for its whole life (block b serves the (b mod active ships)-th ship that has
// a network); a chunk is 32 consecutive envs of that ship, i.e. again 32
// SEGMENTS, one per env.  A ship without a network gets no workgroup and no
// chunk: nothing of it is read or written.  The three phases are
// astro_qvalues':
//
//   A  the features of BOTH ships of the chunk's 32 envs, one (env, ship) per
//      lane of the whole wave, into LDS; per env the live-row counts and their
//      prefix sum; per segment the part of f0 that depends on the ships only,
//      in the served ship's ego view.
//   B  the chunk's live object rows, 32 at a time, as the 32 columns of an
//      f32-input MFMA tile: f0's object part on top of the segment's part,
//      softsign, f.0, softsign, f.1, then a max per segment into LDS.
//   C  the head on the 32 pooled vectors as one more tile, tanh, argmax,
//      exploration, stores.
//
// Bit identity with astro_qvalues.  Every value a column of a tile holds
// depends on that column's own inputs only (the MFMA's columns do not
// interact, and every other operation is per lane), each row's chain of
// operations is astro_qvalues' -- the same fmaf order for the ship part of f0,
// the same MFMA sequence and k order, the same softsign, the same tanhf --
// and the pool takes a segment's rows in the same order.  Which other
// segments share a tile therefore changes nothing: ship s's q and control are
// astro_qvalues' with nets[s], bit for bit.
//
// The device helpers that both sources need and astro_common.h does not have
// (Store, softsign, layer, Explore, WaveLds) are restated here, so
// libastro_qnet.so is what it was.
#include <algorithm>

#include "astro_common.h"
#include "astro_qduel.h"

namespace {

constexpr int NH = ASTRO_QNET_HIDDEN;
constexpr int QN_WAVES = 4;
constexpr int QN_BLOCK = 64 * QN_WAVES;
constexpr int SEGS = 32;          // envs per chunk = columns of the head's tile
constexpr int LD = NH + 1;        // LDS row stride of a [32][32] float image (bank-conflict-free columns)
constexpr int MAX_BLOCKS = 512;   // two workgroups per CU on 256 CUs

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

// The ships that have a network, in ship order
struct Nets {
    const float *w[2];
    int32_t ship[2];
    int32_t nact;   // 1 or 2
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
__global__ __launch_bounds__(QN_BLOCK, 2) void astro_qduel_kernel(AstroParams p, AstroState st, Nets nets, int nout,
                                                               float *__restrict__ q_out,
                                                               int8_t *__restrict__ ctl_out, Explore ex,
                                                               int nchunks) {
    using V = typename Store<T>::V;
    constexpr int NF = 5 + 5 * S;
    constexpr int OBJ = 1 + 5 * S;         // first object column
    __shared__ float s_w0[NH][16];         // f0.weight, row stride 16
    __shared__ float s_b[6][NH];           // f0, f.0, f.1, v.0, v.1, v0 biases (v0's padded with 0)
    __shared__ __attribute__((aligned(16))) float s_union[UNION_FLOATS];

    const int t = threadIdx.x;
    const int l = t & 63, wv = t >> 6;
    const int c = l & 31, h = l >> 5;
    const int N = st.n_env;
    const size_t NN = size_t(N);

    // The grid is one workgroup or a multiple of nact (the host sees to it):
    // `sets` groups of workgroups, one per network; a lone workgroup with two
    // networks (max_blocks = 1) takes them in turn.
    const int sets = min(int(gridDim.x), nets.nact);
    const int per_set = int(gridDim.x) / sets;
    const int first_chunk = (int(blockIdx.x) / sets) * QN_WAVES + wv;

    for (int a = int(blockIdx.x) % sets; a < nets.nact; a += sets) {
    const float *__restrict__ wts = a == 0 ? nets.w[0] : nets.w[1];
    const int ship = S == 1 ? 0 : (a == 0 ? nets.ship[0] : nets.ship[1]);

    // ---- stage the weights (whole workgroup), then each lane's operand registers ----
    {
        const float *w = wts;
        for (int k = t; k < NH * NF; k += QN_BLOCK) s_w0[k / NF][k % NF] = w[k];
        w += NH * NF;
        for (int k = t; k < NH; k += QN_BLOCK) s_b[0][k] = w[k];
        w += NH;
        for (int L = 0; L < 4; ++L) {
            for (int k = t; k < NH * NH; k += QN_BLOCK) s_union[(L * NH + (k >> 5)) * LD + (k & 31)] = w[k];
            w += NH * NH;
            for (int k = t; k < NH; k += QN_BLOCK) s_b[1 + L][k] = w[k];
            w += NH;
        }
        for (int k = t; k < NH * NH; k += QN_BLOCK)
            s_union[(4 * NH + (k >> 5)) * LD + (k & 31)] = (k >> 5) < nout ? w[k] : 0.0f;
        w += nout * NH;
        for (int k = t; k < NH; k += QN_BLOCK) s_b[5][k] = k < nout ? w[k] : 0.0f;
    }
    __syncthreads();
    float w0r[3], wf0[16], wf1[16], wv0[16], wv1[16], wq[16];
#pragma unroll
    for (int k3 = 0; k3 < 3; ++k3) {   // f0's object part: k = (type, x, y, dx, dy, 0)
        const int k = 2 * k3 + h;
        w0r[k3] = k == 0 ? s_w0[c][0] : (k < 5 ? s_w0[c][OBJ + k - 1] : 0.0f);
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

    WaveLds &W = *reinterpret_cast<WaveLds *>(s_union + wv * WAVE_FLOATS);
    const float ninf = -__builtin_huge_valf();

    for (int chunk = first_chunk; chunk < nchunks; chunk += per_set * QN_WAVES) {
        const int e0 = chunk * SEGS;

        // ---- phase A: both ships' features, counts, prefix sum, per-segment part of f0 ----
        int rows = 0;
        if (l < SEGS * S) {
            const int le = l & 31, s = l >> 5, i = e0 + le;   // lane half = ship
            float f0 = 0.f, f1 = 0.f, f2 = 0.f, f3 = 0.f, f4 = 0.f;
            if (i < N) {
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
                for (int k = 0; k < 5; ++k) f[5 * j + k] = sf[k];
            }
            for (int o = 0; o < NH; ++o) {
                float acc = s_b[0][o];
#pragma unroll
                for (int k = 0; k < 5 * S; ++k) acc = fmaf(s_w0[o][1 + k], f[k], acc);
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
                // a segment with items is an env below N (the others have rows = 0), and
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
            const int i = e0 + c;
            const bool valid = i < N;
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

template <typename T, int S>
int launch(const AstroParams &p, const AstroState &s, const Nets &nets, int nout, float *q, int8_t *control,
           const Explore &ex, int max_blocks, hipStream_t stream) {
    const int nchunks = (s.n_env + SEGS - 1) / SEGS;                 // per ship
    const int per_set = (nchunks + QN_WAVES - 1) / QN_WAVES;         // workgroups that find a chunk, per ship
    const int cap = max_blocks > 0 ? max_blocks : MAX_BLOCKS;
    // one workgroup, or the same number for every ship that has a network
    const int blocks = cap < nets.nact ? 1 : std::min(per_set, cap / nets.nact) * nets.nact;
    hipLaunchKernelGGL((astro_qduel_kernel<T, S>), dim3(unsigned(blocks)), dim3(QN_BLOCK), 0, stream, p, s, nets, nout,
                       q, control, ex, nchunks);
    return launched("astro_qvalues_ships");
}

}  // namespace

extern "C" {

int astro_qduel_abi_version(void) { return ASTRO_QDUEL_ABI_VERSION; }

const char *astro_qduel_last_error(void) { return g_err; }

int astro_qvalues_ships(const AstroParams *p, const AstroState *s, const AstroQNet *const nets[2], float *q,
                        int8_t *control, const AstroPolicy *explore, double epsilon, int32_t max_blocks,
                        void *stream) {
    if (!p) return fail(-10, "params is NULL");
    if (!s) return fail(-2, "state is NULL");
    if (!nets) return fail(-120, "nets is NULL");
    if (p->nships != 1 && p->nships != 2) return fail(-11, "nships must be 1 or 2");
    if (p->p_pad < 1 || p->p_pad > 16) return fail(-13, "p_pad must be in [1, 16]");
    if (p->b_cap < 1 || p->b_cap > 65535) return fail(-15, "b_cap must be in [1, 65535]");
    Nets act{};
    const AstroQNet *have[2] = {nullptr, nullptr};
    for (int k = 0; k < p->nships; ++k)
        if (nets[k]) {
            have[act.nact] = nets[k];
            act.ship[act.nact++] = k;
        }
    if (act.nact == 0) return fail(-121, "every net is NULL");
    for (int k = 0; k < act.nact; ++k)
        if (have[k]->nships != p->nships)
            return fail(-101, "nets[%d].nships (%d) must equal params.nships (%d)", int(act.ship[k]),
                        int(have[k]->nships), int(p->nships));
    for (int k = 0; k < act.nact; ++k)
        if (have[k]->nout < 1 || have[k]->nout > ASTRO_QNET_MAX_OUT)
            return fail(-102, "nets[%d].nout must be in [1, %d], got %d", int(act.ship[k]), ASTRO_QNET_MAX_OUT,
                        int(have[k]->nout));
    if (act.nact == 2 && have[0]->nout != have[1]->nout)
        return fail(-122, "the nets differ in nout (%d and %d)", int(have[0]->nout), int(have[1]->nout));
    if (!q && !control) return fail(-103, "q and control are both NULL");
    if (!(epsilon >= 0.0 && epsilon <= 1.0)) return fail(-104, "epsilon must be in [0, 1], got %g", epsilon);
    if (max_blocks < 0) return fail(-123, "max_blocks must be >= 0, got %d", int(max_blocks));
    if (s->n_env < 0) return fail(-3, "n_env < 0");
    if (s->n_env == 0) return 0;
    for (int k = 0; k < act.nact; ++k) {
        if (!have[k]->weights || !aligned(have[k]->weights, 4))
            return fail(-105, "nets[%d].weights must be a 4-byte aligned device pointer", int(act.ship[k]));
        act.w[k] = have[k]->weights;
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
    const int nout = int(have[0]->nout);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (s->state_f64)
        return p->nships == 1 ? launch<double, 1>(*p, *s, act, nout, q, control, ex, max_blocks, st)
                              : launch<double, 2>(*p, *s, act, nout, q, control, ex, max_blocks, st);
    return p->nships == 1 ? launch<float, 1>(*p, *s, act, nout, q, control, ex, max_blocks, st)
                          : launch<float, 2>(*p, *s, act, nout, q, control, ex, max_blocks, st);
}

}  // extern "C"
