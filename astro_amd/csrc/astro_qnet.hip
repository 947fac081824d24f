// libastro_qnet.so: rl.ValueNetwork.forward + rl.QBot's argmax (+ epsilon-greedy)
// for every ship of every env, fused over the AstroState arrays
// (include/astro_qnet.h).
//
// Layout.  A workgroup is four waves that share nothing but the staged
// weights; each wave owns chunks of CH = 32 / S consecutive envs, i.e. 32
// (env, ego) SEGMENTS, and walks them in three phases:
//
//   A  per segment: the ships' features of the ego view and the part of f0
//      that depends on them only (bias + ship columns), kept in LDS; per
//      env the live-row counts and their prefix sum.
//   B  the chunk's live object rows, 32 at a time, as the 32 columns of an
//      f32-input MFMA tile (v_mfma_f32_32x32x2_f32, A = W, B = X^T, so
//      D[out][row] has one object row per lane column): f0's object part
//      (K = 5 padded to 6: 3 MFMAs on top of the segment's part as the
//      initial accumulator), softsign, f.0, softsign, f.1 (16 MFMAs each),
//      then a max per segment into LDS.  A tile holds rows of several
//      segments and a segment spans several tiles.
//   C  the head on the 32 pooled vectors as one more tile: v.0, v.1, v0
//      (16 MFMAs each), tanh, argmax, exploration, stores.
//
// D's rows sit in the 16 accumulator registers of a lane: register j of lane
// half h is output (j & 3) + 8 (j >> 2) + 4 h.  The next layer sums over that
// index, so it takes register j as the B operand of its k-step j, and its A
// operand (the weights, loaded once per wave into registers) has its columns
// permuted to match: no lane movement between layers.
//
// Numerics: float32 throughout (the MFMA is an exact f32 fma chain).  What
// differs from the reference's float32 forward: the summation order,
// softsign's divide (a multiply by v_rcp_f32, 1 ulp) and tanhf.
#include <algorithm>

#include "astro_common.h"
#include "astro_qnet.h"

namespace {

constexpr int NH = ASTRO_QNET_HIDDEN;
constexpr int QN_WAVES = 4;
constexpr int QN_BLOCK = 64 * QN_WAVES;
constexpr int SEGS = 32;          // (env, ego) segments per chunk = columns of the head's tile
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

// Per-wave LDS (floats / ints)
struct WaveLds {
    float ego[SEGS][LD];     // f0's per-segment part: bias + ship columns
    float pool[SEGS][LD];    // max over the segment's rows after f.1
    float tile[SEGS][LD];    // phase A: the chunk's ship features; phase B: a tile's D, [column][out]
    int segoff[SEGS + 1];    // first item of each segment, and the chunk's total
    int cnp[SEGS], cnb[SEGS];   // per env of the chunk: planets, bullets (clamped)
};

// Raw weights as staged for the registers' load: [5][32][LD] for f.0, f.1, v.0, v.1, v0
constexpr int STAGE_FLOATS = 5 * NH * LD;
constexpr int WAVE_FLOATS = int(sizeof(WaveLds) / 4);
constexpr int UNION_FLOATS = STAGE_FLOATS > QN_WAVES * WAVE_FLOATS ? STAGE_FLOATS : QN_WAVES * WAVE_FLOATS;

template <typename T, int S>
__global__ __launch_bounds__(QN_BLOCK, 2) void astro_qvalues_kernel(AstroParams p, AstroState st,
                                                                 const float *__restrict__ wts, int nout,
                                                                 float *__restrict__ q_out,
                                                                 int8_t *__restrict__ ctl_out, Explore ex,
                                                                 int nchunks) {
    using V = typename Store<T>::V;
    constexpr int NF = 5 + 5 * S;
    constexpr int CH = SEGS / S;           // envs per chunk
    constexpr int OBJ = 1 + 5 * S;         // first object column
    __shared__ float s_w0[NH][16];         // f0.weight, row stride 16
    __shared__ float s_b[6][NH];           // f0, f.0, f.1, v.0, v.1, v0 biases (v0's padded with 0)
    __shared__ __attribute__((aligned(16))) float s_union[UNION_FLOATS];

    const int t = threadIdx.x;
    const int l = t & 63, wv = t >> 6;
    const int c = l & 31, h = l >> 5;
    const int N = st.n_env;
    const size_t NN = size_t(N);

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

    for (int chunk = blockIdx.x * QN_WAVES + wv; chunk < nchunks; chunk += gridDim.x * QN_WAVES) {
        const int e0 = chunk * CH;

        // ---- phase A: ships' features, counts, prefix sum, per-segment part of f0 ----
        int rows = 0;
        if (l < SEGS) {
            const int le = l / S, s = l - le * S, i = e0 + le;
            float f0 = 0.f, f1 = 0.f, f2 = 0.f, f3 = 0.f, f4 = 0.f;
            if (i < N) {
                const int4 hd = reinterpret_cast<const int4 *>(st.hdr)[i];
                int np = hd.y & 0xff;
                np = np < 1 ? 1 : (np > p.p_pad ? p.p_pad : np);
                const int nb = min(int(uint32_t(hd.y) >> 16), p.b_cap);
                rows = np + nb;
                if (s == 0) {
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
            float *sf = &W.tile[0][0] + l * 8;
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
            const int le = l / S, ego = l - le * S;
            float f[5 * S];
#pragma unroll
            for (int j = 0; j < S; ++j) {
                const int sh = (ego + j) % S;   // core.roll_ships: the ego's own ship first
                const float *sf = &W.tile[0][0] + (le * S + sh) * 8;
#pragma unroll
                for (int k = 0; k < 5; ++k) f[5 * j + k] = sf[k];
            }
            for (int o = 0; o < NH; ++o) {
                float a = s_b[0][o];
#pragma unroll
                for (int k = 0; k < 5 * S; ++k) a = fmaf(s_w0[o][1 + k], f[k], a);
                W.ego[l][o] = a;
            }
        }
        wave_fence();
        const int total = __builtin_amdgcn_readfirstlane(W.segoff[SEGS]);

        // ---- phase B: the chunk's object rows, 32 per tile ----
        // A tile's rows are fetched one tile ahead, so their memory latency
        // runs under the previous tile's MFMAs.
        struct Rows {
            int g;          // the column's segment, -1 past the chunk's items
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
                const int le = g / S, i = e0 + le;
                const int r = item - W.segoff[g], np = W.cnp[le];
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

        // ---- phase C: the head on the chunk's 32 pooled vectors (column c = segment c) ----
        {
            const int le = c / S, s = c - le * S, i = e0 + le;
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
                const size_t sid = size_t(i) * S + s;
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
                        const uint64_t id = uint64_t(ex.env_offset + i) * uint64_t(S) + uint64_t(s);
                        const uint64_t z = random_word(id, ex.tick0, ex.seed);
                        if (uint64_t(uint32_t(z)) < ex.threshold) best = int(((z >> 32) * 6ull) >> 32);
                    }
                    ctl_out[sid] = int8_t(best);
                }
            }
        }
        wave_fence();
    }
}

// ---------------------------------------------------------------------------
// host side

template <typename T, int S>
int launch(const AstroParams &p, const AstroState &s, const AstroQNet &net, float *q, int8_t *control,
           const Explore &ex, hipStream_t stream) {
    constexpr int CH = SEGS / S;
    const int nchunks = (s.n_env + CH - 1) / CH;
    const int blocks = std::min((nchunks + QN_WAVES - 1) / QN_WAVES, MAX_BLOCKS);
    hipLaunchKernelGGL((astro_qvalues_kernel<T, S>), dim3(unsigned(blocks)), dim3(QN_BLOCK), 0, stream, p, s,
                       net.weights, int(net.nout), q, control, ex, nchunks);
    return launched("astro_qvalues");
}

}  // namespace

extern "C" {

int astro_qnet_abi_version(void) { return ASTRO_QNET_ABI_VERSION; }

const char *astro_qnet_last_error(void) { return g_err; }

int astro_qvalues(const AstroParams *p, const AstroState *s, const AstroQNet *net, float *q, int8_t *control,
                  const AstroPolicy *explore, double epsilon, void *stream) {
    if (!p) return fail(-10, "params is NULL");
    if (!s) return fail(-2, "state is NULL");
    if (!net) return fail(-100, "net is NULL");
    if (p->nships != 1 && p->nships != 2) return fail(-11, "nships must be 1 or 2");
    if (p->p_pad < 1 || p->p_pad > 16) return fail(-13, "p_pad must be in [1, 16]");
    if (p->b_cap < 1 || p->b_cap > 65535) return fail(-15, "b_cap must be in [1, 65535]");
    if (net->nships != p->nships)
        return fail(-101, "net.nships (%d) must equal params.nships (%d)", int(net->nships), int(p->nships));
    if (net->nout < 1 || net->nout > ASTRO_QNET_MAX_OUT)
        return fail(-102, "net.nout must be in [1, %d], got %d", ASTRO_QNET_MAX_OUT, int(net->nout));
    if (!q && !control) return fail(-103, "q and control are both NULL");
    if (!(epsilon >= 0.0 && epsilon <= 1.0)) return fail(-104, "epsilon must be in [0, 1], got %g", epsilon);
    if (s->n_env < 0) return fail(-3, "n_env < 0");
    if (s->n_env == 0) return 0;
    if (!net->weights || !aligned(net->weights, 4)) return fail(-105, "net.weights must be a 4-byte aligned device pointer");
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
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (s->state_f64)
        return p->nships == 1 ? launch<double, 1>(*p, *s, *net, q, control, ex, st)
                              : launch<double, 2>(*p, *s, *net, q, control, ex, st);
    return p->nships == 1 ? launch<float, 1>(*p, *s, *net, q, control, ex, st)
                          : launch<float, 2>(*p, *s, *net, q, control, ex, st);
}

}  // extern "C"
