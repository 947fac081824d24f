// libastro_qtrain.so: rl.ValueNetwork.forward on a to_batch feature tensor and
// rl.QNetworkTrainer.step's loss gradient (include/astro_qtrain.h), on the
// packed weights of astro_qnet.h.
//
// Layout.  A workgroup is four waves that share nothing but the staged
// weights (in LDS for the whole kernel: every MFMA's A operand is one LDS
// read, which leaves the registers to the gradient accumulators).  Each wave
// owns chunks of 32 consecutive samples and keeps, for all its chunks, the
// six layers' weight-gradient tiles in its own registers.  Per chunk:
//
//   1  forward sweep over the chunk's LIVE rows, 32 at a time, as the 32
//      columns of an f32-input MFMA tile (v_mfma_f32_32x32x2_f32, A = W,
//      B = X^T, D[unit][row]): f0, softsign, f.0, softsign, f.1, then per
//      (sample, unit) the maximum and the first row that attains it, in LDS.
//      Live rows are found by a scan of column 0 (ballot + compaction into a
//      ring in LDS, one scan step and one tile's rows fetched ahead), so
//      padding costs a 4-byte read and no MFMA; a tile holds rows of several
//      samples and a sample spans several tiles.
//   2  the head on the 32 pooled vectors as one tile: v.0, v.1, v0, tanh;
//      then the loss, and the head backwards: for each layer dW += dZ X^T
//      (both operands transposed through LDS, the tile's column index is K)
//      and dX = W^T dZ (dZ straight from the accumulator registers, the
//      weights read transposed).  The pooled units' gradients go to LDS.
//   3  backward sweep over the live rows that are the argmax of at least one
//      pooled unit (at most 32 per sample; the others' gradient is zero, and
//      the scan drops them like padding): f0 and f.0 recomputed, dZ of f.1 is
//      the pooled unit's gradient where the row is the unit's argmax and 0
//      elsewhere, then f.1, f.0 and f0 backwards as in 2.
//
// D's rows sit in the 16 accumulator registers of a lane: register j of lane
// half h is unit (j & 3) + 8 (j >> 2) + 4 h.  A layer that consumes them takes
// register j as the B operand of its k-step j and reads its weights by the
// same index: no lane movement between layers.
//
// At the end every wave writes its partial gradient to the workspace and a
// second kernel adds the partials in float64 in a fixed order.
//
// Numerics: float32 throughout (the MFMA is an exact f32 fma chain).  What
// differs from torch's float32: the summation order, softsign's divide (a
// multiply by v_rcp_f32, 1 ulp; its derivative is that reciprocal squared)
// and tanhf.
#include <algorithm>

#include "astro_common.h"
#include "astro_qtrain.h"

namespace {

constexpr int NH = ASTRO_QNET_HIDDEN;
constexpr int QT_WAVES = 4;
constexpr int QT_BLOCK = 64 * QT_WAVES;
constexpr int SEGS = 32;          // samples per chunk = columns of the head's tile
constexpr int LD = NH + 1;        // LDS row stride of a [32][32] float image
constexpr int XLD = 17;           // LDS row stride of a [32][16] feature image
constexpr int MAX_BLOCKS = 256;   // one workgroup per CU (LDS) on 256 CUs
constexpr int RING = 512;         // live-row ring: 31 left over + one scan step
constexpr int SCAN = 4;           // column-0 loads in flight per lane and scan step
#ifndef ASTRO_QTRAIN_SPARSE
#define ASTRO_QTRAIN_SPARSE 1     // 0: the backward sweep visits every live row (the A/B of DESIGN.md section 13)
#endif
constexpr int RED_PARAMS = 16, RED_GROUPS = 16;   // the reduction's block: parameters x partial groups
constexpr int RED_BLOCK = RED_PARAMS * RED_GROUPS;

// 1 / (1 + |a|): the denominator is in [1, inf), so v_rcp_f32 (1 ulp) is safe.
// softsign(a) = a r, softsign'(a) = r r.
__device__ __forceinline__ float ss_rcp(float a) { return __builtin_amdgcn_rcpf(1.0f + fabsf(a)); }

// acc + W x: w is a [32][LD] image of torch's [out][in] rows, x the 32 inputs in a lane's 16 registers
__device__ __forceinline__ f32x16 layer_fwd(const float *w, const f32x16 &x, f32x16 acc, int c, int h) {
#pragma unroll
    for (int j = 0; j < 16; ++j)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[c * LD + out_of(j, h)], x[j], acc, 0, 0, 0);
    return acc;
}

// W^T d: the same image read by columns
__device__ __forceinline__ f32x16 layer_bwd(const float *w, const f32x16 &d, int c, int h) {
    f32x16 acc;
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.0f;
#pragma unroll
    for (int j = 0; j < 16; ++j)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[out_of(j, h) * LD + c], d[j], acc, 0, 0, 0);
    return acc;
}

// D-layout registers -> a [column][unit] image
__device__ __forceinline__ void put_tile(float (*t)[LD], const f32x16 &v, int c, int h) {
#pragma unroll
    for (int j = 0; j < 16; ++j) t[c][out_of(j, h)] = v[j];
}

// dW[u][i] += sum over the tile's columns of dz[col][u] x[col][i]; db: the lane's half of sum_col dz[col][c]
__device__ __forceinline__ void accum(f32x16 &dW, float &db, const float (*dz)[LD], const float (*x)[LD], int c,
                                      int h) {
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
        const float a = dz[2 * kk + h][c];
        dW = __builtin_amdgcn_mfma_f32_32x32x2f32(a, x[2 * kk + h][c], dW, 0, 0, 0);
        db += a;
    }
}

// Per-wave LDS
struct WaveLds {
    float pool[SEGS][LD];   // max over the sample's rows after f.1; after the head: its gradient
    int arg[SEGS][LD];      // the first row that attains it
    float ta[SEGS][LD];     // a tile's activations, [column][unit]
    float td[SEGS][LD];     // a tile's dZ (sweep 1: f.1's output), [column][unit]
    float xs[SEGS][XLD];    // a tile's feature rows, zero-padded to 16 columns
    int ring[RING];         // live slots (sample-in-chunk * rows + row) not yet in a tile
};

// The chunk's live rows in order, 32 per tile.  pos, head and cnt are
// wave-uniform; v holds column 0 of the slots [pos, pos + 64 SCAN), loaded one
// scan step ahead so that its latency runs under the tiles' MFMAs.
struct Scan {
    int pos, head, cnt;
    float v[SCAN];
};

__device__ __forceinline__ void scan_fetch(Scan &sc, const float *fchunk, int limit, int nf, int l) {
#pragma unroll
    for (int u = 0; u < SCAN; ++u) {
        const int slot = sc.pos + u * 64 + l;
        sc.v[u] = slot < limit ? fchunk[size_t(slot) * size_t(nf)] : -1.0f;
    }
}

__device__ __forceinline__ Scan scan_begin(const float *fchunk, int limit, int nf, int l) {
    Scan sc;
    sc.pos = sc.head = sc.cnt = 0;
    scan_fetch(sc, fchunk, limit, nf, l);
    return sc;
}

// Lane's column of the next tile: the slot, or -1 past the chunk's live rows.  Returns the tile's size in `take`.
// ARGMAX_ONLY (the backward sweep): of the live rows, only those that are the argmax of at least one of the
// sample's 32 pooled units -- the others' gradient is zero.
template <bool ARGMAX_ONLY>
__device__ __forceinline__ int next_tile(WaveLds &W, Scan &sc, const float *fchunk, int limit, int nf, int rows, int l,
                                         int &take) {
    while (sc.cnt < 32 && sc.pos < limit) {
#pragma unroll
        for (int u = 0; u < SCAN; ++u) {
            bool live = !(sc.v[u] < 0.0f);
            if (ARGMAX_ONLY && live) {
                const int slot = sc.pos + u * 64 + l;
                const int g = slot / rows, r = slot - g * rows;
                bool hit = false;
#pragma unroll
                for (int o = 0; o < NH; ++o) hit |= W.arg[g][o] == r;
                live = hit;
            }
            const unsigned long long mask = __ballot(live);
            const int before = __popcll(mask & ((1ull << l) - 1ull));
            if (live) W.ring[(sc.head + sc.cnt + before) & (RING - 1)] = sc.pos + u * 64 + l;
            sc.cnt += __popcll(mask);
        }
        sc.pos += SCAN * 64;
        scan_fetch(sc, fchunk, limit, nf, l);
    }
    wave_fence();
    take = sc.cnt < 32 ? sc.cnt : 32;
    const int c = l & 31;
    const int slot = c < take ? W.ring[(sc.head + c) & (RING - 1)] : -1;
    sc.head = (sc.head + take) & (RING - 1);
    sc.cnt -= take;
    wave_fence();
    return slot;
}

// A tile's feature rows: the lane's 8 elements of the [32][16] image (columns nf..15 and dead columns are 0),
// fetched one tile ahead
struct Rows {
    float v[8];
};

__device__ __forceinline__ Rows fetch_rows(const float *fchunk, int slot, int nf, int l) {
    Rows r;
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int idx = it * 64 + l;
        const int col = idx >> 4, k = idx & 15;
        const int sl = __shfl(slot, col, 64);
        r.v[it] = (sl >= 0 && k < nf) ? fchunk[size_t(sl) * size_t(nf) + k] : 0.0f;
    }
    return r;
}

__device__ __forceinline__ void store_rows(WaveLds &W, const Rows &r, int l) {
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int idx = it * 64 + l;
        W.xs[idx >> 4][idx & 15] = r.v[it];
    }
}

template <int S, bool BWD>
__global__ __launch_bounds__(QT_BLOCK, 1) void astro_qtrain_kernel(
    const float *__restrict__ wts, int nout, const float *__restrict__ features, int n, int rows,
    float *__restrict__ q_out, float *__restrict__ qmax_out, const int8_t *__restrict__ action,
    const float *__restrict__ target, float inv_n, float *__restrict__ loss_out, float *__restrict__ partials,
    int nparams, int nchunks) {
    constexpr int NF = 5 + 5 * S;
    constexpr int KS0 = (NF + 1) / 2;      // f0's k-steps
    __shared__ float s_w0[NH][XLD];        // f0.weight, columns NF..15 zero
    __shared__ float s_b[6][NH];           // f0, f.0, f.1, v.0, v.1, v0 biases (v0's padded with 0)
    __shared__ float s_w[5][NH * LD];      // f.0, f.1, v.0, v.1, v0 (rows nout.. zero) as [out][LD] images
    __shared__ WaveLds s_wave[QT_WAVES];

    const int t = threadIdx.x;
    const int l = t & 63, wv = t >> 6;
    const int c = l & 31, h = l >> 5;

    {
        const float *w = wts;
        for (int k = t; k < NH * 16; k += QT_BLOCK) s_w0[k >> 4][k & 15] = (k & 15) < NF ? w[(k >> 4) * NF + (k & 15)] : 0.0f;
        w += NH * NF;
        for (int k = t; k < NH; k += QT_BLOCK) s_b[0][k] = w[k];
        w += NH;
        for (int L = 0; L < 4; ++L) {
            for (int k = t; k < NH * NH; k += QT_BLOCK) s_w[L][(k >> 5) * LD + (k & 31)] = w[k];
            w += NH * NH;
            for (int k = t; k < NH; k += QT_BLOCK) s_b[1 + L][k] = w[k];
            w += NH;
        }
        for (int k = t; k < NH * NH; k += QT_BLOCK) s_w[4][(k >> 5) * LD + (k & 31)] = (k >> 5) < nout ? w[k] : 0.0f;
        w += nout * NH;
        for (int k = t; k < NH; k += QT_BLOCK) s_b[5][k] = k < nout ? w[k] : 0.0f;
    }
    __syncthreads();

    WaveLds &W = s_wave[wv];
    f32x16 dW[6];
    float db[6];
    if (BWD) {
#pragma unroll
        for (int L = 0; L < 6; ++L) {
            db[L] = 0.0f;
#pragma unroll
            for (int j = 0; j < 16; ++j) dW[L][j] = 0.0f;
        }
    }

    // f0 on the tile's feature image W.xs
    auto f0_fwd = [&]() {
        f32x16 acc = bias_of(s_b[0], h);
#pragma unroll
        for (int kk = 0; kk < KS0; ++kk)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(s_w0[c][2 * kk + h], W.xs[c][2 * kk + h], acc, 0, 0, 0);
        return acc;
    };

    for (int chunk = blockIdx.x * QT_WAVES + wv; chunk < nchunks; chunk += gridDim.x * QT_WAVES) {
        const int s0 = chunk * SEGS;
        const int ns = n - s0 < SEGS ? n - s0 : SEGS;
        const int limit = ns * rows;
        const float *fchunk = features + size_t(s0) * size_t(rows) * size_t(NF);

        for (int k = l; k < SEGS * LD; k += 64) {
            (&W.pool[0][0])[k] = 0.0f;
            (&W.arg[0][0])[k] = -1;
        }
        wave_fence();

        // ---- 1: forward over the live rows, max and argmax per (sample, unit) ----
        {
            Scan sc = scan_begin(fchunk, limit, NF, l);
            int cur = -1, ar = -1;
            float m = 0.0f;
            int take;
            int slot_next = next_tile<false>(W, sc, fchunk, limit, NF, rows, l, take);
            Rows rows_next = fetch_rows(fchunk, slot_next, NF, l);
            while (take) {
                const int slot = slot_next;
                const int g = slot >= 0 ? slot / rows : -1;
                const int r = slot >= 0 ? slot - g * rows : -1;
                store_rows(W, rows_next, l);
                slot_next = next_tile<false>(W, sc, fchunk, limit, NF, rows, l, take);
                rows_next = fetch_rows(fchunk, slot_next, NF, l);
                wave_fence();
                f32x16 acc = f0_fwd();
                f32x16 x;
#pragma unroll
                for (int j = 0; j < 16; ++j) x[j] = acc[j] * ss_rcp(acc[j]);
                acc = layer_fwd(s_w[0], x, bias_of(s_b[1], h), c, h);
#pragma unroll
                for (int j = 0; j < 16; ++j) x[j] = acc[j] * ss_rcp(acc[j]);
                acc = layer_fwd(s_w[1], x, bias_of(s_b[2], h), c, h);
                put_tile(W.td, acc, c, h);
                wave_fence();
                // every lane walks the tile's columns for unit c (both halves alike);
                // a finished sample's result is stored, the last one's carries on
                float v[32];
#pragma unroll
                for (int cc = 0; cc < 32; ++cc) v[cc] = W.td[cc][c];
#pragma unroll
                for (int cc = 0; cc < 32; ++cc) {
                    const int sg = __builtin_amdgcn_readlane(g, cc);
                    const int rr = __builtin_amdgcn_readlane(r, cc);
                    if (sg >= 0) {
                        if (sg != cur) {
                            if (cur >= 0) {
                                W.pool[cur][c] = m;
                                W.arg[cur][c] = ar;
                            }
                            cur = sg;
                            m = v[cc];
                            ar = rr;
                        } else if (v[cc] > m) {   // strictly: the first maximal row keeps it
                            m = v[cc];
                            ar = rr;
                        }
                    }
                }
                wave_fence();
            }
            if (cur >= 0) {
                W.pool[cur][c] = m;
                W.arg[cur][c] = ar;
            }
            wave_fence();
        }

        // ---- 2: the head on the chunk's 32 pooled vectors (column c = sample s0 + c) ----
        {
            const bool valid = c < ns;
            const size_t sid = size_t(s0) + size_t(c);
            f32x16 x, rv0, av0, rv1, av1;
#pragma unroll
            for (int j = 0; j < 16; ++j) x[j] = W.pool[c][out_of(j, h)];
            f32x16 acc = layer_fwd(s_w[2], x, bias_of(s_b[3], h), c, h);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                rv0[j] = ss_rcp(acc[j]);
                av0[j] = acc[j] * rv0[j];
            }
            acc = layer_fwd(s_w[3], av0, bias_of(s_b[4], h), c, h);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                rv1[j] = ss_rcp(acc[j]);
                av1[j] = acc[j] * rv1[j];
            }
            acc = layer_fwd(s_w[4], av1, bias_of(s_b[5], h), c, h);
            // outputs 0..3 are registers 0..3 of half 0, outputs 4, 5 registers 0, 1 of half 1
            float qv[6];
#pragma unroll
            for (int j = 0; j < 4; ++j) qv[j] = tanhf(acc[j]);
            qv[4] = __shfl_down(qv[0], 32, 64);
            qv[5] = __shfl_down(qv[1], 32, 64);
            if (!BWD) {
                if (valid && h == 0) {
                    float best = qv[0];
#pragma unroll
                    for (int o = 1; o < 6; ++o)
                        if (o < nout) best = fmaxf(best, qv[o]);
                    if (q_out) {
#pragma unroll
                        for (int o = 0; o < 6; ++o)
                            if (o < nout) q_out[sid * size_t(nout) + o] = qv[o];
                    }
                    if (qmax_out) qmax_out[sid] = best;
                }
            } else {
                float gy = 0.0f;
                int a = -1;
                if (valid && h == 0) {
                    const int av = action[sid];
                    const bool ok = av >= 0 && av < nout;
                    float y = qv[0];
#pragma unroll
                    for (int o = 1; o < 6; ++o) y = av == o ? qv[o] : y;
                    const float d = y - target[sid];
                    if (loss_out) loss_out[sid] = ok ? d * d : __builtin_nanf("");
                    if (ok) {
                        a = av;
                        gy = (2.0f * d * inv_n) * (1.0f - y * y);   // dL/dz of the chosen output (tanh' = 1 - y^2)
                    }
                }
                gy = __shfl(gy, c, 64);
                a = __shfl(a, c, 64);
                f32x16 d;
#pragma unroll
                for (int j = 0; j < 16; ++j) d[j] = out_of(j, h) == a ? gy : 0.0f;
                // v0
                put_tile(W.ta, av1, c, h);
                put_tile(W.td, d, c, h);
                wave_fence();
                accum(dW[5], db[5], W.td, W.ta, c, h);
                acc = layer_bwd(s_w[4], d, c, h);
#pragma unroll
                for (int j = 0; j < 16; ++j) d[j] = acc[j] * rv1[j] * rv1[j];
                wave_fence();
                // v.1
                put_tile(W.ta, av0, c, h);
                put_tile(W.td, d, c, h);
                wave_fence();
                accum(dW[4], db[4], W.td, W.ta, c, h);
                acc = layer_bwd(s_w[3], d, c, h);
#pragma unroll
                for (int j = 0; j < 16; ++j) d[j] = acc[j] * rv0[j] * rv0[j];
                wave_fence();
                // v.0: its input is the pooled image itself, [sample][unit]
                put_tile(W.td, d, c, h);
                wave_fence();
                accum(dW[3], db[3], W.td, W.pool, c, h);
                acc = layer_bwd(s_w[2], d, c, h);
                wave_fence();
                put_tile(W.pool, acc, c, h);   // the pooled units' gradients
            }
            wave_fence();
        }

        // ---- 3: backward over the live rows ----
        if (BWD) {
            Scan sc = scan_begin(fchunk, limit, NF, l);
            int take;
            int slot_next = next_tile<ASTRO_QTRAIN_SPARSE != 0>(W, sc, fchunk, limit, NF, rows, l, take);
            Rows rows_next = fetch_rows(fchunk, slot_next, NF, l);
            while (take) {
                const int slot = slot_next;
                const int g = slot >= 0 ? slot / rows : -1;
                const int r = slot >= 0 ? slot - g * rows : -1;
                const int gi = g < 0 ? 0 : g;
                store_rows(W, rows_next, l);
                slot_next = next_tile<ASTRO_QTRAIN_SPARSE != 0>(W, sc, fchunk, limit, NF, rows, l, take);
                rows_next = fetch_rows(fchunk, slot_next, NF, l);
                wave_fence();
                f32x16 acc = f0_fwd();
                f32x16 r0, a0, r1, a1, d;
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    r0[j] = ss_rcp(acc[j]);
                    a0[j] = acc[j] * r0[j];
                }
                acc = layer_fwd(s_w[0], a0, bias_of(s_b[1], h), c, h);
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    r1[j] = ss_rcp(acc[j]);
                    a1[j] = acc[j] * r1[j];
                }
                // f.1: dZ is the pooled unit's gradient at its argmax row
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int o = out_of(j, h);
                    d[j] = (g >= 0 && W.arg[gi][o] == r) ? W.pool[gi][o] : 0.0f;
                }
                put_tile(W.ta, a1, c, h);
                put_tile(W.td, d, c, h);
                wave_fence();
                accum(dW[2], db[2], W.td, W.ta, c, h);
                acc = layer_bwd(s_w[1], d, c, h);
#pragma unroll
                for (int j = 0; j < 16; ++j) d[j] = acc[j] * r1[j] * r1[j];
                wave_fence();
                // f.0
                put_tile(W.ta, a0, c, h);
                put_tile(W.td, d, c, h);
                wave_fence();
                accum(dW[1], db[1], W.td, W.ta, c, h);
                acc = layer_bwd(s_w[0], d, c, h);
#pragma unroll
                for (int j = 0; j < 16; ++j) d[j] = acc[j] * r0[j] * r0[j];
                wave_fence();
                // f0: its input is the feature image (lanes past its 16 columns add into unused columns)
                put_tile(W.td, d, c, h);
                wave_fence();
#pragma unroll
                for (int kk = 0; kk < 16; ++kk) {
                    const float a = W.td[2 * kk + h][c];
                    const float b = c < 16 ? W.xs[2 * kk + h][c & 15] : 0.0f;
                    dW[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, dW[0], 0, 0, 0);
                    db[0] += a;
                }
                wave_fence();
            }
        }
    }

    // ---- the wave's partial gradient, in the packed layout ----
    if (BWD) {
        float *P = partials + size_t(blockIdx.x * QT_WAVES + wv) * size_t(nparams);
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (c < NF) P[out_of(j, h) * NF + c] = dW[0][j];
        int off = NH * NF;
        const float b0 = db[0] + __shfl_xor(db[0], 32, 64);
        if (h == 0) P[off + c] = b0;
        off += NH;
#pragma unroll
        for (int L = 1; L < 5; ++L) {
#pragma unroll
            for (int j = 0; j < 16; ++j) P[off + out_of(j, h) * NH + c] = dW[L][j];
            off += NH * NH;
            const float b = db[L] + __shfl_xor(db[L], 32, 64);
            if (h == 0) P[off + c] = b;
            off += NH;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (out_of(j, h) < nout) P[off + out_of(j, h) * NH + c] = dW[5][j];
        off += nout * NH;
        const float b5 = db[5] + __shfl_xor(db[5], 32, 64);
        if (h == 0 && c < nout) P[off + c] = b5;
    }
}

// grad[k] = the partials' sum in float64, rounded once, in a fixed order: 16 threads per parameter take every
// 16th partial each in turn, then their 16 sums are added in turn.
__global__ __launch_bounds__(RED_BLOCK) void astro_qgrad_reduce_kernel(const float *__restrict__ partials, int nparts,
                                                                       int nparams, float *__restrict__ grad) {
    __shared__ double s_sum[RED_GROUPS][RED_PARAMS];
    const int kl = threadIdx.x % RED_PARAMS, grp = threadIdx.x / RED_PARAMS;
    const int k = blockIdx.x * RED_PARAMS + kl;
    double s = 0.0;
    if (k < nparams)
        for (int p = grp; p < nparts; p += RED_GROUPS) s += double(partials[size_t(p) * size_t(nparams) + k]);
    s_sum[grp][kl] = s;
    __syncthreads();
    if (grp == 0 && k < nparams) {
        double tot = 0.0;
#pragma unroll
        for (int g = 0; g < RED_GROUPS; ++g) tot += s_sum[g][kl];
        grad[k] = float(tot);
    }
}

// ---------------------------------------------------------------------------
// host side

int nparams_of(const AstroQNet &net) {
    const int nf = 5 + 5 * net.nships;
    return NH * nf + NH + 4 * (NH * NH + NH) + (NH + 1) * net.nout;
}

int blocks_of(int n) {
    const int nchunks = (n + SEGS - 1) / SEGS;
    return std::min((nchunks + QT_WAVES - 1) / QT_WAVES, MAX_BLOCKS);
}

int check_net(const AstroQNet *net) {
    if (!net) return fail(-100, "net is NULL");
    if (net->nships != 1 && net->nships != 2) return fail(-101, "net.nships must be 1 or 2, got %d", int(net->nships));
    if (net->nout < 1 || net->nout > ASTRO_QNET_MAX_OUT)
        return fail(-102, "net.nout must be in [1, %d], got %d", ASTRO_QNET_MAX_OUT, int(net->nout));
    return 0;
}

int check_shape(int32_t n, int32_t rows) {
    if (n < 0) return fail(-111, "n < 0");
    if (rows < 1 || rows > ASTRO_QTRAIN_MAX_ROWS)
        return fail(-112, "rows must be in [1, %d], got %d", ASTRO_QTRAIN_MAX_ROWS, int(rows));
    return 0;
}

template <bool BWD>
int launch(const AstroQNet &net, const float *features, int n, int rows, float *q, float *qmax, const int8_t *action,
           const float *target, float *loss, float *partials, hipStream_t stream, const char *what) {
    const int nchunks = (n + SEGS - 1) / SEGS;
    const int blocks = blocks_of(n);
    const float inv_n = 1.0f / float(n);
    const int np = nparams_of(net);
    with_nships(net.nships, [&](auto S) {
        hipLaunchKernelGGL((astro_qtrain_kernel<S(), BWD>), dim3(unsigned(blocks)), dim3(QT_BLOCK), 0, stream, net.weights,
                           int(net.nout), features, n, rows, q, qmax, action, target, inv_n, loss, partials, np, nchunks);
    });
    return launched(what);
}

}  // namespace

extern "C" {

int astro_qtrain_abi_version(void) { return ASTRO_QTRAIN_ABI_VERSION; }

const char *astro_qtrain_last_error(void) { return g_err; }

int astro_qforward(const AstroQNet *net, const float *features, int32_t n, int32_t rows, float *q, float *qmax,
                   void *stream) {
    if (int rc = check_net(net)) return rc;
    if (int rc = check_shape(n, rows)) return rc;
    if (!q && !qmax) return fail(-114, "q and qmax are both NULL");
    if (n == 0) return 0;
    if (!net->weights || !aligned(net->weights, 4)) return fail(-105, "net.weights must be a 4-byte aligned device pointer");
    if (!features) return fail(-110, "features is NULL");
    if (!aligned(features, 4) || !aligned(q, 4) || !aligned(qmax, 4))
        return fail(-119, "features, q and qmax must be 4-byte aligned");
    return launch<false>(*net, features, n, rows, q, qmax, nullptr, nullptr, nullptr, nullptr,
                         static_cast<hipStream_t>(stream), "astro_qforward");
}

size_t astro_qgrad_workspace_bytes(const AstroQNet *net, int32_t n) {
    if (!net || (net->nships != 1 && net->nships != 2) || net->nout < 1 || net->nout > ASTRO_QNET_MAX_OUT || n <= 0)
        return 0;
    return size_t(blocks_of(n)) * QT_WAVES * size_t(nparams_of(*net)) * sizeof(float);
}

int astro_qgrad(const AstroQNet *net, const float *features, int32_t n, int32_t rows, const int8_t *action,
                const float *target, float *loss, float *grad, void *workspace, size_t workspace_bytes,
                void *stream) {
    if (int rc = check_net(net)) return rc;
    if (int rc = check_shape(n, rows)) return rc;
    if (!grad) return fail(-117, "grad is NULL");
    if (!aligned(grad, 4)) return fail(-119, "grad must be 4-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int np = nparams_of(*net);
    int nparts = 0;
    if (n > 0) {
        if (!net->weights || !aligned(net->weights, 4))
            return fail(-105, "net.weights must be a 4-byte aligned device pointer");
        if (!features) return fail(-110, "features is NULL");
        if (!action) return fail(-115, "action is NULL");
        if (!target) return fail(-116, "target is NULL");
        const size_t need = astro_qgrad_workspace_bytes(net, n);
        if (!workspace || workspace_bytes < need)
            return fail(-118, "workspace of %zu bytes, astro_qgrad_workspace_bytes is %zu", workspace ? workspace_bytes : size_t(0),
                        need);
        if (!aligned(features, 4) || !aligned(target, 4) || !aligned(loss, 4))
            return fail(-119, "features, target and loss must be 4-byte aligned");
        if (!aligned(workspace, 16)) return fail(-119, "workspace must be 16-byte aligned");
        if (int rc = launch<true>(*net, features, n, rows, nullptr, nullptr, action, target, loss,
                                  static_cast<float *>(workspace), st, "astro_qgrad"))
            return rc;
        nparts = blocks_of(n) * QT_WAVES;
    }
    hipLaunchKernelGGL(astro_qgrad_reduce_kernel, dim3(unsigned((np + RED_PARAMS - 1) / RED_PARAMS)), dim3(RED_BLOCK), 0, st,
                       static_cast<const float *>(workspace), nparts, np, grad);
    return launched("astro_qgrad reduce");
}

}  // extern "C"
