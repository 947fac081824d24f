// libastro_es.so: an antithetic evolution strategy on a packed parameter
// buffer (include/astro_es.h).
//
// perturb   one lane per (pair, parameter): one random word, one multiply and
//           two adds, two coalesced stores (the pair's + row and its - row).
//           grid.y is the pair, grid.x walks the parameters.
// score     one workgroup of 256 lanes per member.  A member's envs are one
//           contiguous run of winner bytes and tick words ([N][G] row-major),
//           which the lanes walk with stride 256; the four integer sums (W, L,
//           D int32, lost int64) are folded inside each wave with shuffles and
//           across the four waves through LDS, and lane 0 evaluates the fitness
//           in float64.  Integer sums: any order gives the same bits.
// gradient  one lane per parameter, 256 a workgroup.  Every workgroup first
//           derives the utilities itself from the K <= 1024 fitness values in
//           LDS (K / 256 values per lane, K compares each: at most 4,096
//           compares a lane, cheaper than a launch of its own), keeps the
//           pairs' float32 differences in LDS, and then walks the pairs in
//           order, regenerating each pair's noise for its parameter and adding
//           in float64.  Workgroup 0 stores the utilities.
//
// All three are launch-bound at the sizes they are made for (32 members of
// 4,934 parameters, a few thousand envs); what they buy is launches, no stored
// noise and no host round trip.  No float atomics, no inline assembly, no
// scratch.  Every float operation rounds on its own (the build's
// -ffp-contract=off; the float32 divide is correctly rounded).
#include "astro_common.h"
#include "astro_es.h"

#include <cmath>

namespace {

constexpr int WAVE = 64;
constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / WAVE;

// eps of (pair j, parameter p) for a launch's drawmix (astro_es.h, THE NOISE)
__device__ __forceinline__ float noise(uint32_t j, uint32_t p, uint64_t drawmix) {
    const uint64_t z = random_word((uint64_t(j) << 32) | uint64_t(p), drawmix);
    const int s = int(z & 0xffff) + int((z >> 16) & 0xffff) + int((z >> 32) & 0xffff) + int(z >> 48);
    return float(s - 131070) * 0x1.bb67aep-16f;
}

__global__ __launch_bounds__(BLOCK) void perturb_kernel(int nparams, float sigma, uint64_t drawmix, int first_pair,
                                                        const float *__restrict__ theta,
                                                        float *__restrict__ members) {
    const int p = blockIdx.x * BLOCK + threadIdx.x;
    const int i = blockIdx.y;
    if (p >= nparams) return;
    const float d = sigma * noise(uint32_t(first_pair + i), uint32_t(p), drawmix);
    const float x = theta[p];
    float *row = members + size_t(2 * i) * size_t(nparams);
    row[p] = x + d;
    row[size_t(nparams) + p] = x - d;
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = WAVE / 2; off >= 1; off >>= 1) v += __shfl_down(v, off, WAVE);
    return v;   // lane 0's is the wave's
}

__global__ __launch_bounds__(BLOCK) void score_kernel(const int8_t *__restrict__ winner,
                                                      const int32_t *__restrict__ ticks, int n_env, int games,
                                                      int nmembers, int ship, double draw, double survive,
                                                      int timeout_tick, int32_t *__restrict__ counts,
                                                      int64_t *__restrict__ lost_ticks, float *__restrict__ fitness) {
    __shared__ int part[WAVES][3];
    __shared__ long long part_lost[WAVES];
    const int k = blockIdx.x;
    const int64_t lo = int64_t(k) * n_env / nmembers, hi = int64_t(k + 1) * n_env / nmembers;
    const int64_t begin = lo * games, end = hi * games;   // (n_env * games fits an int32: checked by the caller)

    int w = 0, l = 0, d = 0;
    long long lost = 0;
    for (int64_t m = begin + threadIdx.x; m < end; m += BLOCK) {
        const int c = winner[m];
        if (c == ship) {
            ++w;
        } else if (c == -1) {
            ++d;
        } else if (c != -2) {
            ++l;
            const int t = ticks[m];
            lost += t < timeout_tick ? t : timeout_tick;
        }
    }
    w = wave_sum(w);
    l = wave_sum(l);
    d = wave_sum(d);
    lost = wave_sum(lost);
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    if (lane == 0) {
        part[wave][0] = w;
        part[wave][1] = l;
        part[wave][2] = d;
        part_lost[wave] = lost;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    w = l = d = 0;
    lost = 0;
    for (int v = 0; v < WAVES; ++v) {
        w += part[v][0];
        l += part[v][1];
        d += part[v][2];
        lost += part_lost[v];
    }
    if (counts) {
        counts[3 * k + 0] = w;
        counts[3 * k + 1] = l;
        counts[3 * k + 2] = d;
    }
    if (lost_ticks) lost_ticks[k] = lost;
    const int n = w + l + d;
    float f = __int_as_float(0x7fc00000);
    if (n > 0) {
        const double a = double(w - l) + draw * double(d);
        const double b = survive * (double(lost) / double(timeout_tick));
        f = float((a + b) / double(n));
    }
    fitness[k] = f;
}

template <int SHAPING>
__global__ __launch_bounds__(BLOCK) void gradient_kernel(int nparams, int pairs, float sigma, uint64_t drawmix,
                                                         const float *__restrict__ fitness,
                                                         float *__restrict__ utilities, float *__restrict__ grad) {
    __shared__ float f[ASTRO_ES_MAX_MEMBERS];
    __shared__ float u[ASTRO_ES_MAX_MEMBERS];
    __shared__ float du[ASTRO_ES_MAX_PAIRS];
    const int K = 2 * pairs;
    const int t = threadIdx.x;

    int bad = 0;
    for (int k = t; k < K; k += BLOCK) {
        const float x = fitness[k];
        f[k] = x;
        bad |= !(fabsf(x) <= 3.4028234663852886e38f);   // an infinity or a NaN
    }
    bad = __syncthreads_or(bad);   // (also: every f[] is written before it is read)
    for (int k = t; k < K; k += BLOCK) {
        float v = 0.0f;
        if (!bad) {
            if (SHAPING == ASTRO_ES_RANKS) {
                const float x = f[k];
                int less = 0, equal = 0;
                for (int j = 0; j < K; ++j) {
                    less += f[j] < x;
                    equal += f[j] == x;
                }
                v = float(2 * less + (equal - 1)) / float(2 * (K - 1)) - 0.5f;
            } else {
                v = f[k];
            }
        }
        u[k] = v;
        if (utilities && blockIdx.x == 0) utilities[k] = v;
    }
    __syncthreads();
    for (int j = t; j < pairs; j += BLOCK) du[j] = u[2 * j] - u[2 * j + 1];
    __syncthreads();

    const int p = blockIdx.x * BLOCK + t;
    if (p >= nparams) return;
    double a = 0.0;
    for (int j = 0; j < pairs; ++j) a = a + double(du[j]) * double(noise(uint32_t(j), uint32_t(p), drawmix));
    grad[p] = float(-a / ((2.0 * double(pairs)) * double(sigma)));
}

// the checks of an AstroES that perturb and gradient share
int check_es(const AstroES *es) {
    if (!es) return fail(-180, "es is NULL");
    if (es->nparams < 1 || es->nparams > ASTRO_ES_MAX_PARAMS)
        return fail(-181, "es.nparams must be in [1, %d], got %d", ASTRO_ES_MAX_PARAMS, int(es->nparams));
    if (es->pairs < 1 || es->pairs > ASTRO_ES_MAX_PAIRS)
        return fail(-182, "es.pairs must be in [1, %d], got %d", ASTRO_ES_MAX_PAIRS, int(es->pairs));
    if (!std::isfinite(es->sigma) || !(es->sigma > 0.0f))
        return fail(-183, "es.sigma must be finite and > 0, got %g", double(es->sigma));
    return 0;
}

}  // namespace

extern "C" {

int astro_es_abi_version(void) { return ASTRO_ES_ABI_VERSION; }

const char *astro_es_last_error(void) { return g_err; }

int astro_es_perturb(const AstroES *es, const float *theta, int32_t first_pair, int32_t npairs, float *members,
                     void *stream) {
    if (const int rc = check_es(es)) return rc;
    if (first_pair < 0 || npairs < 0 || int64_t(first_pair) + npairs > es->pairs)
        return fail(-184, "the pairs [%d, %d + %d) are not inside [0, %d)", int(first_pair), int(first_pair),
                    int(npairs), int(es->pairs));
    if (npairs == 0) return 0;
    if (!theta || !members) return fail(-185, "theta or members is NULL");
    const uintptr_t t0 = reinterpret_cast<uintptr_t>(theta), m0 = reinterpret_cast<uintptr_t>(members);
    const uintptr_t tn = uintptr_t(es->nparams) * sizeof(float), mn = tn * 2 * uintptr_t(npairs);
    if (m0 < t0 + tn && t0 < m0 + mn) return fail(-186, "members overlaps theta");
    if (!aligned(theta, 4) || !aligned(members, 4)) return fail(-189, "theta and members must be 4-byte aligned");

    const dim3 grid(blocks_for(es->nparams, BLOCK), unsigned(npairs)), block(BLOCK);
    hipLaunchKernelGGL(perturb_kernel, grid, block, 0, static_cast<hipStream_t>(stream), int(es->nparams), es->sigma,
                       draw_mix(uint64_t(es->generation), es->seed), int(first_pair), theta, members);
    return launched("astro_es_perturb");
}

int astro_es_score(const int8_t *winner, const int32_t *ticks, int32_t n_env, int32_t games, int32_t nmembers,
                   int32_t ship, double draw, double survive, int32_t timeout_tick, int32_t *counts,
                   int64_t *lost_ticks, float *fitness, void *stream) {
    if (n_env < 0) return fail(-3, "n_env < 0");
    if (games < 1) return fail(-187, "games must be >= 1, got %d", int(games));
    if (int64_t(n_env) * games > INT32_MAX) return fail(-187, "n_env * games does not fit an int32");
    if (nmembers < 1 || nmembers > ASTRO_ES_MAX_MEMBERS)
        return fail(-187, "nmembers must be in [1, %d], got %d", ASTRO_ES_MAX_MEMBERS, int(nmembers));
    if (timeout_tick < 1) return fail(-187, "timeout_tick must be >= 1, got %d", int(timeout_tick));
    if (ship != 0 && ship != 1) return fail(-11, "ship must be 0 or 1 (nships is 1 or 2), got %d", int(ship));
    if (!std::isfinite(draw) || !std::isfinite(survive)) return fail(-183, "draw and survive must be finite");
    if (!fitness) return fail(-185, "fitness is NULL");
    if (n_env > 0 && (!winner || !ticks)) return fail(-185, "winner or ticks is NULL");
    if (!aligned(ticks, 4) || !aligned(counts, 4) || !aligned(fitness, 4) || !aligned(lost_ticks, 8))
        return fail(-189, "ticks, counts and fitness must be 4-byte and lost_ticks 8-byte aligned");

    const dim3 grid{unsigned(nmembers)}, block(BLOCK);
    hipLaunchKernelGGL(score_kernel, grid, block, 0, static_cast<hipStream_t>(stream), winner, ticks, int(n_env),
                       int(games), int(nmembers), int(ship), draw, survive, int(timeout_tick), counts, lost_ticks,
                       fitness);
    return launched("astro_es_score");
}

int astro_es_gradient(const AstroES *es, const float *fitness, int32_t shaping, float *utilities, float *grad,
                      void *stream) {
    if (const int rc = check_es(es)) return rc;
    if (shaping != ASTRO_ES_RANKS && shaping != ASTRO_ES_RAW) return fail(-188, "shaping %d is unknown", int(shaping));
    if (!fitness || !grad) return fail(-185, "fitness or grad is NULL");
    if (!aligned(fitness, 4) || !aligned(utilities, 4) || !aligned(grad, 4))
        return fail(-189, "fitness, utilities and grad must be 4-byte aligned");

    const dim3 grid(blocks_for(es->nparams, BLOCK)), block(BLOCK);
    hipStream_t hs = static_cast<hipStream_t>(stream);
    const uint64_t drawmix = draw_mix(uint64_t(es->generation), es->seed);
    if (shaping == ASTRO_ES_RANKS)
        hipLaunchKernelGGL(gradient_kernel<ASTRO_ES_RANKS>, grid, block, 0, hs, int(es->nparams), int(es->pairs),
                           es->sigma, drawmix, fitness, utilities, grad);
    else
        hipLaunchKernelGGL(gradient_kernel<ASTRO_ES_RAW>, grid, block, 0, hs, int(es->nparams), int(es->pairs),
                           es->sigma, drawmix, fitness, utilities, grad);
    return launched("astro_es_gradient");
}

}  // extern "C"
