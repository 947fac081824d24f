// libastro_search.so: a branched step plus rollout reduced to values and a
// decision (include/astro_search.h).
//
// values  one lane per (env, control), sixty lanes of a wave in use: a wave
//         covers ten whole envs (A R is 6 or 36, neither divides 64), four
//         waves a workgroup, forty envs.  A lane owns the R branches
//         m = (i A + a) R .. + R - 1 of its control, which are consecutive, and
//         so are the lanes' runs: a wave's read of one tick row of done bytes
//         is one contiguous segment of 60 R bytes.
//           scan    tick 0 from done0, then ticks 1..K-1 from the rollout's
//                   rows; a branch takes the first non-zero byte and reads no
//                   further, and the wave leaves the loop once no lane of it
//                   has a branch pending (one ballot per tick)
//           value   per branch ONE reward load (the first done tick's, ship's
//                   column) times gamma[t*]; or six leaf loads folded with
//                   fmaxf times gamma[K]; or 0.0f.  Then the minimum over the
//                   lane's R branches in reply order, in registers.
//           pick    an env's six values sit in six neighbouring lanes of one
//                   wave: every lane reads them with six wave shuffles (no LDS
//                   allocation, no barrier), folds the first maximum and the
//                   own control's value, and the env's lane a = 0 stores the
//                   control.
//         What the kernel removes is launches (ten and more elementwise ones
//         per search tick), not bytes: at search sizes the inputs are a few MB
//         and mostly not even read, thanks to the early exit.  Nothing here is
//         tuned for bandwidth.
//
// No LDS, no atomics, no inline assembly, no scratch (first[] is indexed by
// unrolled constants only).
#include "astro_common.h"
#include "astro_search.h"

namespace {

constexpr int A = ASTRO_SEARCH_NCONTROL;
constexpr int WAVE = 64;
constexpr int ENVS_PER_WAVE = WAVE / A;          // 10
constexpr int USED = ENVS_PER_WAVE * A;          // 60 lanes
constexpr int BLOCK = 256;
constexpr int ENVS_PER_BLOCK = (BLOCK / WAVE) * ENVS_PER_WAVE;

template <int R>
__global__ __launch_bounds__(BLOCK) void values_kernel(AstroSearch s, float *__restrict__ value,
                                                       const int8_t *__restrict__ own, int8_t *__restrict__ control,
                                                       int32_t *__restrict__ first_out) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = blockIdx.x * (BLOCK / WAVE) + (threadIdx.x / WAVE);
    const int a = lane % A;
    const int i = wave * ENVS_PER_WAVE + lane / A;
    // (idle lanes stay in the wave: the ballot and the shuffles below are the whole wave's)
    const bool valid = lane < USED && i < s.n_env;
    const int S = s.nships, K = s.horizon;
    const size_t M = size_t(s.n_env) * A * R;
    const size_t m0 = (size_t(valid ? i : 0) * A + a) * R;   // the lane's first branch

    int first[R];
    bool pending = false;
#pragma unroll
    for (int o = 0; o < R; ++o) {
        first[o] = (valid && s.done0[m0 + o] != 0) ? 0 : -1;
        pending |= valid && first[o] < 0;
    }
    for (int t = 1; t < K; ++t) {
        if (!__any(pending)) break;
        const uint8_t *row = s.done + size_t(t - 1) * M + m0;
        pending = false;
#pragma unroll
        for (int o = 0; o < R; ++o) {
            if (valid && first[o] < 0) {
                if (row[o] != 0)
                    first[o] = t;
                else
                    pending = true;
            }
        }
    }

    float v = 0.0f;
    if (valid) {
#pragma unroll
        for (int o = 0; o < R; ++o) {
            const size_t m = m0 + o;
            const int t = first[o];
            float b = 0.0f;
            if (t == 0) {
                b = s.gamma[0] * s.reward0[m * S + s.ship];
            } else if (t > 0) {
                b = s.gamma[t] * s.reward[(size_t(t - 1) * M + m) * S + s.ship];
            } else if (s.leaf) {
                const float *q = s.leaf + (m * S + s.ship) * A;
                float best = q[0];
#pragma unroll
                for (int k = 1; k < A; ++k) best = fmaxf(best, q[k]);
                b = s.gamma[K] * best;
            }
            if (o == 0 || b < v) v = b;
            if (first_out) first_out[m] = t;
        }
        value[size_t(i) * A + a] = v;
    }
    if (!control) return;

    // the env's six values, from its six lanes
    const int base = lane - a;
    const int mine = valid ? int(own[i]) : 0;
    float best = 0.0f, held = 0.0f;
    int arg = 0;
#pragma unroll
    for (int k = 0; k < A; ++k) {
        const float vk = __shfl(v, base + k, WAVE);
        if (k == 0 || vk > best) {
            best = vk;
            arg = k;
        }
        if (k == mine) held = vk;
    }
    if (valid && a == 0) {
        const bool keep = mine >= 0 && mine < A && !(best > held);
        control[i] = int8_t(keep ? mine : arg);
    }
}

}  // namespace

extern "C" {

int astro_search_abi_version(void) { return ASTRO_SEARCH_ABI_VERSION; }

const char *astro_search_last_error(void) { return g_err; }

int astro_search_values(const AstroSearch *s, float *value, const int8_t *own, int8_t *control, int32_t *first,
                        void *stream) {
    if (!s) return fail(-170, "s is NULL");
    if (s->n_env < 0) return fail(-3, "n_env < 0");
    if (s->nships != 1 && s->nships != 2) return fail(-11, "nships must be 1 or 2, got %d", int(s->nships));
    if (s->ship < 0 || s->ship >= s->nships)
        return fail(-171, "ship must be in [0, %d), got %d", int(s->nships), int(s->ship));
    if (s->horizon < 1) return fail(-172, "horizon must be >= 1, got %d", int(s->horizon));
    if (s->replies != 1 && s->replies != A) return fail(-173, "replies must be 1 or 6, got %d", int(s->replies));
    if (int64_t(s->n_env) * A * s->replies * s->nships * A > INT32_MAX)
        return fail(-174, "n_env * 6 * replies * nships * 6 does not fit an int32");
    if (!value) return fail(-175, "value is NULL");
    if (control && !own) return fail(-176, "control is given without own");
    if (s->n_env == 0) return 0;
    if (!s->reward0 || !s->done0 || !s->gamma) return fail(-177, "reward0, done0 or gamma is NULL");
    if (s->horizon > 1 && (!s->reward || !s->done)) return fail(-178, "reward or done is NULL with horizon > 1");
    if (!aligned(s->reward0, 4) || !aligned(s->reward, 4) || !aligned(s->gamma, 4) || !aligned(s->leaf, 4) ||
        !aligned(value, 4) || !aligned(first, 4))
        return fail(-179, "the float and int32 arrays must be 4-byte aligned");

    hipStream_t hs = static_cast<hipStream_t>(stream);
    const dim3 grid(blocks_for(s->n_env, ENVS_PER_BLOCK)), block(BLOCK);
    if (s->replies == 1)
        hipLaunchKernelGGL(values_kernel<1>, grid, block, 0, hs, *s, value, own, control, first);
    else
        hipLaunchKernelGGL(values_kernel<A>, grid, block, 0, hs, *s, value, own, control, first);
    return launched("astro_search_values");
}

}  // extern "C"
