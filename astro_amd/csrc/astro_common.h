// What the five libraries' sources share (astro_kernels, astro_qnet,
// astro_qtrain, astro_replay, astro_actor .hip): the device math that must
// round alike wherever a bearing or a random word is computed, the wave and
// MFMA helpers of the Q-network kernels, and the host side's error and launch
// boilerplate.  Internal: not part of the C ABI (include/), and everything
// here is in an anonymous namespace, so every library has its own g_err and
// exports nothing from this file.
#ifndef ASTRO_COMMON_H
#define ASTRO_COMMON_H

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <type_traits>

namespace {

constexpr uint32_t TICK_MASK = (1u << 22) - 1;   // hdr[0]: tick (astro_step.h)

// ---------------------------------------------------------------------------
// exact device math (every library is built with -ffp-contract=off)

// fmod(x, y) for finite x and y > 0 with |x / y| < 2^24 (float) / 2^53
// (double), exactly, in five instructions instead of ocml's fmod: q =
// trunc(x / y) is the true quotient's integer part or, when x / y rounded up
// to the next integer, one more in magnitude (the division is correctly
// rounded, so never one less); x - q y is then a multiple of y's last mantissa
// bit smaller than y in magnitude -- exactly representable -- so the fma
// returns it exactly, and the correction by +-y is an add whose exact result
// (the true remainder) is representable too.  (tests/test_host.py checks the
// argument with exact rationals.)
template <typename C>
__device__ __forceinline__ C exact_fmod(C x, C y) {
    const C q = trunc(x / y);
    C r = __builtin_fma(-q, y, x);
    r = x >= C(0) ? (r < C(0) ? r + y : r) : (r > C(0) ? r - y : r);
    return r;
}
__device__ __forceinline__ float exact_fmod(float x, float y) {
    const float q = truncf(x / y);
    float r = __builtin_fmaf(-q, y, x);
    r = x >= 0.0f ? (r < 0.0f ? r + y : r) : (r > 0.0f ? r - y : r);
    return r;
}

// util.norm_angle (util.py:125-132): ((b + pi) % (2 pi)) - pi with numpy's
// floored remainder (npy_divmod: fmod, + divisor when the signs differ, +0
// for a zero result), in C
template <typename C>
__device__ __forceinline__ C np_norm_angle(C b) {
    const C pi = C(3.141592653589793);          // np.pi (float32: 3.1415927f)
    const C two_pi = C(6.283185307179586);      // 2 * np.pi
    const C x = b + pi;
    // (|x| < 2^24 * 2 pi: bearings change by at most dt * ship_rspeed per tick)
    C m = exact_fmod(x, two_pi);
    m = m != C(0) ? (m < C(0) ? m + two_pi : m) : C(0);
    return m - pi;
}

// the bearing feature, util.norm_angle(b) / pi
template <typename C>
__device__ __forceinline__ C norm_angle_over_pi(C b) {
    return np_norm_angle<C>(b) / C(3.141592653589793);
}

// ---------------------------------------------------------------------------
// the random word behind every random decision: splitmix64 of
// id * 0x9E37... + (draw + 1) * 0xD1B5... + seed

__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the part of the word's argument that a whole launch shares (hoisted to the host where a launch has one draw)
__host__ __device__ inline uint64_t draw_mix(uint64_t draw, uint64_t seed) {
    return (draw + 1) * 0xD1B54A32D192ED03ull + seed;
}

// the word's state before the finaliser (adding 2^63 to it gives the word of id + 2^63: the multiplier is odd)
__device__ __forceinline__ uint64_t random_state(uint64_t id, uint64_t drawmix) {
    return id * 0x9E3779B97F4A7C15ull + drawmix;
}
__device__ __forceinline__ uint64_t random_word(uint64_t id, uint64_t drawmix) {
    return splitmix64(random_state(id, drawmix));
}
__device__ __forceinline__ uint64_t random_word(uint64_t id, int64_t draw, uint64_t seed) {
    return random_word(id, draw_mix(uint64_t(draw), seed));
}

// ---------------------------------------------------------------------------
// wave and MFMA helpers

// A wave's own LDS traffic in order: every lane's writes before any lane's
// later reads (LDS runs a wave's instructions in issue order; this keeps the
// compiler from reordering around it).  No s_barrier: the waves of a
// workgroup do not wait for each other.
__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}

// The D operand of v_mfma_f32_32x32x2_f32: register j of lane half h holds
// output (unit) out_of(j, h)
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ constexpr int out_of(int j, int h) { return (j & 3) + 8 * (j >> 2) + 4 * h; }

__device__ __forceinline__ f32x16 bias_of(const float *b, int h) {
    f32x16 a;
#pragma unroll
    for (int j = 0; j < 16; ++j) a[j] = b[out_of(j, h)];
    return a;
}

// ---------------------------------------------------------------------------
// host side

thread_local char g_err[512] = "";   // astro_*_last_error() of the library that includes this

int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

inline bool aligned(const void *ptr, unsigned a) { return (reinterpret_cast<uintptr_t>(ptr) & (a - 1)) == 0; }

// after a launch (or several on one stream): 0, or the launch error as the library's last error
inline int launched(const char *what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(-1000 - int(e), "%s launch: %s", what, hipGetErrorString(e));
    return 0;
}

inline unsigned blocks_for(int64_t n, int per) { return unsigned((n + per - 1) / per); }

// f(std::integral_constant<int, nships>) for nships 1 or 2 (checked by the
// caller): a kernel template's launch is written once, with S() as its argument
template <typename F>
inline void with_nships(int nships, F &&f) {
    if (nships == 1)
        f(std::integral_constant<int, 1>{});
    else
        f(std::integral_constant<int, 2>{});
}

}  // namespace

#endif
