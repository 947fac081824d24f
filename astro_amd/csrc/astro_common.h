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
// script.ScriptBot (script.py:13-91) on the bot's ego view (core.roll_ships:
// its own ship first), in the precision numpy evaluates it for the state's
// dtypes (NEP 50: Python-float constants take the array's dtype):
//   X -- ship positions, velocities and bearings, and ship - planet
//        positions: float32 at a game's first tick (create()'s arrays),
//        float64 after;
//   V -- ship - planet velocities: float32 only at the first tick of a
//        one-planet game (its planet's dx is float32 for ever), else float64.
// Scalar ** 2 in the reference is pow(x, 2); x * x here (they differ only
// where pow is not correctly rounded).
// D holds the bot's six constants as AstroPolicy names them (script_r2,
// script_threshold, ship_thrust, ship_rspeed, bullet_speed, ship_radius): the
// step library's TickDriver, astro_seats.hip's per-ship seat record.

__device__ __forceinline__ float np_atan2(float y, float x) { return atan2f(y, x); }
__device__ __forceinline__ double np_atan2(double y, double x) { return atan2(y, x); }

// ScriptBot._fly_to (script.py:26-35); t is a value of the angle's dtype
template <typename C>
__device__ __forceinline__ int fly_to(C target, C bearing, C t, bool fwd) {
    const C angle = np_norm_angle<C>(target - bearing);
    if (angle < -t) return 0;   // rotate left
    if (t < angle) return 4;    // rotate right
    return fwd ? 3 : 2;
}

// ScriptBot._danger (script.py:37-62) for one planet: true with the bearing
// to steer for when the course meets the inflated planet soon.  (As in the
// reference, `b` is rebound to the quadratic's linear coefficient before the
// rotation estimate uses it.)
template <typename X, typename V, typename D>
__device__ __forceinline__ bool script_danger(const D &d, X rx, X ry, V rvx, V rvy, X &steer) {
    using L = typename std::conditional<(sizeof(X) >= sizeof(V)), X, V>::type;
    const V speed = sqrt(rvx * rvx + rvy * rvy);            // util.mag(dx)
    const V den = speed + V(1e-12);                          // util.norm(dx)
    const V nx = rvx / den, ny = rvy / den;
    const L lin = L(2) * (L(nx) * L(rx) + L(ny) * L(ry));   // 2 * util.dot(norm(dx), x)
    const X mag = sqrt(rx * rx + ry * ry);
    const X c = mag * mag - X(d.script_r2);
    const L det = lin * lin - L(X(4) * c);
    if (!(L(0) < det)) return false;
    const L sq = sqrt(det);
    if (!(L(0) <= -lin + sq)) return false;
    const L distance = -lin - sq;
    const X bx = np_atan2(rx, ry);                           // util.bearing(x)
    const L rotation = fabs(np_norm_angle<L>(L(bx) - lin));
    const L reach = (L(speed / V(d.ship_thrust)) + L(d.ship_rspeed) / rotation) * L(speed);
    if (!(distance < reach)) return false;
    steer = bx;
    return true;
}

// ScriptBot.__call__ (script.py:64-91): (m*) the bot's own ship, (e*) the
// other ship (two-ship games), planets j < np
template <typename X, typename V, int S, int PMAX, typename D>
__device__ __forceinline__ int script_decide(const D &d, bool solo, int np, const double (&px)[PMAX],
                                          const double (&py)[PMAX], const double (&pdx)[PMAX],
                                          const double (&pdy)[PMAX], double mx, double my, double mdx,
                                          double mdy, double mb, double ex, double ey, double edx, double edy) {
    for (int j = 0; j < PMAX; ++j) {   // don't crash into planets (in index order)
        X steer;
        if (j < np && script_danger<X, V>(d, X(mx) - X(px[j]), X(my) - X(py[j]), V(mdx) - V(pdx[j]),
                                          V(mdy) - V(pdy[j]), steer))
            return fly_to<X>(steer, X(mb), X(d.script_threshold), true);
    }
    if (S == 1 || solo) return 2;      // no enemy to aim for
    // aim for the enemy: where it will be when a bullet gets there
    const X dx = X(ex) - X(mx), dy = X(ey) - X(my);
    const X distance = sqrt(dx * dx + dy * dy);
    const X flight = distance / X(d.bullet_speed);
    const X fx = X(ex) + flight * (X(edx) - X(mdx));
    const X fy = X(ey) + flight * (X(edy) - X(mdy));
    return fly_to<X>(np_atan2(fx - X(mx), fy - X(my)), X(mb), X(d.ship_radius) / distance, false);
}

// dtype dispatch: X float32 at tick 0, V float32 at tick 0 of a one-planet game
template <int S, int PMAX, typename D>
__device__ __forceinline__ int script_control(const D &d, bool solo, bool t0, int np,
                                              const double (&px)[PMAX], const double (&py)[PMAX],
                                              const double (&pdx)[PMAX], const double (&pdy)[PMAX], double mx,
                                              double my, double mdx, double mdy, double mb, double ex, double ey,
                                              double edx, double edy) {
    if (!t0)
        return script_decide<double, double, S, PMAX>(d, solo, np, px, py, pdx, pdy, mx, my, mdx, mdy, mb, ex, ey,
                                                      edx, edy);
    if (np == 1)
        return script_decide<float, float, S, PMAX>(d, solo, np, px, py, pdx, pdy, mx, my, mdx, mdy, mb, ex, ey,
                                                    edx, edy);
    return script_decide<float, double, S, PMAX>(d, solo, np, px, py, pdx, pdy, mx, my, mdx, mdy, mb, ex, ey,
                                                 edx, edy);
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
