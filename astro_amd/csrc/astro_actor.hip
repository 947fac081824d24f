// libastro_actor.so: the acting side of rl.py's trainer around astro_step
// (include/astro_actor.h).
//
// explore   one lane per ship: the env's tick from the header, one splitmix64
//           word for the transition and a second one only for the lane that
//           enters, integer compares, one int8 load and store of the policy and
//           a store of the control where a policy is held.  Neighbouring lanes
//           touch neighbouring bytes.
//
// episodes  one lane per env: the env's counters are private to its lane, so
//           plain loads and stores serve and no atomic is needed.  Most lanes
//           (no game ended) store one int32.
//
// Both move well under 1 MB at 65,536 envs and are bound by the launch.
#include "astro_actor.h"
#include "astro_common.h"

namespace {

constexpr int BLOCK = 256;

template <int S>
__global__ __launch_bounds__(BLOCK) void explore_kernel(const int32_t *__restrict__ hdr, int8_t *__restrict__ policy,
                                                        int8_t *__restrict__ control, int n_ships, uint64_t stay_out,
                                                        uint64_t stay_in, uint64_t id0, uint64_t drawmix,
                                                        uint32_t nrandom) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;   // env * S + ship
    if (i >= n_ships) return;
    const int env = i / S;
    int pol = policy[i];
    const uint32_t tick = uint32_t(hdr[4 * size_t(env)]) & TICK_MASK;
    if (tick != 0) {
        const uint64_t g = random_state(id0 + uint64_t(i), drawmix);
        const uint64_t k = splitmix64(g) >> 11;
        if (pol < 0) {
            if (k >= stay_out) {
                const uint64_t w = splitmix64(g + (1ull << 63));   // the word of id + 2^63
                pol = int(((w >> 32) * uint64_t(nrandom)) >> 32);
                policy[i] = int8_t(pol);
            }
        } else if (k >= stay_in) {
            pol = -1;
            policy[i] = int8_t(-1);
        }
    }
    if (pol >= 0) control[i] = int8_t(pol);
}

template <int S>
__global__ __launch_bounds__(BLOCK) void episodes_kernel(AstroEpisodes ep, const float *__restrict__ reward,
                                                         const uint8_t *__restrict__ done) {
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= ep.n_env) return;
    const int len = ep.length[e] + 1;
    if (done[e] == 0) {
        ep.length[e] = len;
        return;
    }
    float mx = reward[size_t(e) * S];
    int w = 0;
#pragma unroll
    for (int s = 1; s < S; ++s) {
        const float r = reward[size_t(e) * S + s];
        if (r > mx) {   // the first maximal ship
            mx = r;
            w = s;
        }
    }
    if (!(mx >= 1.0f)) w = -1;
    const int g = ep.got[e];
    if (uint32_t(g) < uint32_t(ep.games)) {   // (a negative got, written by the caller, records nothing)
        ep.winner[size_t(e) * ep.games + g] = int8_t(w);
        ep.ticks[size_t(e) * ep.games + g] = len;
    }
    if (w >= 0) ep.wins[size_t(e) * S + w] += 1;
    ep.finished[e] += 1;
    ep.tick_sum[e] += len;
    ep.got[e] = g + 1;
    ep.length[e] = 0;
}

}  // namespace

extern "C" {

int astro_actor_abi_version(void) { return ASTRO_ACTOR_ABI_VERSION; }

const char *astro_actor_last_error(void) { return g_err; }

int astro_explore(const AstroParams *p, const AstroState *s, const AstroExplore *ex, int64_t draw, int8_t *control,
                  void *stream) {
    if (!p || !s || !ex) return fail(-100, "p, s or ex is NULL");
    if (p->nships != 1 && p->nships != 2) return fail(-101, "p.nships must be 1 or 2, got %d", int(p->nships));
    if (s->n_env < 1) return fail(-102, "s.n_env must be >= 1, got %d", int(s->n_env));
    if (ex->nrandom < 1 || ex->nrandom > ASTRO_EXPLORE_MAX_RANDOM)
        return fail(-103, "ex.nrandom must be in [1, %d], got %d", ASTRO_EXPLORE_MAX_RANDOM, int(ex->nrandom));
    if (ex->stay_out > ASTRO_EXPLORE_ONE || ex->stay_in > ASTRO_EXPLORE_ONE)
        return fail(-104, "ex.stay_out and ex.stay_in must be <= 2^53");
    const int64_t n = int64_t(s->n_env) * p->nships;
    if (n > INT32_MAX) return fail(-106, "n_env * nships = %lld does not fit an int32", (long long)n);
    if (!s->hdr || !ex->policy) return fail(-108, "s.hdr and ex.policy must not be NULL");
    if (!aligned(s->hdr, 16)) return fail(-109, "s.hdr must be 16-byte aligned");
    if (!control) return fail(-112, "control is NULL");
    const uint64_t id0 = uint64_t(ex->env_offset) * uint64_t(p->nships);
    const uint64_t drawmix = draw_mix(uint64_t(draw), ex->seed);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(blocks_for(n, BLOCK)), block(BLOCK);
    with_nships(p->nships, [&](auto S) {
        hipLaunchKernelGGL(explore_kernel<S()>, grid, block, 0, st, s->hdr, ex->policy, control, int(n), ex->stay_out,
                           ex->stay_in, id0, drawmix, uint32_t(ex->nrandom));
    });
    return launched("astro_explore");
}

int astro_episodes(const AstroEpisodes *ep, const float *reward, const uint8_t *done, void *stream) {
    if (!ep) return fail(-100, "ep is NULL");
    if (ep->nships != 1 && ep->nships != 2) return fail(-101, "ep.nships must be 1 or 2, got %d", int(ep->nships));
    if (ep->n_env < 1) return fail(-102, "ep.n_env must be >= 1, got %d", int(ep->n_env));
    if (ep->games < 1) return fail(-105, "ep.games must be >= 1, got %d", int(ep->games));
    if (int64_t(ep->n_env) * ep->games > INT32_MAX || int64_t(ep->n_env) * ep->nships > INT32_MAX)
        return fail(-106, "n_env * games = %lld does not fit an int32", (long long)(int64_t(ep->n_env) * ep->games));
    if (!ep->length || !ep->got || !ep->winner || !ep->ticks || !ep->wins || !ep->finished || !ep->tick_sum)
        return fail(-108, "ep.length, got, winner, ticks, wins, finished and tick_sum must not be NULL");
    if (!aligned(ep->length, 4) || !aligned(ep->got, 4) || !aligned(ep->ticks, 4) || !aligned(ep->wins, 4) ||
        !aligned(ep->finished, 4) || !aligned(ep->tick_sum, 8))
        return fail(-109, "an array of ep is not aligned to its element size");
    if (!reward || !done) return fail(-112, "reward or done is NULL");
    if (!aligned(reward, 4)) return fail(-119, "reward must be 4-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(blocks_for(ep->n_env, BLOCK)), block(BLOCK);
    with_nships(ep->nships, [&](auto S) {
        hipLaunchKernelGGL(episodes_kernel<S()>, grid, block, 0, st, *ep, reward, done);
    });
    return launched("astro_episodes");
}

}  // extern "C"
