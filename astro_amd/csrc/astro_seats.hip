// libastro_seats.so: astro_controls (csrc/astro_kernels.hip) with a table of
// seats, each a bot -- and a ScriptBot's own arguments -- playing one ship of a
// block of envs (include/astro_seats.h).
//
// The bot is csrc/astro_common.h's script_control, the one the step library
// runs, on the same float64 copies of the same loads; the random bot's word is
// astro_common.h's random_word of the same (global ship id, tick, seed).  A
// decision depends on its env's state and its seat's constants only, so where
// the launch begins changes nothing: every covered (ship, env) gets
// astro_controls' byte, bit for bit.  What is this kernel's own: one lane per
// env of [e0, e1), the envs between the lowest lo and the highest hi of the
// live seats (a bot, at least one env).  A lane scans the live seats -- the
// table reaches the kernel by value, at most 64 entries of 32 bytes, and the
// loop and every table read are wave-uniform; only the compare with the lane's
// env and the selects that follow are per lane -- and keeps, per ship, the bot
// and the two script arguments of the seat that holds its env.  A lane without
// a seat returns before any load.  There is no communication between lanes, no
// LDS, no atomic.
#include "astro_common.h"
#include "astro_seats.h"

namespace {

constexpr int BLOCK = 64;
constexpr int MAX_SEATS = ASTRO_SEATS_MAX;

struct alignas(16) F4 { float x, y, z, w; };
struct alignas(16) D4 { double x, y, z, w; };
template <typename T> struct Store;
template <> struct Store<float> { using V = F4; };
template <> struct Store<double> { using V = D4; };

// The live seats, by value (checked on the host: 0 <= ship < nships,
// 0 <= lo < hi <= n_env, bot one of astro_step.h's codes)
struct Table {
    double r2[MAX_SEATS], threshold[MAX_SEATS];
    int32_t ship[MAX_SEATS], bot[MAX_SEATS], lo[MAX_SEATS], hi[MAX_SEATS];
    int32_t n;   // 1 .. MAX_SEATS
    int32_t e0, e1;   // the launch's envs: min lo, max hi
};

// What script_control reads of its first argument: one ship's seat
struct SeatConsts {
    double script_r2, script_threshold, ship_thrust, ship_rspeed, bullet_speed, ship_radius;
};

// base's part of a launch
struct Base {
    uint64_t seed;
    int64_t tick0, env_offset;
    double ship_thrust, ship_rspeed, bullet_speed, ship_radius;
};

template <typename T, int S, int PMAX>
__global__ __launch_bounds__(BLOCK) void astro_seats_kernel(AstroParams p, AstroState st, Base base, Table tab,
                                                            int8_t *__restrict__ out) {
    using V = typename Store<T>::V;
    const int i = tab.e0 + int(blockIdx.x) * BLOCK + int(threadIdx.x);
    if (i >= tab.e1) return;

    int bot[S];
    SeatConsts seat[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        bot[s] = -1;
        seat[s] = SeatConsts{0.0, 0.0, base.ship_thrust, base.ship_rspeed, base.bullet_speed, base.ship_radius};
    }
    for (int k = 0; k < tab.n; ++k) {   // wave-uniform: k, and all of tab[k]
        const bool mine = tab.lo[k] <= i && i < tab.hi[k];
#pragma unroll
        for (int s = 0; s < S; ++s)
            if ((S == 1 || tab.ship[k] == s) && mine) {
                bot[s] = tab.bot[k];
                seat[s].script_r2 = tab.r2[k];
                seat[s].script_threshold = tab.threshold[k];
            }
    }
    bool any = false;
#pragma unroll
    for (int s = 0; s < S; ++s) any = any || bot[s] >= 0;
    if (!any) return;

    // the state, as astro_controls_kernel loads it
    const size_t NN = size_t(st.n_env);
    const int4 h = reinterpret_cast<const int4 *>(st.hdr)[i];
    const int tick = int(uint32_t(h.x) & TICK_MASK);
    int np = h.y & 0xff;
    np = np < 1 ? 1 : (np > PMAX ? PMAX : np);
    double sx[S], sy[S], sdx[S], sdy[S], sb[S], px[PMAX], py[PMAX], pdx[PMAX], pdy[PMAX];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const V v = reinterpret_cast<const V *>(st.ships)[size_t(s) * NN + i];
        sx[s] = double(v.x);
        sy[s] = double(v.y);
        sdx[s] = double(v.z);
        sdy[s] = double(v.w);
        sb[s] = double(reinterpret_cast<const T *>(st.ships_b)[size_t(s) * NN + i]);
    }
#pragma unroll
    for (int j = 0; j < PMAX; ++j) {
        const V v = reinterpret_cast<const V *>(st.planets)[size_t(j < p.p_pad ? j : 0) * NN + i];
        px[j] = double(v.x);
        py[j] = double(v.y);
        pdx[j] = double(v.z);
        pdy[j] = double(v.w);
    }
#pragma unroll
    for (int s = 0; s < S; ++s) {
        if (bot[s] < 0) continue;
        int c = 2;   // script.NothingBot
        if (bot[s] == ASTRO_BOT_RANDOM) {   // tick_control's draw (csrc/astro_kernels.hip)
            const uint64_t id = uint64_t(base.env_offset + i) * uint64_t(S) + uint64_t(s);
            const uint64_t z = random_word(id, base.tick0, base.seed);
            c = int(((z >> 32) * 6ull) >> 32);
        }
        const int o = S - 1 - s;
        if (bot[s] == ASTRO_BOT_SCRIPT)
            c = script_control<S, PMAX>(seat[s], p.solo != 0, tick == 0, np, px, py, pdx, pdy, sx[s], sy[s], sdx[s],
                                        sdy[s], sb[s], sx[o], sy[o], sdx[o], sdy[o]);
        out[size_t(i) * S + s] = int8_t(c);
    }
}

// ---------------------------------------------------------------------------
// host side

template <typename T, int S, int PM>
int launch(const AstroParams &p, const AstroState &s, const Base &base, const Table &tab, int8_t *out,
           hipStream_t stream) {
    hipLaunchKernelGGL((astro_seats_kernel<T, S, PM>), dim3(blocks_for(int64_t(tab.e1) - tab.e0, BLOCK)), dim3(BLOCK),
                       0, stream, p, s, base, tab, out);
    return launched("astro_controls_seats");
}

// the step library's dispatch: (storage type, ships, planet register capacity)
int dispatch(const AstroParams &p, const AstroState &s, const Base &base, const Table &tab, int8_t *out,
             hipStream_t stream) {
    const int pm = p.p_pad <= 4 ? 4 : (p.p_pad <= 8 ? 8 : 16);
#define ASTRO_CASE(T, S, PM) \
    if (std::is_same<T, double>::value == bool(s.state_f64) && p.nships == S && pm == PM) \
        return launch<T, S, PM>(p, s, base, tab, out, stream);
    ASTRO_CASE(float, 1, 4) ASTRO_CASE(float, 1, 8) ASTRO_CASE(float, 1, 16)
    ASTRO_CASE(float, 2, 4) ASTRO_CASE(float, 2, 8) ASTRO_CASE(float, 2, 16)
    ASTRO_CASE(double, 1, 4) ASTRO_CASE(double, 1, 8) ASTRO_CASE(double, 1, 16)
    ASTRO_CASE(double, 2, 4) ASTRO_CASE(double, 2, 8) ASTRO_CASE(double, 2, 16)
#undef ASTRO_CASE
    return fail(-20, "no kernel instance for this configuration");
}

}  // namespace

extern "C" {

int astro_seats_abi_version(void) { return ASTRO_SEATS_ABI_VERSION; }

const char *astro_seats_last_error(void) { return g_err; }

int astro_controls_seats(const AstroParams *p, const AstroState *s, const AstroPolicy *base, const AstroSeat *seats,
                         int32_t nseats, int8_t *control, void *stream) {
    if (!p) return fail(-10, "params is NULL");
    if (!s) return fail(-2, "state is NULL");
    if (!base) return fail(-140, "base is NULL");
    if (!seats) return fail(-141, "seats is NULL");
    if (p->nships != 1 && p->nships != 2) return fail(-11, "nships must be 1 or 2");
    if (p->p_pad < 1 || p->p_pad > 16) return fail(-13, "p_pad must be in [1, 16]");
    if (p->b_cap < 1 || p->b_cap > 65535) return fail(-15, "b_cap must be in [1, 65535]");
    if (nseats < 1 || nseats > MAX_SEATS) return fail(-142, "nseats must be in [1, %d], got %d", MAX_SEATS, int(nseats));
    if (s->n_env < 0) return fail(-3, "n_env < 0");
    for (int k = 0; k < nseats; ++k)
        if (seats[k].ship < 0 || seats[k].ship >= p->nships)
            return fail(-143, "seats[%d].ship must be in [0, %d), got %d", k, int(p->nships), int(seats[k].ship));
    for (int k = 0; k < nseats; ++k)
        if (seats[k].bot != -1 && seats[k].bot != ASTRO_BOT_NOTHING && seats[k].bot != ASTRO_BOT_SCRIPT &&
            seats[k].bot != ASTRO_BOT_RANDOM)
            return fail(-144, "seats[%d].bot must be -1, 0 (nothing), 1 (script) or 2 (random), got %d", k,
                        int(seats[k].bot));
    for (int k = 0; k < nseats; ++k)
        if (seats[k].lo < 0 || seats[k].lo > seats[k].hi || seats[k].hi > s->n_env)
            return fail(-145, "seats[%d] must have 0 <= lo <= hi <= n_env (%d), got [%d, %d)", k, int(s->n_env),
                        int(seats[k].lo), int(seats[k].hi));
    for (int a = 0; a < nseats; ++a)
        for (int b = a + 1; b < nseats; ++b)
            if (seats[a].ship == seats[b].ship && seats[a].lo < seats[a].hi && seats[b].lo < seats[b].hi &&
                seats[a].lo < seats[b].hi && seats[b].lo < seats[a].hi)
                return fail(-146, "seats[%d] and seats[%d] of ship %d overlap", a, b, int(seats[a].ship));
    if (!control) return fail(-147, "control is NULL");

    Table tab{};
    for (int k = 0; k < nseats; ++k) {
        const AstroSeat &seat = seats[k];
        if (seat.bot < 0 || seat.lo >= seat.hi) continue;
        const int n = tab.n++;
        tab.ship[n] = seat.ship;
        tab.bot[n] = seat.bot;
        tab.lo[n] = seat.lo;
        tab.hi[n] = seat.hi;
        tab.r2[n] = seat.script_r2;
        tab.threshold[n] = seat.script_threshold;
        tab.e0 = n == 0 || seat.lo < tab.e0 ? seat.lo : tab.e0;
        tab.e1 = n == 0 || seat.hi > tab.e1 ? seat.hi : tab.e1;
    }
    if (tab.n == 0) return 0;

    if (!s->ships || !s->ships_b || !s->planets || !s->bullets || !s->hdr) return fail(-4, "a state array is NULL");
    if (!aligned(s->ships, 16) || !aligned(s->planets, 16) || !aligned(s->bullets, 16) || !aligned(s->hdr, 16))
        return fail(-5, "ships/planets/bullets/hdr must be 16-byte aligned");
    if (s->state_f64 != 0 && s->state_f64 != 1) return fail(-6, "state_f64 must be 0 or 1");

    const Base b{base->seed, base->tick0, base->env_offset, base->ship_thrust, base->ship_rspeed, base->bullet_speed,
                 base->ship_radius};
    return dispatch(*p, *s, b, tab, control, static_cast<hipStream_t>(stream));
}

}  // extern "C"
