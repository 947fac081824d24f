// libastro_qpool.so: astro_qvalues (csrc/astro_qnet.hip) with a pool of
// networks, each playing one ship of a block of envs (include/astro_qpool.h).
//
// The forward is csrc/astro_qfwd.h's, and so is the argument why every covered
// (ship, env) gets astro_qvalues' q and control with its network, bit for bit:
// where a chunk begins changes nothing.  What is this kernel's own:
// astro_qvalues_ships (csrc/astro_qduel.hip) is ship-major, a workgroup stages
// ONE network's weights and walks chunks of 32 consecutive envs of one ship.
// Here the unit is a SPAN -- ship s of the envs [lo, hi), played by network k
// -- and the rest is that kernel: a workgroup stages the weights of a span's
// network and serves chunks of that span; a chunk is 32 consecutive envs
// counted from lo (not aligned to 32), the last one of a span partial, so
// astro_qduel_kernel's `i < N` is `i < hi` here.  A (ship, env) outside every
// span with a network belongs to no chunk: nothing of it is read or written.
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
#include <algorithm>

#include "astro_qfwd.h"
#include "astro_qpool.h"

namespace {

constexpr int MAX_NETS = ASTRO_QPOOL_MAX_NETS;
constexpr int MAX_SPANS = ASTRO_QPOOL_MAX_SPANS;

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

template <typename T, int S>
__global__ __launch_bounds__(QN_BLOCK, 2) void astro_qpool_kernel(AstroParams p, AstroState st, Work work, int nout,
                                                               float *__restrict__ q_out,
                                                               int8_t *__restrict__ ctl_out, Explore ex) {
    __shared__ float s_w0[NH][16];
    __shared__ float s_b[6][NH];
    __shared__ __attribute__((aligned(16))) float s_union[UNION_FLOATS];

    const int l = threadIdx.x & 63, wv = threadIdx.x >> 6;

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

    Operands op;
    int staged = -1;
    WaveLds &W = *reinterpret_cast<WaveLds *>(s_union + wv * WAVE_FLOATS);

    for (int k = k0; k < k1; ++k) {
        const int net = work.net[k];
        const int ship = S == 1 ? 0 : work.ship[k];
        const int lo = work.lo[k], hi = work.hi[k];

        if (net != staged) {
            staged = net;
            stage_network<S>(work.w[net], nout, s_w0, s_b, s_union, op);
        }

        const int nchunks = (hi - lo + SEGS - 1) / SEGS;
        for (int chunk = mine * QN_WAVES + wv; chunk < nchunks; chunk += nblk * QN_WAVES) {
            const int e0 = lo + chunk * SEGS;   // < hi
            const int left = hi - e0;           // the chunk's envs are e0 + (0 .. min(left, 32) - 1)
            const int le = l & 31, i = e0 + le;   // the lane's column: env i; in phase A its half is the ship it loads

            int rows = 0;
            if (l < SEGS * S) {
                const int r = load_ship<T, S>(p, st, W, le < left, i, le, l >> 5);
                if (l < SEGS) rows = r;
            }
            scan_rows(W, rows);
            wave_fence();
            if (l < SEGS) ego_part<S>(W, s_w0, s_b, l, l, ship);
            wave_fence();
            pool_rows<T, 1>(p, st, W, op, s_b, e0);
            head<S>(W, op, s_b, nout, q_out, ctl_out, ex, le < left, i, ship);   // lo <= i < hi <= n_env where valid
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

int launch(const AstroParams &p, const AstroState &s, const Work &work, int grid, int nout, float *q, int8_t *control,
           const Explore &ex, hipStream_t stream) {
    with_state(p, s, [&](auto T, auto S) {
        hipLaunchKernelGGL((astro_qpool_kernel<decltype(T), S()>), dim3(unsigned(grid)), dim3(QN_BLOCK), 0, stream, p,
                           s, work, nout, q, control, ex);
    });
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
    if (int rc = check_shape(p)) return rc;
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
    if (int rc = check_outputs(q, control, epsilon)) return rc;
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
    if (int rc = check_arrays(s, q)) return rc;

    const int grid = share_out(work, max_blocks);
    return launch(*p, *s, work, grid, int(nets[one].nout), q, control, explore_of(explore, epsilon),
                  static_cast<hipStream_t>(stream));
}

}  // extern "C"
