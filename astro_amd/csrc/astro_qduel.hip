// libastro_qduel.so: astro_qvalues (csrc/astro_qnet.hip) with one network per
// ship, or none (include/astro_qduel.h).
//
// The forward is csrc/astro_qfwd.h's, and so is the argument why every ship's
// q and control are astro_qvalues' with that ship's network, bit for bit.
// What is this kernel's own: astro_qvalues mixes the segments of both ships
// into one 32-column tile and keeps ONE network's five 32x32 layers as
// per-lane MFMA operand registers, so it cannot serve two weight sets.  Here
// the work is ship-major: a workgroup stages the weights of ONE ship's network
// and serves that ship for its whole life (block b serves the (b mod active
// ships)-th ship that has a network); a chunk is 32 consecutive envs of that
// ship, i.e. again 32 SEGMENTS, one per env, in the served ship's ego view.
// Phase A loads the features of BOTH ships of the chunk's 32 envs, one (env,
// ship) per lane of the whole wave.  A ship without a network gets no
// workgroup and no chunk: nothing of it is read or written.
#include <algorithm>

#include "astro_qfwd.h"
#include "astro_qduel.h"

namespace {

// The ships that have a network, in ship order
struct Nets {
    const float *w[2];
    int32_t ship[2];
    int32_t nact;   // 1 or 2
};

template <typename T, int S>
__global__ __launch_bounds__(QN_BLOCK, 2) void astro_qduel_kernel(AstroParams p, AstroState st, Nets nets, int nout,
                                                               float *__restrict__ q_out,
                                                               int8_t *__restrict__ ctl_out, Explore ex,
                                                               int nchunks) {
    __shared__ float s_w0[NH][16];
    __shared__ float s_b[6][NH];
    __shared__ __attribute__((aligned(16))) float s_union[UNION_FLOATS];

    const int l = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int N = st.n_env;

    // The grid is one workgroup or a multiple of nact (the host sees to it):
    // `sets` groups of workgroups, one per network; a lone workgroup with two
    // networks (max_blocks = 1) takes them in turn.
    const int sets = min(int(gridDim.x), nets.nact);
    const int per_set = int(gridDim.x) / sets;
    const int first_chunk = (int(blockIdx.x) / sets) * QN_WAVES + wv;

    for (int a = int(blockIdx.x) % sets; a < nets.nact; a += sets) {
        const float *__restrict__ wts = a == 0 ? nets.w[0] : nets.w[1];
        const int ship = S == 1 ? 0 : (a == 0 ? nets.ship[0] : nets.ship[1]);

        Operands op;
        stage_network<S>(wts, nout, s_w0, s_b, s_union, op);
        WaveLds &W = *reinterpret_cast<WaveLds *>(s_union + wv * WAVE_FLOATS);

        for (int chunk = first_chunk; chunk < nchunks; chunk += per_set * QN_WAVES) {
            const int e0 = chunk * SEGS;
            const int le = l & 31, i = e0 + le;   // the lane's column: env i; in phase A its half is the ship it loads

            int rows = 0;
            if (l < SEGS * S) {
                const int r = load_ship<T, S>(p, st, W, i < N, i, le, l >> 5);
                if (l < SEGS) rows = r;
            }
            scan_rows(W, rows);
            wave_fence();
            if (l < SEGS) ego_part<S>(W, s_w0, s_b, l, l, ship);
            wave_fence();
            pool_rows<T, 1>(p, st, W, op, s_b, e0);
            head<S>(W, op, s_b, nout, q_out, ctl_out, ex, i < N, i, ship);
        }
        __syncthreads();   // every wave is done with its buffers before the next network is staged over them
    }
}

// ---------------------------------------------------------------------------
// host side

int launch(const AstroParams &p, const AstroState &s, const Nets &nets, int nout, float *q, int8_t *control,
           const Explore &ex, int max_blocks, hipStream_t stream) {
    const int nchunks = (s.n_env + SEGS - 1) / SEGS;                 // per ship
    const int per_set = (nchunks + QN_WAVES - 1) / QN_WAVES;         // workgroups that find a chunk, per ship
    const int cap = max_blocks > 0 ? max_blocks : MAX_BLOCKS;
    // one workgroup, or the same number for every ship that has a network
    const int blocks = cap < nets.nact ? 1 : std::min(per_set, cap / nets.nact) * nets.nact;
    with_state(p, s, [&](auto T, auto S) {
        hipLaunchKernelGGL((astro_qduel_kernel<decltype(T), S()>), dim3(unsigned(blocks)), dim3(QN_BLOCK), 0, stream, p,
                           s, nets, nout, q, control, ex, nchunks);
    });
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
    if (int rc = check_shape(p)) return rc;
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
    if (int rc = check_outputs(q, control, epsilon)) return rc;
    if (max_blocks < 0) return fail(-123, "max_blocks must be >= 0, got %d", int(max_blocks));
    if (s->n_env < 0) return fail(-3, "n_env < 0");
    if (s->n_env == 0) return 0;
    for (int k = 0; k < act.nact; ++k) {
        if (!have[k]->weights || !aligned(have[k]->weights, 4))
            return fail(-105, "nets[%d].weights must be a 4-byte aligned device pointer", int(act.ship[k]));
        act.w[k] = have[k]->weights;
    }
    if (int rc = check_arrays(s, q)) return rc;
    return launch(*p, *s, act, int(have[0]->nout), q, control, explore_of(explore, epsilon), max_blocks,
                  static_cast<hipStream_t>(stream));
}

}  // extern "C"
