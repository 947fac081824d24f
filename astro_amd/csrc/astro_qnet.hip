// libastro_qnet.so: rl.ValueNetwork.forward + rl.QBot's argmax (+ epsilon-greedy)
// for every ship of every env, fused over the AstroState arrays
// (include/astro_qnet.h).
//
// The forward, its three phases and its numerics are csrc/astro_qfwd.h's.
// What is this kernel's own: one network serves every ship, a chunk is
// CH = 32 / S consecutive envs whose 32 tile columns are (env, ego) SEGMENTS,
// S per env with the column's ship as ego, and the chunks go round the grid.
#include <algorithm>

#include "astro_qfwd.h"

namespace {

template <typename T, int S>
__global__ __launch_bounds__(QN_BLOCK, 2) void astro_qvalues_kernel(AstroParams p, AstroState st,
                                                                 const float *__restrict__ wts, int nout,
                                                                 float *__restrict__ q_out,
                                                                 int8_t *__restrict__ ctl_out, Explore ex,
                                                                 int nchunks) {
    constexpr int CH = SEGS / S;           // envs per chunk
    __shared__ float s_w0[NH][16];
    __shared__ float s_b[6][NH];
    __shared__ __attribute__((aligned(16))) float s_union[UNION_FLOATS];

    const int l = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int N = st.n_env;

    Operands op;
    stage_network<S>(wts, nout, s_w0, s_b, s_union, op);
    WaveLds &W = *reinterpret_cast<WaveLds *>(s_union + wv * WAVE_FLOATS);

    for (int chunk = blockIdx.x * QN_WAVES + wv; chunk < nchunks; chunk += gridDim.x * QN_WAVES) {
        const int e0 = chunk * CH;
        const int le = (l & 31) / S, s = (l & 31) - le * S, i = e0 + le;   // the lane's column: segment l & 31

        int rows = 0;
        if (l < SEGS) rows = load_ship<T, S>(p, st, W, i < N, i, le, s);
        scan_rows(W, rows);
        wave_fence();
        if (l < SEGS) ego_part<S>(W, s_w0, s_b, l, le, s);
        wave_fence();
        pool_rows<T, S>(p, st, W, op, s_b, e0);
        head<S>(W, op, s_b, nout, q_out, ctl_out, ex, i < N, i, s);
    }
}

// ---------------------------------------------------------------------------
// host side

int launch(const AstroParams &p, const AstroState &s, const AstroQNet &net, float *q, int8_t *control,
           const Explore &ex, hipStream_t stream) {
    const int CH = SEGS / p.nships;
    const int nchunks = (s.n_env + CH - 1) / CH;
    const int blocks = std::min((nchunks + QN_WAVES - 1) / QN_WAVES, MAX_BLOCKS);
    with_state(p, s, [&](auto T, auto S) {
        hipLaunchKernelGGL((astro_qvalues_kernel<decltype(T), S()>), dim3(unsigned(blocks)), dim3(QN_BLOCK), 0, stream,
                           p, s, net.weights, int(net.nout), q, control, ex, nchunks);
    });
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
    if (int rc = check_shape(p)) return rc;
    if (net->nships != p->nships)
        return fail(-101, "net.nships (%d) must equal params.nships (%d)", int(net->nships), int(p->nships));
    if (net->nout < 1 || net->nout > ASTRO_QNET_MAX_OUT)
        return fail(-102, "net.nout must be in [1, %d], got %d", ASTRO_QNET_MAX_OUT, int(net->nout));
    if (int rc = check_outputs(q, control, epsilon)) return rc;
    if (s->n_env < 0) return fail(-3, "n_env < 0");
    if (s->n_env == 0) return 0;
    if (!net->weights || !aligned(net->weights, 4))
        return fail(-105, "net.weights must be a 4-byte aligned device pointer");
    if (int rc = check_arrays(s, q)) return rc;
    return launch(*p, *s, *net, q, control, explore_of(explore, epsilon), static_cast<hipStream_t>(stream));
}

}  // extern "C"
