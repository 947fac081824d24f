"""Shared by tests/test_qnet_host.py, tests/test_gpu_qnet.py and
tests/test_gpu_qnet_edges.py: the tests/golden/qnet.npz fixture
(tools/gen_golden.py: gen_qnet), the host reference of astro_qvalues on an
oracle Batch with synthetic states for it, and a numpy restatement of
astro_qvalues' exploration rule."""
import functools

import numpy as np

from tests import golden_io as gio

NAMES = ('f0.weight', 'f0.bias', 'f.0.weight', 'f.0.bias', 'f.1.weight', 'f.1.bias',
         'v.0.weight', 'v.0.bias', 'v.1.weight', 'v.1.bias', 'v0.weight', 'v0.bias')


@functools.lru_cache(maxsize=None)
def fixture():
    """{'duo' / 'solo': dict(weights, e_ref, tol)}, q32 [n, 2, 6], q64 [n, 2, 6]."""
    z = gio.load('qnet.npz')
    nets = {}
    for name in ('duo', 'solo'):
        e_ref = float(z['e_ref_' + name])
        nets[name] = dict(weights={k: z['%s__%s' % (name, k)] for k in NAMES}, e_ref=e_ref, tol=4.0 * e_ref)
    return nets, z['q32'], z['q64']


def kind(nships):
    return 'solo' if nships == 1 else 'duo'


def check_argmax_rule(q64, control, tol):
    """The issue's argmax rule on [..., nout] / [...]: wherever the top-2 gap
    of q64 exceeds 2 tol the control must be argmax(q64).  Returns (number
    checked, number skipped for a gap at or below 2 tol)."""
    top = np.sort(q64, axis=-1)
    decided = (top[..., -1] - top[..., -2]) > 2.0 * tol
    want = np.argmax(q64, axis=-1)
    bad = decided & (control != want)
    assert not bad.any(), (np.argwhere(bad)[:5], control[bad][:5], want[bad][:5])
    return int(decided.size), int((~decided).sum())


# ---------------------------------------------------------------------------
# The host reference of astro_qvalues on an oracle Batch (nothing from the
# device enters it) and synthetic states for tests/test_gpu_qnet_edges.py.

def batch_views(B, S):
    """The network's input of every (env, ego view) of an oracle.batched.Batch:
    [float32 [N, rows, nf]] * S, rows = the batch's most live rows, -1 padding
    (oracle.features.batched, pinned bit for bit to the reference's
    get_features; ego 1 by qnet.swap_ego)."""
    from astro_amd import qnet
    from oracle import features
    rows = max(1, int((np.asarray(B.nplanets) + np.asarray(B.nbullets)).max()))
    f = features.batched(B, S, rows=rows)
    return [f] if S == 1 else [f, qnet.swap_ego(f)]


def q64_of_views(weights, views, block=512):
    """qnet.forward64 on batch_views' output: float64 [N, S, nout]."""
    from astro_amd import qnet
    n = views[0].shape[0]
    return np.stack([np.concatenate([qnet.forward64(weights, v[a:a + block]) for a in range(0, n, block)])
                     for v in views], 1)


def q32_of_views(weights, views, block=512):
    """The project's torch ValueNetwork in float32 on the CPU on the same
    input: float32 [N, S, nout]."""
    import torch
    from astro_amd import qnet
    w = {k: np.asarray(v, dtype=np.float32) for k, v in weights.items()}
    m = qnet.ValueNetwork(w['f0.weight'].shape[1] == 10, w['v0.weight'].shape[0])
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in w.items()})
    n = views[0].shape[0]
    with torch.no_grad():
        return np.stack([torch.cat([m(torch.from_numpy(np.ascontiguousarray(v[a:a + block])))
                                    for a in range(0, n, block)]).numpy() for v in views], 1)


def reference_of(weights, B, S):
    """(q64 [N, S, nout], e_ref = max |q32 - q64|) of a Batch, from one set of features."""
    views = batch_views(B, S)
    q64 = q64_of_views(weights, views)
    return q64, float(np.abs(q32_of_views(weights, views).astype(np.float64) - q64).max())


def q64_of_batch(weights, B, S):
    """The float64 forward pass of every ship's ego view of every env of B."""
    return q64_of_views(weights, batch_views(B, S))


def e_ref_of(weights, B, S):
    """max |q32 - q64| over B: the float32 forward's own distance from float64 (tol = 4 e_ref)."""
    return reference_of(weights, B, S)[1]


def synthetic_batch(counts, S, p_pad, rng, tick, bearings=None):
    """A Batch of len(counts) envs with (nplanets, nbullets) = counts[i] live
    objects, b_cap = max(1, most bullets) slots, every env at ``tick``.  All
    values are float32-representable: positions and velocities uniform in
    [-1.2, 1.2], bearings uniform in [-10, 10] unless given ([N, S]).  Dead
    slots hold NaN (they are never read).  The states need not be reachable
    games: the forward pass is defined on any state."""
    from oracle import batched
    counts = np.asarray(counts, dtype=np.int64).reshape(-1, 2)
    n = counts.shape[0]
    if (counts[:, 0] < 1).any() or (counts[:, 0] > p_pad).any() or (counts[:, 1] < 0).any():
        raise ValueError('counts must have 1 <= nplanets <= p_pad and nbullets >= 0')
    b_cap = max(1, int(counts[:, 1].max()))
    u = lambda *shape: rng.uniform(-1.2, 1.2, size=shape).astype(np.float32).astype(np.float64)  # noqa: E731
    B = batched.Batch.zeros(n, S, p_pad, b_cap)
    B.tick[:] = tick
    B.nplanets[:] = counts[:, 0]
    B.nbullets[:] = counts[:, 1]
    B.ships[:] = u(n, S, 4)
    B.planets[:] = u(n, p_pad, 4)
    B.bullets[:] = u(n, b_cap, 4)
    if bearings is None:
        B.ships_b[:] = rng.uniform(-10.0, 10.0, size=(n, S)).astype(np.float32)
    else:
        B.ships_b[:] = np.asarray(bearings, dtype=np.float64).reshape(n, S)
    B.planets[np.arange(p_pad)[None, :] >= counts[:, :1]] = np.nan
    B.bullets[np.arange(b_cap)[None, :] >= counts[:, 1:]] = np.nan
    return B


def scaled(weights, factor):
    """Every weight and bias of a network times ``factor`` (float32)."""
    return {k: (np.asarray(v, dtype=np.float32) * np.float32(factor)) for k, v in weights.items()}


M64 = (1 << 64) - 1


def random_words(n_env, nships, env_offset, tick0, seed):
    """The splitmix64 word ASTRO_POLICY_RANDOM draws for every (env, ship) at
    tick ``tick0`` (include/astro_step.h), as uint64 [n_env, nships]."""
    out = np.zeros((n_env, nships), dtype=np.uint64)
    for i in range(n_env):
        for s in range(nships):
            z = ((env_offset + i) * nships + s) * 0x9E3779B97F4A7C15 + (tick0 + 1) * 0xD1B54A32D192ED03 + seed
            z &= M64
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
            z ^= z >> 31
            out[i, s] = z
    return out


def explore(greedy, epsilon, env_offset, tick0, seed):
    """astro_qvalues' epsilon-greedy choice: greedy int [n_env, nships] ->
    (controls, explored mask)."""
    n_env, nships = greedy.shape
    z = random_words(n_env, nships, env_offset, tick0, seed)
    lo = (z & np.uint64(0xFFFFFFFF)).astype(np.uint64)
    threshold = np.uint64(int(epsilon * 4294967296.0))
    hit = lo < threshold
    rnd = (((z >> np.uint64(32)) * np.uint64(6)) >> np.uint64(32)).astype(np.int64)
    return np.where(hit, rnd, greedy), hit
