"""Shared by tests/test_qnet_host.py and tests/test_gpu_qnet.py: the
tests/golden/qnet.npz fixture (tools/gen_golden.py: gen_qnet) and a numpy
restatement of astro_qvalues' exploration rule."""
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
