"""The value reduction of a search over copies of the game (libastro_search.so,
include/astro_search.h): what a branched ``step`` plus ``rollout`` returned,
reduced to one value per (env, control) and a decision, in one launch.

``reduce``        the checked device call (astro_search_values)
``reduce_host``   the numpy mirror, float32 throughout, that the kernel equals
                  bit for bit
``reduce_torch``  the same in plain torch ops, a launch each: what
                  ``fork.Lookahead`` did before the kernel, kept as the
                  yardstick of the tests and of tools/bench_search.py.  Nothing
                  on the play path calls it.

The shape, for all three: N envs, A = 6 own controls, R replies (1 or 6),
M = N A R branches, branch m = (i A + a) R + o; S ships, K ticks.

    reward0  f32 [M, S]      the step's reward, tick 0
    done0    u8  [M]         the step's done
    reward   f32 [K-1, M, S] the rollout's, ticks 1..K-1 (None with K == 1)
    done     u8  [K-1, M]    the same
    gamma    f32 [K+1]       ``gammas(discount, K)``
    leaf     f32 [M, S, 6]   or None: Q values of each branch's last state
                             (only ``ship``'s rows are read)

A branch is worth ``gamma[t] * reward[t, ship]`` at its FIRST done tick t < K;
if it never ends, ``gamma[K] * max(leaf row)`` with a leaf and 0 without.  A
control is worth its worst branch over the R replies.  The decision keeps
``own`` unless some control is strictly better, then takes the first maximal.
"""
import ctypes

import numpy as np
import torch

from . import _lib


class AstroSearch(ctypes.Structure):
    """include/astro_search.h AstroSearch: the shape and the inputs of one value reduction."""
    _fields_ = [
        ('reward0', ctypes.c_void_p),
        ('done0', ctypes.c_void_p),
        ('reward', ctypes.c_void_p),
        ('done', ctypes.c_void_p),
        ('gamma', ctypes.c_void_p),
        ('leaf', ctypes.c_void_p),
        ('n_env', ctypes.c_int32),
        ('replies', ctypes.c_int32),
        ('nships', ctypes.c_int32),
        ('ship', ctypes.c_int32),
        ('horizon', ctypes.c_int32),
        ('reserved', ctypes.c_int32),
    ]


A = NCONTROL = 6        # include/astro_search.h ASTRO_SEARCH_NCONTROL
ABI_VERSION = 1         # ASTRO_SEARCH_ABI_VERSION

SYMBOLS = {
    'astro_search_abi_version': (ctypes.c_int, []),
    'astro_search_last_error': (ctypes.c_char_p, []),
    'astro_search_values': (ctypes.c_int, [ctypes.POINTER(AstroSearch), ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
}

# The library's row.  The binding lives here and not in _lib.py: _lib.LIBS is that module's own table of
# eleven, and this row joins it through _lib.MORE, which build() compiles and _lib.row() finds as well.
load, check = _lib.register('search', 'libastro_search.so', 'astro_search.hip', 'ASTRO_SEARCH_LIB', ABI_VERSION,
                            'astro_search_', SYMBOLS)
ROW = _lib.row('search')


def gammas(discount, horizon):
    """float32 [horizon + 1]: ``discount ** t`` computed in float64 and rounded once."""
    return (float(discount) ** np.arange(int(horizon) + 1)).astype(np.float32)


def shape_of(reward0, done0, reward, done, gamma, replies, leaf=None, own=None):
    """(N, S, K) of the arguments (tensors or arrays), checked against each other; ValueError otherwise."""
    R = int(replies)
    if R not in (1, A):
        raise ValueError('replies must be 1 or %d, got %s' % (A, replies))
    if len(reward0.shape) != 2 or reward0.shape[1] not in (1, 2):
        raise ValueError('reward0 must be [M, S] with S 1 or 2, got %s' % (tuple(reward0.shape),))
    M, S = int(reward0.shape[0]), int(reward0.shape[1])
    if M % (A * R):
        raise ValueError('reward0 has %d branches, not a multiple of %d * %d' % (M, A, R))
    if tuple(done0.shape) != (M,):
        raise ValueError('done0 must be [%d], got %s' % (M, tuple(done0.shape)))
    if len(gamma.shape) != 1 or gamma.shape[0] < 2:
        raise ValueError('gamma must be [K + 1] with K >= 1, got %s' % (tuple(gamma.shape),))
    K = int(gamma.shape[0]) - 1
    if K > 1 or reward is not None or done is not None:
        if reward is None or done is None:
            raise ValueError('reward and done are needed with a horizon of %d' % K)
        if tuple(reward.shape) != (K - 1, M, S) or tuple(done.shape) != (K - 1, M):
            raise ValueError('reward and done must be [%d, %d, %d] and [%d, %d], got %s and %s'
                             % (K - 1, M, S, K - 1, M, tuple(reward.shape), tuple(done.shape)))
    if leaf is not None and tuple(leaf.shape) != (M, S, A):
        raise ValueError('leaf must be [%d, %d, %d], got %s' % (M, S, A, tuple(leaf.shape)))
    N = M // (A * R)
    if own is not None and tuple(own.shape) != (N,):
        raise ValueError('own must be [%d], got %s' % (N, tuple(own.shape)))
    return N, S, K


def _dev(t, dtype, device, what):
    if t is None:
        return
    if not torch.is_tensor(t) or t.dtype != dtype or t.device != device or not t.is_contiguous():
        raise ValueError('%s must be a contiguous %s tensor on %s' % (what, str(dtype).replace('torch.', ''), device))


def reduce(reward0, done0, reward=None, done=None, *, gamma, ship=0, replies=1, leaf=None, own=None, first=False,
           out=None):
    """The device call: ``values`` (float32 [N, 6]; ``out`` if given), then
    ``control`` (int8 [N]) if ``own`` (int8 [N]) is given, then ``first``
    (int32 [M]: each branch's first done tick or -1) if asked -- a tuple when
    more than ``values`` is returned.  All arguments are contiguous device
    tensors of the module docstring's dtypes; one launch on the current stream,
    no synchronisation."""
    N, S, K = shape_of(reward0, done0, reward, done, gamma, replies, leaf, own)
    if not 0 <= int(ship) < S:
        raise ValueError('ship must be in [0, %d), got %s' % (S, ship))
    dev = reward0.device
    for t, dt, what in ((reward0, torch.float32, 'reward0'), (done0, torch.uint8, 'done0'),
                        (reward, torch.float32, 'reward'), (done, torch.uint8, 'done'),
                        (gamma, torch.float32, 'gamma'), (leaf, torch.float32, 'leaf'), (own, torch.int8, 'own')):
        _dev(t, dt, dev, what)
    if out is None:
        out = torch.empty((N, A), dtype=torch.float32, device=dev)
    else:
        _dev(out, torch.float32, dev, 'out')
        if tuple(out.shape) != (N, A):
            raise ValueError('out must be [%d, %d], got %s' % (N, A, tuple(out.shape)))
    control = None if own is None else torch.empty(N, dtype=torch.int8, device=dev)
    t_first = torch.empty(N * A * int(replies), dtype=torch.int32, device=dev) if first else None

    def ptr(t):
        return None if t is None or t.numel() == 0 else t.data_ptr()
    s = AstroSearch(reward0=ptr(reward0), done0=ptr(done0), reward=ptr(reward), done=ptr(done), gamma=ptr(gamma),
                    leaf=ptr(leaf), n_env=N, replies=int(replies), nships=S, ship=int(ship), horizon=K)
    if N:
        check(load().astro_search_values(
            ctypes.byref(s), out.data_ptr(), ptr(own), ptr(control), ptr(t_first), _lib.stream_ptr(dev)),
            'astro_search_values')
    res = (out,) + (() if control is None else (control,)) + (() if t_first is None else (t_first,))
    return res[0] if len(res) == 1 else res


def pick_host(value, own):
    """The decision on float32 [N, 6] values: int8 [N]."""
    value, own = np.asarray(value, np.float32), np.asarray(own).astype(np.int64)
    control = np.empty(len(value), np.int8)
    for i, row in enumerate(value):
        arg = 0
        for k in range(1, A):
            if row[k] > row[arg]:
                arg = k
        keep = 0 <= own[i] < A and not row[arg] > row[own[i]]
        control[i] = own[i] if keep else arg
    return control


def reduce_host(reward0, done0, reward=None, done=None, *, gamma, ship=0, replies=1, leaf=None, own=None):
    """The kernel in numpy, one branch at a time in its own order of
    operations, float32 throughout: ``(value [N, 6], control [N] or None,
    first [M])``."""
    N, S, K = shape_of(reward0, done0, reward, done, gamma, replies, leaf, own)
    R = int(replies)
    reward0, gamma = np.asarray(reward0, np.float32), np.asarray(gamma, np.float32)
    M = N * A * R
    first = np.full(M, -1, np.int32)
    b = np.zeros(M, np.float32)
    for m in range(M):
        if done0[m] != 0:
            first[m] = 0
        else:
            for t in range(1, K):
                if done[t - 1][m] != 0:
                    first[m] = t
                    break
        t = first[m]
        if t == 0:
            b[m] = gamma[0] * reward0[m, ship]
        elif t > 0:
            b[m] = gamma[t] * np.float32(reward[t - 1][m, ship])
        elif leaf is not None:
            best = np.float32(leaf[m, ship, 0])
            for k in range(1, A):
                best = np.fmax(best, np.float32(leaf[m, ship, k]))
            b[m] = gamma[K] * best
    b = b.reshape(N * A, R)
    value = b[:, 0].copy()
    for o in range(1, R):
        less = b[:, o] < value
        value[less] = b[less, o]
    value = value.reshape(N, A)
    return value, (None if own is None else pick_host(value, own)), first


def reduce_torch(reward0, done0, reward=None, done=None, *, gamma, ship=0, replies=1, leaf=None, own=None):
    """The reduction in plain torch: ``values``, or ``(values, control)`` with
    ``own``.  The first-done-tick value and the decision are the formulas
    ``fork.Lookahead`` used before the kernel, unchanged; the leaf, the
    reply minimum and an ``own`` outside 0..5 are added in the plainest ops."""
    N, S, K = shape_of(reward0, done0, reward, done, gamma, replies, leaf, own)
    R = int(replies)
    rew, dn = reward0[None, :, ship], done0[None]
    if K > 1:
        rew, dn = torch.cat([rew, reward[:, :, ship]]), torch.cat([dn, done])
    ended = dn != 0                                            # [K, M]
    first = ended.to(torch.int8).argmax(0, keepdim=True)       # the first done tick (0 where none)
    if leaf is None:
        rest = torch.zeros((), dtype=torch.float32, device=rew.device)
    else:
        rest = gamma[K] * leaf[:, ship, :].max(1).values
    value = torch.where(ended.any(0), gamma[first[0]] * rew.gather(0, first)[0], rest)
    if R > 1:
        b = value.view(N * A, R)
        value = b[:, 0]
        for o in range(1, R):
            value = torch.where(b[:, o] < value, b[:, o], value)
    v = value.reshape(N, A)
    if own is None:
        return v
    own = own.to(torch.int64)
    best, arg = v.max(1).values, v.argmax(1)    # argmax: the first maximal control
    inside = (own >= 0) & (own < A)
    held = v.gather(1, own.clamp(0, A - 1)[:, None])[:, 0]
    return v, torch.where((best > held) | ~inside, arg, own).to(torch.int8)
