"""The experience replay of astro/rl.py's ``QBotTrainer`` (rl.py:231-332) for a
whole ``BatchedEnv``, on the device (csrc/astro_replay.hip,
include/astro_replay.h).

``ReplayBuffer`` is a time-major ring: tick ``t`` of every env lives in row
``t % ticks``.  One feature tensor per (tick, env) serves both ships (ship 1
sees ``qnet.swap_ego`` of it) and every experience's next state, which is an
index (``next``) to a later row of the same env -- in the reference a
non-terminal flush's ``new_state_f`` is the ``state_f`` the same bot records on
the next tick.  A training tick is::

    env.features(out=buf.head())              # the observation, straight into the ring
    control = env.qcontrols(net, epsilon, seed, tick0=buf.t)
    _, reward, done = env.step(control)
    buf.push(control, reward, done)           # n-step returns (rl.py:303-319)
    ids = buf.sample(1024, seed, draw=buf.t)  # rl.py:263-276
    f, a, r, d, nf, term = buf.gather(ids)
    loss = net.sgd_step(f, a, net.td_targets(r, d, nf, term))
    buf.update_loss(ids, loss)                # rl.py:298-299

What differs from the reference: the ring overwrites its oldest row where the
reference drops half of its list at ``max_replay``; the sampling is the
distribution of ``RandomState.choice(replace=False, p=loss / sum)`` (successive
sampling without replacement, by exponential keys) but not numpy's random
stream; and where ``_step`` asserts (more unscored experiences than ``n``) or
numpy raises (fewer positive losses than needed) ``sample`` returns a uniform
subset of the unscored ones, and takes zero-loss experiences last, in id order.

``push_host`` and ``sample_host`` restate the two kernels in numpy (the tests'
truth).
"""
import ctypes

import numpy as np
import torch

from . import _lib

NEXT_TERMINAL, NEXT_PENDING = -1, -2
M64 = (1 << 64) - 1


def gpow_table(discount, n_steps):
    """discount ** i for i = 0 .. n_steps in Python float64: the powers
    rl.py:313 takes, so the device multiplies by the reference's own values."""
    return np.array([float(discount) ** i for i in range(int(n_steps) + 1)], dtype=np.float64)


# ---------------------------------------------------------------------------
# the host model

def new_host(n_env, nships, ticks):
    """The metadata of an empty ring as numpy arrays (ReplayBuffer's initial state)."""
    N, S, T = int(n_env), int(nships), int(ticks)
    return dict(action=np.zeros((T, N, S), np.int8), reward=np.zeros((T, N, S), np.float32),
                discount=np.zeros((T, N), np.float32), next=np.full((T, N), NEXT_PENDING, np.int32),
                loss=np.full((T, N, S), np.inf, np.float32), wstart=np.zeros(N, np.int64))


def push_host(h, t, control, reward, done, n_steps=100, discount=0.995):
    """astro_replay_push on ``new_host``'s arrays, in place: tick ``t`` with
    control int8 [N, S], reward float32 [N, S], done [N] (nonzero = ended)."""
    ticks = h['next'].shape[0]
    row = t % ticks
    reward = np.asarray(reward, dtype=np.float32)
    h['action'][row] = np.asarray(control, dtype=np.int8)
    h['reward'][row] = 0
    h['discount'][row] = 0
    h['next'][row] = NEXT_PENDING
    h['loss'][row] = np.inf
    gpow = gpow_table(discount, n_steps)
    done = np.asarray(done) != 0
    w = h['wstart']
    for e in np.nonzero(done | (t - w + 1 >= n_steps))[0]:
        L = int(t - w[e]) + 1
        for j in range(L):
            r = int(w[e] + j) % ticks
            g = gpow[L - 1 - j]
            h['reward'][r, e] = (reward[e].astype(np.float64) * g).astype(np.float32)
            h['discount'][r, e] = np.float32(float(discount) * g)
            h['next'][r, e] = NEXT_TERMINAL if done[e] else (t + 1) % ticks
        w[e] = t + 1


def random_words(ids, seed, draw):
    """The splitmix64 word of each id (uint64): the project's mix of
    id * 0x9E3779B97F4A7C15 + (draw + 1) * 0xD1B54A32D192ED03 + seed."""
    with np.errstate(over='ignore'):
        z = (np.asarray(ids).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
             + np.uint64(((int(draw) + 1) * 0xD1B54A32D192ED03 + int(seed)) & M64))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def keys_host(loss, ids, seed, draw, ulps=0):
    """(class int [n], key float32 [n]) of the experiences ``ids`` with losses
    ``loss``.  ulps: move every E by that many float64 steps first (the tests'
    guard against two log implementations that differ in the last place)."""
    loss = np.asarray(loss, dtype=np.float32)
    z = random_words(ids, seed, draw)
    u = ((z >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    E = np.abs(-np.log(u))
    if ulps:
        E = np.maximum(E.view(np.int64) + int(ulps), 0).view(np.float64)
    cls = np.where(loss == np.inf, 0, np.where((loss > 0) & np.isfinite(loss), 1, 2))
    with np.errstate(all='ignore'):
        ratio = (E / loss.astype(np.float64)).astype(np.float32)
    key = np.where(cls == 0, E.astype(np.float32), np.where(cls == 1, ratio, np.float32(0))).astype(np.float32)
    return cls, key


def select_host(loss, eligible, n, seed=0, draw=0, ulps=0):
    """The selection on flat arrays: of the ids where ``eligible``, the
    min(n, eligible) smallest in (class, key, id), ascending (int32)."""
    ids = np.nonzero(np.asarray(eligible).ravel())[0]
    cls, key = keys_host(np.asarray(loss).ravel()[ids], ids, seed, draw, ulps)
    order = np.lexsort((ids, key, cls))      # a full sort; the last key is the primary one
    return np.sort(ids[order[:max(0, int(n))]]).astype(np.int32)


def eligible_host(nxt, t, nships):
    """bool [ticks, N, S]: the row is written, is not the head row, and its
    next is neither pending nor the head row (``t`` pushes so far)."""
    ticks = nxt.shape[0]
    head = t % ticks
    rows = np.arange(ticks)
    ok = ((rows < min(t, ticks)) & (rows != head))[:, None] & (nxt != NEXT_PENDING) & (nxt != head)
    return np.repeat(ok[:, :, None], int(nships), axis=2)


def sample_host(loss, nxt, t, n, seed=0, draw=0, ulps=0):
    """astro_replay_sample in numpy: keys in float64 then float32, a full sort.
    loss float32 [ticks, N, S], nxt int32 [ticks, N], ``t`` pushes so far."""
    return select_host(loss, eligible_host(np.asarray(nxt), int(t), np.asarray(loss).shape[2]), n, seed, draw, ulps)


# ---------------------------------------------------------------------------
# the device buffer

class ReplayBuffer:
    """rl.QBotTrainer's n-step buffer and replay buffer for ``n_env`` envs of
    ``nships`` ships, ``rows`` feature rows per state, ``ticks`` ring rows
    (>= n_steps + 2).  The public tensors (all on ``device``):

      features [ticks, N, rows, 5 + 5 S] f32    action [ticks, N, S] i8
      reward   [ticks, N, S] f32                discount [ticks, N] f32
      next     [ticks, N] i32 (ring row of the next state; -1 terminal, -2 pending)
      loss     [ticks, N, S] f32 (+inf = not yet scored)
      wstart   [N] i64 (tick at which the env's open window began)

    ``t`` is the number of pushes so far; the head row is ``t % ticks``.  The
    head row is never sampled, nor an entry whose next is the head row, so the
    coming tick's features may be written (``head()``) before ``push``.  An
    entry's next row is newer than the entry, so the ring overwrites an entry
    before the row it points to.  Calls are stream-ordered on the current
    stream; ``sample`` shares one cached workspace (one stream at a time)."""

    def __init__(self, n_env, rows, nships, ticks, n_steps=100, discount=0.995, device='cuda'):
        N, R, S, T, n_steps = int(n_env), int(rows), int(nships), int(ticks), int(n_steps)
        if S not in (1, 2):
            raise ValueError('nships must be 1 or 2, got %d' % S)
        if N < 1 or R < 1 or n_steps < 1:
            raise ValueError('n_env, rows and n_steps must be >= 1')
        if T < n_steps + 2:
            raise ValueError('ticks must be >= n_steps + 2 = %d, got %d' % (n_steps + 2, T))
        if T * N * S > 2 ** 31 - 1:
            raise ValueError('ticks * n_env * nships = %d ids do not fit an int32' % (T * N * S))
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise ValueError('ReplayBuffer lives on a HIP device (got %s)' % self.device)
        self.n_env, self.rows, self.nships, self.ticks, self.n_steps = N, R, S, T, n_steps
        self.gamma = float(discount)
        self.nf = 5 + 5 * S
        self.t = 0
        dev = self.device
        self.features = torch.zeros((T, N, R, self.nf), dtype=torch.float32, device=dev)
        self.action = torch.zeros((T, N, S), dtype=torch.int8, device=dev)
        self.reward = torch.zeros((T, N, S), dtype=torch.float32, device=dev)
        self.discount = torch.zeros((T, N), dtype=torch.float32, device=dev)
        self.next = torch.full((T, N), NEXT_PENDING, dtype=torch.int32, device=dev)
        self.loss = torch.full((T, N, S), float('inf'), dtype=torch.float32, device=dev)
        self.wstart = torch.zeros(N, dtype=torch.int64, device=dev)
        self.gpow = torch.from_numpy(gpow_table(discount, n_steps)).to(dev)
        self.c = _lib.AstroReplay(
            features=self.features.data_ptr(), action=self.action.data_ptr(), reward=self.reward.data_ptr(),
            discount=self.discount.data_ptr(), next=self.next.data_ptr(), loss=self.loss.data_ptr(),
            wstart=self.wstart.data_ptr(), gpow=self.gpow.data_ptr(), gamma=self.gamma, n_env=N, rows=R, nships=S,
            ticks=T, n_steps=n_steps, reserved=0)
        self._count = torch.zeros(1, dtype=torch.int32, device=dev)
        self._workspace = None

    def _arg(self, v, shape, dtype, what):
        if not torch.is_tensor(v) or v.device != self.device:
            v = torch.as_tensor(v, device=self.device)
        if tuple(v.shape) != tuple(shape):
            raise ValueError('%s must be %s, got %s' % (what, list(shape), list(v.shape)))
        return v.to(dtype).contiguous()

    def _out(self, out, shape, dtype, what):
        if out is None:
            return torch.empty(shape, dtype=dtype, device=self.device)
        if (not torch.is_tensor(out) or tuple(out.shape) != tuple(shape) or out.dtype != dtype
                or out.device != self.device or not out.is_contiguous()):
            raise ValueError('%s must be a contiguous %s %s tensor on %s' % (what, dtype, list(shape), self.device))
        return out

    def _ids(self, ids):
        if (not torch.is_tensor(ids) or ids.dim() != 1 or ids.dtype != torch.int32 or ids.device != self.device
                or not ids.is_contiguous()):
            raise ValueError('ids must be a contiguous int32 [n] tensor on %s' % self.device)
        return int(ids.shape[0])

    def head(self):
        """The contiguous [N, rows, nf] view of the row of the coming tick:
        ``env.features(out=buf.head())`` writes the observation into the ring."""
        return self.features[self.t % self.ticks]

    def push(self, control, reward, done):
        """One tick of every env (rl.py:255 and 303-319): ``control`` int8
        [N, S] acted on the state in ``head()``, ``reward`` float32 [N, S] and
        ``done`` uint8 [N] are what ``env.step(control)`` returned.  A window
        closes when its env is done or it holds n_steps ticks; its entries get
        reward * discount ** (L-1-j), discount ** (L-j) and their next row."""
        N, S = self.n_env, self.nships
        c = self._arg(control, (N, S), torch.int8, 'control')
        r = self._arg(reward, (N, S), torch.float32, 'reward')
        d = self._arg(done, (N,), torch.uint8, 'done')
        _lib.check_replay(_lib.load_replay().astro_replay_push(
            ctypes.byref(self.c), self.t, c.data_ptr(), r.data_ptr(), d.data_ptr(), _lib.stream_ptr(self.device)),
            'astro_replay_push')
        self._keep = (c, r, d)   # alive until the call has run
        self.t += 1

    def eligible_lower_bound(self):
        """Experiences eligible whatever the dones were: every window of a row
        older than n_steps + 1 ticks has closed on an earlier row than the head."""
        return max(0, min(self.t, self.ticks - 1) - self.n_steps) * self.n_env * self.nships

    def sample(self, n, seed=0, draw=0, out=None):
        """rl.QBotTrainer._step's choice (rl.py:263-276): up to ``n`` eligible
        experience ids (int32, ascending; id = (row * N + env) * S + ship).
        Unscored experiences (loss +inf) come first; the rest are drawn without
        replacement with probability proportional to their loss, the
        distribution of numpy's ``choice(replace=False, p)``, by exponential
        keys from the project's splitmix64 stream of (id, draw, seed) --
        numpy's random stream is not reproduced.  Zero-loss experiences come
        last.  Deterministic bit for bit.  The device count is read (a host
        synchronisation) only when ``n`` exceeds ``eligible_lower_bound()``."""
        n = int(n)
        if n < 0:
            raise ValueError('n < 0')
        ids = self._out(out, (n,), torch.int32, 'out')
        lib = _lib.load_replay()
        need = int(lib.astro_replay_sample_workspace_bytes(ctypes.byref(self.c)))
        ws = self._workspace
        if ws is None or ws.numel() * 4 < need:
            ws = self._workspace = torch.empty((need + 3) // 4, dtype=torch.float32, device=self.device)
        return self._sample(n, seed, draw, ids, ws)

    def _sample(self, n, seed, draw, ids, ws):
        _lib.check_replay(_lib.load_replay().astro_replay_sample(
            ctypes.byref(self.c), self.t, n, int(seed) & M64, int(draw) & M64, ids.data_ptr() if n else None,
            self._count.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size(), _lib.stream_ptr(self.device)),
            'astro_replay_sample')
        if n <= self.eligible_lower_bound():
            return ids
        return ids[:int(self._count.item())]

    def last_count(self):
        """The device count of the last ``sample``: min(n, eligible).  Synchronises."""
        return int(self._count.item())

    def gather(self, ids, out=None):
        """The experiences ``ids`` as training tensors: (features [n, rows, nf],
        action int8 [n], reward f32 [n], discount f32 [n], next_features
        [n, rows, nf], terminal uint8 [n]), ship 1's in its own ego view.
        Column 0 of every row and every column of a live row are exact; the
        other columns of padding rows are not written (the Q-network kernels
        never read them).  A terminal sample's next_features has column 0 = -1
        throughout.  out: a tuple of six tensors to write into."""
        n = self._ids(ids)
        o = (None,) * 6 if out is None else tuple(out)
        shape = (n, self.rows, self.nf)
        f = self._out(o[0], shape, torch.float32, 'out[0]')
        a = self._out(o[1], (n,), torch.int8, 'out[1]')
        r = self._out(o[2], (n,), torch.float32, 'out[2]')
        d = self._out(o[3], (n,), torch.float32, 'out[3]')
        nf = self._out(o[4], shape, torch.float32, 'out[4]')
        term = self._out(o[5], (n,), torch.uint8, 'out[5]')
        if n:
            _lib.check_replay(_lib.load_replay().astro_replay_gather(
                ctypes.byref(self.c), ids.data_ptr(), n, f.data_ptr(), a.data_ptr(), r.data_ptr(), d.data_ptr(),
                nf.data_ptr(), term.data_ptr(), _lib.stream_ptr(self.device)), 'astro_replay_gather')
        return f, a, r, d, nf, term

    def update_loss(self, ids, loss):
        """rl.py:298-299: ``loss[ids] = loss`` (float32 [n]); the next ``sample``
        weighs these experiences by it."""
        n = self._ids(ids)
        loss = self._arg(loss, (n,), torch.float32, 'loss')
        if n:
            _lib.check_replay(_lib.load_replay().astro_replay_update(
                ctypes.byref(self.c), ids.data_ptr(), loss.data_ptr(), n, _lib.stream_ptr(self.device)),
                'astro_replay_update')
            self._keep_loss = loss
