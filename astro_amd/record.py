"""Whole games of a few envs of a ``BatchedEnv``, recorded on the device
(csrc/astro_trace.hip, include/astro_trace.h).

The reference's trainer saves a validation game with ``core.save_log``
(rl.py:352-355), each tick with ``QBot.data`` = ``dict(q=...)`` (rl.py:195-209)
for the viewer's six arrows (static/astro.js:129-143).  ``logs.record_games``
gets such games by copying the whole batch to the host every tick; a
``Recorder`` gathers the chosen envs' ticks into a small device ring instead --
one launch before the step (the state the bots saw, their controls, the
networks' Q values) and one after it (reward, done) -- and copies the ring to
the host only where the caller synchronises anyway:

    rec = Recorder(env, [0, 1, 2, 3], q=True)
    env.play_q(net, opponent='script', games=2, record=rec)
    rec.save('logs')              # logs/<env>_<k>.log, read by the reference's load_log and viewer

``decode`` turns drained slots into the reference's ``Game`` / ``Tick`` tuples
on the host (no device needed); ``play`` is ``logs.record_games`` on the device.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from . import logs as _logs
from .config import Game, Tick, reference_state

INT32_MAX = 2 ** 31 - 1


def check_ring(n_env, env_ids, ticks, S, p_pad, b_cap, nout=0):
    """The validated ids (int32 array) of a ring of ``ticks`` slots for the
    envs ``env_ids`` of a batch of ``n_env``; ValueError for an empty list,
    duplicates, an id outside [0, n_env), ticks < 1, nout outside 0..6 or a
    ring array of more than 2^31 - 1 elements.  Host arithmetic only."""
    try:
        ids = [int(i) for i in env_ids]
        if any(i != v for i, v in zip(ids, env_ids)):
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError('env_ids must be a sequence of integers') from None
    if not ids:
        raise ValueError('env_ids is empty')
    if len(set(ids)) != len(ids):
        raise ValueError('env_ids names an env twice')
    bad = [i for i in ids if not 0 <= i < int(n_env)]
    if bad:
        raise ValueError('env id %d is outside [0, %d)' % (bad[0], int(n_env)))
    ticks, nout = int(ticks), int(nout)
    if ticks < 1:
        raise ValueError('ticks must be >= 1, got %d' % ticks)
    if not 0 <= nout <= _lib.TRACE_MAX_OUT:
        raise ValueError('nout must be in [0, %d], got %d' % (_lib.TRACE_MAX_OUT, nout))
    largest = ticks * len(ids) * max(4 * int(S), 4 * int(p_pad), 4 * int(b_cap), int(S) * nout)
    if largest > INT32_MAX:
        raise ValueError('a ring of %d ticks for %d envs has an array of %d elements: more than an int32'
                         % (ticks, len(ids), largest))
    return np.asarray(ids, dtype=np.int32)


def decode(ring, n, ids, schedule, config, S, pending=None, played=None, skip=()):
    """Slots 0 .. n-1 of a drained ring as the reference's tuples.

    ring: numpy arrays in the ring's layout -- ``ships`` [ticks, m, S, 4],
    ``ships_b`` [ticks, m, S], ``planets`` [ticks, m, p_pad, 4], ``bullets``
    [ticks, m, b_cap, 4], ``hdr`` int32 [ticks, m, 4] (tick, nplanets | flags
    << 8 | nbullets << 16, the game's seed, 0), ``control`` int8 [ticks, m, S],
    ``reward`` float32 [ticks, m, S], ``done`` uint8 [ticks, m] and, optionally,
    ``q`` float32 [ticks, m, S, nout].  ids: the m env ids.  schedule, config,
    S: the env's.  pending: per env id the ticks of its open game, extended in
    place (a dict; None: every env starts empty).  played: per slot either None
    or a bool [S] / [m, S] array, True where a network played the ship -- its
    ``bot_data`` is ``dict(q=float32 [nout])`` there and None elsewhere (None
    everywhere without ``q``).  skip: env ids whose slots are ignored.

    Every Tick is what ``logs.record_games`` builds: the state by
    ``config.reference_state``, control int64 [S], reward int64 on a collision,
    float32 on a timeout and float32 zeros otherwise, and a finished game's
    winner and ``config._replace(seed=...)`` from its last tick.  Returns
    (the newly finished games as [(env_id, Game)] in slot order, pending)."""
    pending = {} if pending is None else pending
    S = int(S)
    hdr = np.asarray(ring['hdr']).view(np.uint32)
    p_pad, b_cap = ring['planets'].shape[2], ring['bullets'].shape[2]
    q = ring.get('q')
    finished = []
    for t in range(int(n)):
        who = None if played is None or q is None else played[t]
        who = None if who is None else np.broadcast_to(np.asarray(who, dtype=bool), (len(ids), S))
        for j, env_id in enumerate(ids):
            env_id = int(env_id)
            if env_id in skip:
                continue
            tick, word = int(hdr[t, j, 0]), int(hdr[t, j, 1])
            npl, nb = min(word & 0xff, p_pad), min((word >> 16) & 0xffff, b_cap)
            state = reference_state(ring['ships'][t, j], ring['ships_b'][t, j], ring['planets'][t, j, :npl],
                                    ring['bullets'][t, j, :nb], tick, schedule)
            d = int(ring['done'][t, j])
            if d == 1:
                reward = ring['reward'][t, j, :S].astype(np.int64)
            elif d == 2:
                reward = ring['reward'][t, j, :S].astype(np.float32)
            else:
                reward = np.zeros(S, dtype=np.float32)
            data = [dict(q=np.array(q[t, j, s], dtype=np.float32)) if who is not None and who[j, s] else None
                    for s in range(S)]
            ticks = pending.setdefault(env_id, [])
            ticks.append(Tick(state=state, control=ring['control'][t, j, :S].astype(np.int64), reward=reward,
                              bot_data=data))
            if d:
                winner = None if np.max(reward) < 1 else int(np.argmax(reward))
                cfg = config._replace(seed=int(hdr[t, j, 2]) & 0xFFFFFFFF)
                finished.append((env_id, Game(config=cfg, winner=winner, ticks=ticks)))
                pending[env_id] = []
    return finished, pending


class Recorder:
    """A device ring of ``ticks`` slots for the envs ``env_ids`` of ``env``.

    q: False -- no Q values, ``bot_data`` is None; True -- the ring takes the
    nout of the first Q tensor ``state`` is given; an int -- that nout.  Each
    tick: ``state(control, q)`` before ``env.step``, ``result(reward, done)``
    after it; ``drain()`` at the latest when ``fill == ticks``.  ``games``:
    per env id the finished games so far.  limit: record at most that many
    games per env (None: all)."""

    def __init__(self, env, env_ids, ticks=64, q=False, limit=None):
        nout = _lib.TRACE_MAX_OUT if q is True else int(q or 0)     # q=True: sized for the largest network
        self.wants_q = nout != 0
        ids = check_ring(env.n_env, env_ids, ticks, env.S, env.p_pad, env.b_cap, nout)
        self.env, self.ids, self.ticks = env, [int(i) for i in ids], int(ticks)
        self.m, self.limit = len(ids), limit
        self.nout = 0 if q is True else nout        # q=True: known at the first state()
        self.fill, self.open = 0, False
        self.games = {i: [] for i in self.ids}
        self._pending = {}
        self._played = [None] * self.ticks
        self.lib = _lib.load_trace()
        dev, T, m, S = env.device, self.ticks, self.m, env.S
        z = lambda *shape, dt=env.dtype: torch.zeros(shape, dtype=dt, device=dev)   # noqa: E731
        self.ids_dev = torch.from_numpy(ids).to(dev)
        self.ring = dict(ships=z(T, m, S, 4), ships_b=z(T, m, S), planets=z(T, m, env.p_pad, 4),
                         bullets=z(T, m, env.b_cap, 4), hdr=z(T, m, 4, dt=torch.int32),
                         control=z(T, m, S, dt=torch.int8), reward=z(T, m, S, dt=torch.float32),
                         done=z(T, m, dt=torch.uint8))
        self.c = None
        if self.nout or not self.wants_q:
            self._bind()

    def _bind(self):
        """The AstroTrace of the ring (the Q array with it, once nout is known)."""
        if self.nout:
            self.ring['q'] = torch.zeros((self.ticks, self.m, self.env.S, self.nout), dtype=torch.float32,
                                         device=self.env.device)
        r = self.ring
        self.c = _lib.AstroTrace(
            ids=self.ids_dev.data_ptr(), ships=r['ships'].data_ptr(), ships_b=r['ships_b'].data_ptr(),
            planets=r['planets'].data_ptr(), bullets=r['bullets'].data_ptr(), hdr=r['hdr'].data_ptr(),
            control=r['control'].data_ptr(), q=r['q'].data_ptr() if self.nout else None,
            reward=r['reward'].data_ptr(), done=r['done'].data_ptr(), m=self.m, ticks=self.ticks, nout=self.nout,
            reserved=0)

    def state(self, control, q=None, played=None):
        """Before the step: the chosen envs' states, ``control`` (the int8 [N,
        S] tensor the step will take) and, for a recorder with ``q``, their
        rows of the float32 [N, S, nout] tensor ``q`` into the next free slot.
        played: a bool [S] or [m, S] array, True where a network played the
        ship (default: everywhere); only those get ``bot_data``."""
        env = self.env
        if self.open:
            raise RuntimeError('state() twice in a row: result() closes a slot')
        if self.fill >= self.ticks:
            raise RuntimeError('the ring is full (%d slots): drain() it' % self.ticks)
        if (not torch.is_tensor(control) or tuple(control.shape) != (env.n_env, env.S) or control.dtype != torch.int8
                or control.device != env.hdr.device or not control.is_contiguous()):
            raise ValueError('control must be a contiguous int8 [%d, %d] tensor on %s'
                             % (env.n_env, env.S, env.hdr.device))
        if (q is not None) != self.wants_q:
            raise ValueError('this recorder was made with q, so state() needs the Q values' if self.wants_q
                             else 'this recorder was made without q')
        if q is not None:
            if (not torch.is_tensor(q) or q.dim() != 3 or tuple(q.shape[:2]) != (env.n_env, env.S)
                    or q.dtype != torch.float32 or q.device != env.hdr.device or not q.is_contiguous()
                    or not 1 <= q.shape[2] <= _lib.TRACE_MAX_OUT):
                raise ValueError('q must be a contiguous float32 [%d, %d, nout <= %d] tensor on %s'
                                 % (env.n_env, env.S, _lib.TRACE_MAX_OUT, env.hdr.device))
            if self.c is None:
                self.nout = int(q.shape[2])
                self._bind()
            if q.shape[2] != self.nout:
                raise ValueError('q has nout %d, the ring %d' % (q.shape[2], self.nout))
        _lib.check_trace(self.lib.astro_trace_state(
            ctypes.byref(env.params), ctypes.byref(env.state), ctypes.byref(self.c), self.fill, control.data_ptr(),
            None if q is None else q.data_ptr(), _lib.stream_ptr(env.device)), 'astro_trace_state')
        self._played[self.fill] = True if played is None and q is not None else played
        self.open = True
        self._keep = (control, q)   # alive until the call has run

    def result(self, reward, done):
        """After the step: its ``reward`` (float32 [N, S]) and ``done`` (uint8 [N]) into the open slot."""
        env = self.env
        if not self.open:
            raise RuntimeError('result() without an open slot: call state() before the step')
        if (not torch.is_tensor(reward) or tuple(reward.shape) != (env.n_env, env.S) or reward.dtype != torch.float32
                or reward.device != env.hdr.device or not reward.is_contiguous()
                or not torch.is_tensor(done) or tuple(done.shape) != (env.n_env,) or done.dtype != torch.uint8
                or done.device != env.hdr.device or not done.is_contiguous()):
            raise ValueError('reward must be a contiguous float32 [%d, %d] tensor and done uint8 [%d], on %s'
                             % (env.n_env, env.S, env.n_env, env.hdr.device))
        _lib.check_trace(self.lib.astro_trace_result(
            ctypes.byref(self.c), self.fill, reward.data_ptr(), done.data_ptr(), env.n_env, env.S,
            _lib.stream_ptr(env.device)), 'astro_trace_result')
        self.open = False
        self.fill += 1

    def host(self, n=None):
        """The first ``n`` (default ``fill``) slots of every ring array as numpy (synchronises)."""
        n = self.fill if n is None else int(n)
        return {k: v[:n].cpu().numpy() for k, v in self.ring.items()}

    def drain(self):
        """Copy the filled slots to the host (synchronises), append them to
        their envs' open games and empty the ring.  Returns the games that
        finished in them as [(env_id, Game)]."""
        if self.open:
            raise RuntimeError('drain() with an open slot: result() closes it')
        n = self.fill
        if n == 0:
            return []
        skip = () if self.limit is None else {i for i in self.ids if len(self.games[i]) >= self.limit}
        finished, _ = decode(self.host(n), n, self.ids, self.env.schedule, self.env.config, self.env.S,
                             self._pending, self._played[:n], skip)
        self.fill = 0
        out = []
        for i, game in finished:
            if self.limit is None or len(self.games[i]) < self.limit:
                self.games[i].append(game)
                out.append((i, game))
        return out

    def save(self, directory):
        """``logs.save_log`` of every finished game, as ``<directory>/<env_id>_<k>.log``; returns the paths."""
        paths = []
        for i in self.ids:
            for k, game in enumerate(self.games[i]):
                paths.append(os.path.join(directory, '%d_%d.log' % (i, k)))
                _logs.save_log(paths[-1], game)
        return paths


def play(env, env_ids, policy, games=1, max_ticks=None, ticks=64):
    """``logs.record_games`` on the device: step ``env`` with ``policy`` (f(env)
    -> int8 [N, S] controls on the env's device) until each env of ``env_ids``
    has finished ``games`` games, from the envs' current states.  With
    auto-reset on these are the env's consecutive games; with it off ``games``
    must be 1.  The ring is drained, and the end looked for, every ``ticks``
    ticks.  Returns {env_id: [Game, ...]}."""
    games = int(games)
    if games < 1:
        raise ValueError('games must be >= 1, got %d' % games)
    if games > 1 and not env.auto_reset:
        raise ValueError('without auto-reset an env plays one game')
    rec = Recorder(env, env_ids, ticks=ticks, limit=games)
    limit = max_ticks if max_ticks is not None else games * (env.schedule.timeout_tick + 1) + rec.ticks
    t = 0
    while any(len(g) < games for g in rec.games.values()):
        if t >= limit:
            raise RuntimeError('record.play: games did not finish within %d ticks' % limit)
        for _ in range(rec.ticks):
            control = torch.as_tensor(policy(env), device=env.device).to(torch.int8).contiguous()
            rec.state(control)
            _, reward, done = env.step(control)
            rec.result(reward, done)
            t += 1
        rec.drain()
    return rec.games
