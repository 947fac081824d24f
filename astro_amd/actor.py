"""The acting side of astro/rl.py's trainer for a whole ``BatchedEnv``, on the
device (csrc/astro_actor.hip, include/astro_actor.h).

``EpsilonGreedy`` is rl.EpsilonGreedy (rl.py:10-29) as rl.QBotTrainer uses it
(rl.py:235-238, 253-254): not an independent coin per tick but a two-state
process per ship.  A ship that holds no random policy enters one with
probability ``1 - exp(-dt / t_in)`` per tick, takes one control from
``randint(0, 5)`` (0..4) and repeats it until it leaves with probability
``1 - exp(-dt / t_out)`` per tick; on a game's first tick nothing moves, so a
held policy carries over into the next game.  With the reference's 1.0 s and
0.1 s that is bursts of about 5.5 ticks, a tenth of the time.

What differs from the reference: numpy's random stream is not reproduced (the
words are the project's splitmix64 of global ship id, draw and seed,
``replay.random_words``), and the time between two ticks is the constant
``config.dt`` where the reference subtracts two accumulated floats -- a
last-place difference in a probability.

``Episodes`` is the per-game bookkeeping of core.play (core.py:377-410) and
rl.train's log (rl.py:352-369) from what ``BatchedEnv.step`` returns: winner
and length of every env's games, and running totals.

``explore_host`` and ``episodes_host`` restate the two kernels in numpy (the
tests' truth).
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from .replay import M64, random_words

ONE = 1 << 53


def thresholds(dt, t_in=1.0, t_out=0.1):
    """(stay_out, stay_in): ``ceil(exp(-dt / t) * 2**53)`` for t_in and t_out,
    the probability in units of 2**-53 that a ship without (with) a random
    policy keeps that state over one tick.  A 53-bit word k moves the state iff
    ``k >= stay``, i.e. with probability ``1 - stay / 2**53``.  ldexp and ceil
    are exact, so the only rounding is exp's.  t = inf gives 2**53 (never
    moves), t = 0 gives 0 (always moves)."""
    def stay(t):
        t = float(t)
        if t < 0 or math.isnan(t):
            raise ValueError('t_in and t_out must be >= 0')
        p = 0.0 if t == 0.0 else math.exp(-float(dt) / t)
        return int(math.ceil(math.ldexp(p, 53)))
    if not float(dt) > 0:
        raise ValueError('dt must be > 0')
    return stay(t_in), stay(t_out)


# ---------------------------------------------------------------------------
# the host models

def explore_host(policy, tick, control, draw, stay_out, stay_in, seed=0, env_offset=0, nrandom=5):
    """astro_explore in numpy, in place on ``policy`` and ``control`` (int8
    [N, S]); ``tick`` int [N] is each env's tick counter."""
    N, S = policy.shape
    with np.errstate(over='ignore'):
        ids = np.arange(N * S, dtype=np.uint64).reshape(N, S) + np.uint64((int(env_offset) * S) & M64)
        k = random_words(ids, seed, draw) >> np.uint64(11)
        w = random_words(ids + np.uint64(1 << 63), seed, draw)
    pick = (((w >> np.uint64(32)) * np.uint64(nrandom)) >> np.uint64(32)).astype(np.int8)
    live = (np.asarray(tick) != 0)[:, None]
    out = policy < 0
    enter = live & out & (k >= np.uint64(stay_out))
    leave = live & ~out & (k >= np.uint64(stay_in))
    policy[enter] = pick[enter]
    policy[leave] = -1
    held = policy >= 0
    control[held] = policy[held]


def new_episodes_host(n_env, nships, games):
    N, S, G = int(n_env), int(nships), int(games)
    return dict(length=np.zeros(N, np.int32), got=np.zeros(N, np.int32), winner=np.full((N, G), -2, np.int8),
                ticks=np.zeros((N, G), np.int32), wins=np.zeros((N, S), np.int32), finished=np.zeros(N, np.int32),
                tick_sum=np.zeros(N, np.int64))


def episodes_host(h, reward, done):
    """astro_episodes in numpy on ``new_episodes_host``'s arrays, in place:
    reward float32 [N, S], done [N] (nonzero = the game ended on this tick)."""
    reward = np.asarray(reward, dtype=np.float32)
    G = h['winner'].shape[1]
    h['length'] += 1
    for e in np.nonzero(np.asarray(done) != 0)[0]:
        mx = reward[e].max()
        w = int(np.argmax(reward[e])) if mx >= 1 else -1     # the first maximal ship (core.py:409)
        g = int(h['got'][e])
        if g < G:
            h['winner'][e, g] = w
            h['ticks'][e, g] = h['length'][e]
        if w >= 0:
            h['wins'][e, w] += 1
        h['finished'][e] += 1
        h['tick_sum'][e] += int(h['length'][e])
        h['got'][e] = g + 1
        h['length'][e] = 0


# ---------------------------------------------------------------------------
# the device objects

class EpsilonGreedy:
    """rl.EpsilonGreedy for every ship of ``env`` (see the module).  ``policy``
    is the int8 [N, S] device tensor of held controls (-1: none): what
    rl.QBotTrainer keeps as ``data['greedy']``.  ``apply(control, draw)``
    advances it by one tick and overrides the controls of the ships that hold
    one, in place; the words depend on (global ship id, draw, seed) only, so
    shards of one batch agree with the whole."""

    def __init__(self, env, t_in=1.0, t_out=0.1, seed=0, nrandom=5):
        nrandom = int(nrandom)
        if not 1 <= nrandom <= 6:
            raise ValueError('nrandom must be in [1, 6], got %d' % nrandom)
        self.env = env
        self.t_in, self.t_out, self.seed, self.nrandom = float(t_in), float(t_out), int(seed), nrandom
        self.stay_out, self.stay_in = thresholds(env.config.dt, t_in, t_out)
        self.policy = torch.full((env.n_env, env.S), -1, dtype=torch.int8, device=env.device)
        self.c = _lib.AstroExplore(policy=self.policy.data_ptr(), stay_out=self.stay_out, stay_in=self.stay_in,
                                   seed=self.seed & M64, env_offset=env.env_offset, nrandom=nrandom, reserved=0)

    def reset(self):
        """No ship holds a policy."""
        self.policy.fill_(-1)

    def apply(self, control, draw):
        """One tick: the transition of every ship whose env's tick is not 0,
        then ``control[held] = policy[held]``.  control: a contiguous int8
        [N, S] tensor on the env's device; returns it."""
        env = self.env
        if (not torch.is_tensor(control) or tuple(control.shape) != (env.n_env, env.S) or control.dtype != torch.int8
                or control.device != self.policy.device or not control.is_contiguous()):
            raise ValueError('control must be a contiguous int8 [%d, %d] tensor on %s'
                             % (env.n_env, env.S, self.policy.device))
        _lib.check_actor(_lib.load_actor().astro_explore(
            ctypes.byref(env.params), ctypes.byref(env.state), ctypes.byref(self.c), int(draw), control.data_ptr(),
            _lib.stream_ptr(env.device)), 'astro_explore')
        return control


class Episodes:
    """Winner and length of every env's next ``games`` games, from the reward
    and done of each ``env.step``.  Device tensors: ``winner`` int8 [N, games]
    (-1: no winner -- a draw or a timeout; -2: not played yet), ``ticks`` int32
    [N, games], ``got`` int32 [N] (games finished, counted past ``games``
    too), ``length`` int32 [N] (ticks of the open game, begun at the env's
    current tick counter), and the totals over all finished games ``wins``
    int32 [N, S], ``finished`` int32 [N], ``tick_sum`` int64 [N]."""

    def __init__(self, env, games=1):
        N, S, G = env.n_env, env.S, int(games)
        if G < 1:
            raise ValueError('games must be >= 1, got %d' % G)
        if N * G > 2 ** 31 - 1:
            raise ValueError('n_env * games = %d does not fit an int32' % (N * G))
        self.env, self.games, self.device = env, G, env.device
        dev = env.device
        self.length = torch.zeros(N, dtype=torch.int32, device=dev)
        self.got = torch.zeros(N, dtype=torch.int32, device=dev)
        self.winner = torch.full((N, G), -2, dtype=torch.int8, device=dev)
        self.ticks = torch.zeros((N, G), dtype=torch.int32, device=dev)
        self.wins = torch.zeros((N, S), dtype=torch.int32, device=dev)
        self.finished = torch.zeros(N, dtype=torch.int32, device=dev)
        self.tick_sum = torch.zeros(N, dtype=torch.int64, device=dev)
        self.c = _lib.AstroEpisodes(
            length=self.length.data_ptr(), got=self.got.data_ptr(), winner=self.winner.data_ptr(),
            ticks=self.ticks.data_ptr(), wins=self.wins.data_ptr(), finished=self.finished.data_ptr(),
            tick_sum=self.tick_sum.data_ptr(), n_env=N, nships=S, games=G, reserved=0)
        self.reset()

    def reset(self):
        """Forget every game; the open games have the length of the env's tick counters."""
        self.length.copy_(self.env.tick)
        self.got.zero_()
        self.winner.fill_(-2)
        for t in (self.ticks, self.wins, self.finished, self.tick_sum):
            t.zero_()

    def push(self, reward, done):
        """One tick: ``reward`` float32 [N, S] and ``done`` uint8 [N] as ``env.step`` returned them."""
        N, S = self.env.n_env, self.env.S
        if not (torch.is_tensor(reward) and reward.dtype == torch.float32 and reward.device == self.device
                and reward.is_contiguous()):
            reward = torch.as_tensor(reward, device=self.device).to(torch.float32).contiguous()
        if not (torch.is_tensor(done) and done.dtype == torch.uint8 and done.device == self.device
                and done.is_contiguous()):
            done = torch.as_tensor(done, device=self.device).to(torch.uint8).contiguous()
        if tuple(reward.shape) != (N, S) or tuple(done.shape) != (N,):
            raise ValueError('reward must be [%d, %d] and done [%d]' % (N, S, N))
        _lib.check_actor(_lib.load_actor().astro_episodes(
            ctypes.byref(self.c), reward.data_ptr(), done.data_ptr(), _lib.stream_ptr(self.device)), 'astro_episodes')
        self._keep = (reward, done)   # alive until the call has run

    def summary(self):
        """Over the recorded games: ``games``, ``wins`` (share won by each
        ship), ``none`` (share without a winner: draws and timeouts) and
        ``median_ticks``.  Synchronises."""
        w = self.winner.cpu().numpy()
        t = self.ticks.cpu().numpy()
        played = w > -2
        n = int(played.sum())
        S = self.env.S
        if n == 0:
            return dict(games=0, wins=[float('nan')] * S, none=float('nan'), median_ticks=float('nan'))
        return dict(games=n, wins=[float((w[played] == s).sum()) / n for s in range(S)],
                    none=float((w[played] == -1).sum()) / n, median_ticks=float(np.median(t[played])))
