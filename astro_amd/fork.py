"""Env state copied between slots on the device (libastro_fork.so,
include/astro_fork.h), and what is built on the copy:

``Fork``       a checked plan: env ``src_ids[j]`` of one ``BatchedEnv`` becomes
               env ``dst_ids[j]`` of another (or of the same), one launch per
               ``apply()``
``Snapshot``   the seven state arrays of a batch and nothing else: what
               ``BatchedEnv.snapshot()`` returns and ``restore()`` takes
``Lookahead``  a one-ply search bot: each of the six controls is tried in a
               copy of the game, a scripted bot plays the copy on for a
               horizon, and the control whose copy ends best is played;
               optionally a Q-network values the copies that do not end, and
               the other ship's six replies are tried too

A fork copies the current game (``game``), the future games (``stream``: the
pending seed, the generate_configs cursor and its MT19937 ring) or both; with
both, the destination steps bit for bit like the source from then on, through
every auto-reset.  That holds for controls that depend on the state alone --
given controls, 'script', 'nothing', a network.  The 'random' policy is keyed
by GLOBAL env id (``env_offset`` + index) and tick, not by the state: a fork
moves a game to another id, so under 'random' the copy draws other controls
and diverges from its source.
"""
import ctypes

import numpy as np
import torch

from . import _lib, search

MT_N = 624


def check_ids(n_src, n_dst, src_ids, dst_ids, same):
    """The pairs of a fork as two int32 numpy arrays, checked on the host as
    include/astro_fork.h's precondition asks (the library cannot: its ids live
    on the device).  ``src_ids`` / ``dst_ids``: integer sequences of one
    length, or None for the identity (0, 1, ...; both None: min(n_src, n_dst)
    pairs).  ValueError for unequal lengths, an id outside its env range, a
    destination named twice and, when ``same`` (both sides are the same
    arrays), a destination that is another pair's source.  A pair that names
    one env on both sides of the same arrays is a no-op and allowed."""
    def ids(x, what):
        if x is None:
            return None
        if torch.is_tensor(x):
            x = x.cpu().numpy()
        a = np.asarray(x)
        if a.ndim != 1:
            raise ValueError('%s must be a one-dimensional sequence' % what)
        if a.size and a.dtype.kind not in 'iu':
            raise ValueError('%s must hold integers' % what)
        return a.astype(np.int64)

    s, d = ids(src_ids, 'src_ids'), ids(dst_ids, 'dst_ids')
    if s is None and d is None:
        m = min(int(n_src), int(n_dst))
    else:
        m = len(s if s is not None else d)
    s = np.arange(m, dtype=np.int64) if s is None else s
    d = np.arange(m, dtype=np.int64) if d is None else d
    if len(s) != len(d):
        raise ValueError('src_ids and dst_ids have unequal lengths (%d and %d)' % (len(s), len(d)))
    for a, n, what in ((s, n_src, 'src'), (d, n_dst, 'dst')):
        if a.size and (a.min() < 0 or a.max() >= n):
            raise ValueError('%s_ids must be in [0, %d): an id is out of range' % (what, n))
    if np.unique(d).size != d.size:
        raise ValueError('dst_ids names a destination env twice (duplicate)')
    if same and m:
        # sources equal to destination j, other than pair j's own
        n = max(int(n_src), int(n_dst))
        used = np.bincount(s, minlength=n)[d] - (s == d)
        if (used > 0).any():
            j = int(np.nonzero(used > 0)[0][0])
            raise ValueError('src and dst are the same arrays and the pairs overlap: destination env %d '
                             '(pair %d) is another pair\'s source' % (int(d[j]), j))
    return s.astype(np.int32), d.astype(np.int32)


_SHAPE = ('device', 'dtype', 'S', 'p_pad', 'b_cap', 'config', 'planets_only')


class Fork:
    """A checked plan: for every j, env ``dst_ids[j]`` of ``dst`` becomes env
    ``src_ids[j]`` of ``src`` (``check_ids``' forms; None: the identity).
    ``src`` and ``dst`` are ``BatchedEnv`` s or ``Snapshot`` s that agree in
    device, dtype, S, p_pad, b_cap, config and planets_only (ValueError
    otherwise); their n_env may differ and they may be one object.  game: the
    current game; stream: the future games (module docstring).  The ids are
    checked and uploaded once; ``apply()`` is one launch (astro_fork) on the
    current torch stream.  Neither env's ``errors``, statistics, reward or
    done buffers are touched, and bullet rows past a source's count are not
    copied."""

    def __init__(self, src, dst, src_ids=None, dst_ids=None, game=True, stream=True):
        for name in _SHAPE:
            a, b = getattr(src, name), getattr(dst, name)
            if a != b:
                raise ValueError('src and dst differ in %s (%s and %s)' % (name, a, b))
        self.what = (_lib.FORK_GAME if game else 0) | (_lib.FORK_STREAM if stream else 0)
        if not self.what:
            raise ValueError('a fork copies the game, the stream or both')
        self.src, self.dst = src, dst
        identity = src_ids is None and dst_ids is None
        s, d = check_ids(src.n_env, dst.n_env, src_ids, dst_ids, src is dst)
        self.m = int(s.size)
        self.src_ids, self.dst_ids = s, d
        # (the identity passes no arrays: the kernel takes the pair's index)
        self._s = self._d = None
        if not identity and self.m:
            self._s = torch.from_numpy(s).to(src.device)
            self._d = torch.from_numpy(d).to(src.device)

    def apply(self):
        """The copy: one launch.  The destination's ``info()`` raises until its next step."""
        _lib.check_fork(_lib.load_fork().astro_fork(
            ctypes.byref(self.src.params), ctypes.byref(self.src.state), ctypes.byref(self.dst.state),
            None if self._s is None else self._s.data_ptr(), None if self._d is None else self._d.data_ptr(),
            self.m, self.what, _lib.stream_ptr(self.dst.device)), 'astro_fork')
        self.dst._last = False

    @property
    def bytes(self):
        """The bytes one ``apply()`` moves now, read plus written: per pair the
        hdr and stream words ``what`` names, with ``game`` the ships, bearings,
        p_pad planet slots and the source's LIVE bullet rows (read from its
        header here: synchronises), with ``stream`` the 2,496-byte ring."""
        src = self.src
        el = 8 if src.dtype == torch.float64 else 4
        per = 0
        live = 0
        if self.what & _lib.FORK_GAME:
            per += 8 + 4 + src.S * 5 * el + src.p_pad * 4 * el
            nb = ((src.hdr[:, 1] >> 16) & 0xffff).clamp(max=src.b_cap)
            ids = torch.from_numpy(self.src_ids.astype(np.int64)).to(src.device)
            live = int(nb[ids].sum().item()) * 4 * el
        if self.what & _lib.FORK_STREAM:
            per += 8 + 12 + MT_N * 4
        return 2 * (per * self.m + live)


class Snapshot:
    """The seven state arrays of a batch of an env's shape, uninitialised: no
    reset, no seed streams, no key table, nothing a step needs beyond the
    arrays -- a place for ``Fork`` to copy to and from."""

    def __init__(self, env):
        for name in _SHAPE + ('n_env',):
            setattr(self, name, getattr(env, name))
        self.params = env.params            # (a fork reads nships, p_pad and b_cap of it)
        N, S, dev, dt = self.n_env, self.S, self.device, self.dtype
        self.ships = torch.empty((S, N, 4), dtype=dt, device=dev)
        self.ships_b = torch.empty((S, N), dtype=dt, device=dev)
        self.planets = torch.empty((self.p_pad, N, 4), dtype=dt, device=dev)
        self.bullets = torch.empty((N, self.b_cap, 4), dtype=dt, device=dev)
        self.hdr = torch.empty((N, 4), dtype=torch.int32, device=dev)
        self.stream = torch.empty((N, 4), dtype=torch.int32, device=dev)
        self.stream_ring = torch.empty((N, MT_N), dtype=torch.int32, device=dev)
        self.state = _lib.AstroState(
            ships=self.ships.data_ptr(), ships_b=self.ships_b.data_ptr(), planets=self.planets.data_ptr(),
            bullets=self.bullets.data_ptr(), hdr=self.hdr.data_ptr(), stream=self.stream.data_ptr(),
            stream_ring=self.stream_ring.data_ptr(), n_env=N, state_f64=1 if dt == torch.float64 else 0, errors=None)
        self._last = None


class Lookahead:
    """A one-ply search player for ship ``ship`` of ``env``: it owns a scratch
    env of ``6 * n_env`` envs of the same shape and the fork plan env i ->
    scratch envs 6 i .. 6 i + 5.

    ``values()``: fork everything, one ``step`` in which ``ship`` plays
    control a in branch a and the other ship ``base``'s control on the copy,
    then ``rollout(horizon - 1, base)`` for every ship in one launch
    (auto-reset on), then one launch of the value reduction
    (``search.reduce``, include/astro_search.h).  A branch's value is
    ``discount ** t * reward[t, ship]`` at its FIRST done tick t < horizon, 0
    if it does not end.
    ``controls()``: ``base``'s own control for ``ship`` unless some control's
    value is strictly greater than that one's, then the first maximal one --
    so a horizon in which nothing ends plays exactly ``base``.

    base: a policy that depends on the state alone ('script', 'nothing'; under
    'random' the copies draw other controls than ``env`` would, see the module
    docstring).  script_args: ScriptBot's, for ``base``.

    leaf (keyword): a ``qnet.QNetwork`` for ``env.S`` ships with six outputs
    (ValueError otherwise).  A branch that does not end is then worth
    ``discount ** horizon * max_a Q(s_K, a)``, the network's view of ``ship``
    in the branch's last state (``scratch.qvalues`` in the per-ship form, one
    more launch, into ``leaf_q``, a buffer kept here), instead of 0.  ``leaf``
    is a plain attribute: a trainer may swap or refresh it between calls.

    reply (keyword; a two-ship env): the other ship's first control is
    searched too.  The scratch env has ``36 * n_env`` envs -- six times the
    state memory and six times the step and rollout work of the default, e.g.
    36,864 scratch envs for 1,024 -- with the plan env i -> 36 i .. 36 i + 35;
    in branch (a, o) = 36 i + 6 a + o ``ship`` plays a and the other ship o at
    the first step, ``base`` plays both from then on, and a control's value is
    its minimum over o."""

    NCONTROL = 6

    def __init__(self, env, ship=0, horizon=32, base='script', discount=0.995, script_args=None, *, leaf=None,
                 reply=False):
        from .env import BatchedEnv
        if not 0 <= int(ship) < env.S:
            raise ValueError('ship must be in [0, %d), got %s' % (env.S, ship))
        if int(horizon) < 1:
            raise ValueError('horizon must be >= 1, got %s' % horizon)
        if reply and env.S != 2:
            raise ValueError('reply needs a two-ship env')
        if leaf is not None:
            from .qnet import QNetwork
            if not isinstance(leaf, QNetwork) or leaf.nships != env.S or leaf.nout != self.NCONTROL:
                raise ValueError('leaf must be a QNetwork for %d ships with %d outputs' % (env.S, self.NCONTROL))
        self.env, self.ship, self.horizon, self.base = env, int(ship), int(horizon), base
        self.discount, self.script_args = float(discount), script_args
        self.leaf, self.reply = leaf, bool(reply)
        A, N = self.NCONTROL, env.n_env
        R = self.replies = A if self.reply else 1
        kernel = [k for k, v in _lib.KERNELS.items() if v == env.params.kernel][0]
        self.scratch = BatchedEnv(env.config, N * A * R, device=env.device, b_cap=env.b_cap, p_pad=env.p_pad,
                                  dtype=env.dtype, env_offset=env.env_offset, auto_reset=True, kernel=kernel,
                                  use_key_table=env.key_table is not None, planets_only=env.planets_only,
                                  mem=env.mem)
        self.plan = Fork(env, self.scratch, np.repeat(np.arange(N), A * R), np.arange(N * A * R))
        m = torch.arange(N * A * R, device=env.device)
        self._branch = (m // R % A).to(torch.int8)
        self._reply = (m % R).to(torch.int8) if self.reply else None
        self._gamma = torch.from_numpy(search.gammas(self.discount, self.horizon)).to(env.device)
        self.leaf_q = None

    def _search(self, own):
        """The branched step and rollout, reduced: ``search.reduce``'s result."""
        sc = self.scratch
        self.plan.apply()
        c = sc.controls(self.base, script_args=self.script_args)
        c[:, self.ship] = self._branch
        if self.reply:
            c[:, 1 - self.ship] = self._reply
        self._first_control = c
        _, r0, d0 = sc.step(c, auto_reset=True)
        r = d = None
        if self.horizon > 1:
            r, d = sc.rollout(self.horizon - 1, self.base, auto_reset=True, script_args=self.script_args)
        q = None
        if self.leaf is not None:
            if self.leaf_q is None:
                self.leaf_q = torch.zeros((sc.n_env, sc.S, self.NCONTROL), dtype=torch.float32, device=sc.device)
            nets = [None] * sc.S
            nets[self.ship] = self.leaf
            q = sc.qvalues(nets, out=self.leaf_q)
        self._outputs = (r0, d0, r, d, q)      # (alive until the launch has run; what the tests reduce again)
        return search.reduce(r0, d0, r, d, gamma=self._gamma, ship=self.ship, replies=self.replies, leaf=q, own=own)

    def _own(self):
        return self.env.controls(self.base, script_args=self.script_args)[:, self.ship].contiguous()

    def values(self):
        """float32 [N, 6]: the value of each control for ``ship`` now."""
        return self._search(None)

    def controls(self, values=None):
        """int8 [N]: the control ``ship`` plays now (deterministic).  values:
        the tensor ``values()`` just returned for this state -- the decision is
        then taken on it (a few torch ops) instead of searching again."""
        if values is None:
            return self._search(self._own())[1]
        v = values
        own = self._own().to(torch.int64)
        best, arg = v.max(1).values, v.argmax(1)    # argmax: the first maximal control
        return torch.where(best > v.gather(1, own[:, None])[:, 0], arg, own).to(torch.int8)

    def play(self, opponent='script', games=1, max_ticks=None, record=None):
        """``env.play``'s (winner int64 [N, games], length int64 [N, games]):
        every env plays its next ``games`` games from its current state, each
        tick ``controls()`` for ``ship`` and ``env.controls(opponent)`` for the
        other ship (a two-ship env), pushed to an ``actor.Episodes`` as
        ``play_q`` does; the device count of finished games is read every 64
        ticks only.  record: a ``record.Recorder`` of ``env`` made with ``q=6``
        and at least 64 slots -- every tick is recorded with the search's six
        values as ``ship``'s Q values (``bot_data``; the other ship has none),
        and the ring is drained every 64 ticks, where the loop synchronises
        anyway; the games end up in ``record.games``."""
        from . import actor
        env, G = self.env, int(games)
        q_out = played = None
        if record is not None:
            if getattr(record, 'env', None) is not env:
                raise ValueError('record must be a Recorder of this env')
            if record.ticks < 64:
                raise ValueError('play drains the recorder every 64 ticks: it needs ticks >= 64, got %d' % record.ticks)
            if not record.wants_q or record.nout != self.NCONTROL:
                raise ValueError('record must be made with q=%d: the search has %d values' % ((self.NCONTROL,) * 2))
            q_out = torch.zeros((env.n_env, env.S, self.NCONTROL), dtype=torch.float32, device=env.device)
            played = [s == self.ship for s in range(env.S)]
        ep = actor.Episodes(env, G)
        limit = max_ticks if max_ticks is not None else G * (env.schedule.timeout_tick + 1) + 64
        t = 0
        while True:
            if t >= limit:
                raise RuntimeError('Lookahead.play: games did not finish within %d ticks' % limit)
            for _ in range(64):
                c = env.controls(opponent, tick0=t) if env.S > 1 else \
                    torch.empty((env.n_env, 1), dtype=torch.int8, device=env.device)
                v, mine = self._search(self._own())
                c[:, self.ship] = mine
                if record is not None:
                    q_out[:, self.ship] = v
                    record.state(c, q_out, played)
                _, r, d = env.step(c, auto_reset=True)
                if record is not None:
                    record.result(r, d)
                ep.push(r, d)
                t += 1
            if record is not None:
                record.drain()
            if int(ep.got.min()) >= G:
                break
        return ep.winner.to(torch.int64), ep.ticks.to(torch.int64)
