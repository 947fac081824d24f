"""CPU-only checks of the trace library's host side (libastro_trace.so's
argument codes) and of astro_amd/record.py's host half: ``decode`` against play-throughs of
the numpy oracle packed into the ring's layout by hand, the log round trip
with Q values, and the Recorder's argument checks that run before any device
call."""
import ctypes
import gzip
import json
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
import astro_amd
from astro_amd import (BatchedEnv, DEFAULT_CONFIG, SOLO_CONFIG, SOLO_EASY_CONFIG, _lib, logs, record,
                       schedule as _schedule)
from oracle import port
from tests import golden_io as gio
from tests import test_libraries as libraries

FIELDS = ('ids', 'ships', 'ships_b', 'planets', 'bullets', 'hdr', 'control', 'q', 'reward', 'done', 'm', 'ticks',
          'nout', 'reserved')


# ---------------------------------------------------------------------------
# the library: header, argument codes

def test_header_compiles_as_c99_and_the_struct_is_the_mirror(tmp_path):
    """AstroTrace, the two redeclared prototypes and ASTRO_TRACE_MAX_OUT: the trace row's layout, prototype
    and constants cases."""
    assert tuple(n for n, _ in _lib.AstroTrace._fields_) == FIELDS
    libraries.test_struct_layouts_are_the_ctypes_mirrors('trace', tmp_path)
    libraries.test_prototypes_agree_with_restype_and_argtypes('trace', tmp_path)
    libraries.test_header_constants_are_the_python_ones('trace', tmp_path)


def _params(**kw):
    d = dict(nships=2, solo=0, p_pad=4, max_planets=4, b_cap=32)
    d.update(kw)
    return _lib.AstroParams(**d)


def _state(**kw):
    d = dict(ships=0x1000, ships_b=0x2000, planets=0x3000, bullets=0x4000, hdr=0x5000, stream=0x6000, n_env=8,
             state_f64=0)
    d.update(kw)
    return _lib.AstroState(**d)


def _trace(**kw):
    d = dict(ids=0x10000, ships=0x11000, ships_b=0x12000, planets=0x13000, bullets=0x14000, hdr=0x15000,
             control=0x16000, q=0x17000, reward=0x18000, done=0x19000, m=3, ticks=4, nout=6)
    d.update(kw)
    return _lib.AstroTrace(**d)


def test_state_argument_codes_without_gpu():
    """Every argument code of astro_trace_state, in the documented order, with no
    device present (the pointers are not memory)."""
    entry.build()
    lib = _lib.load_trace()
    V = ctypes.c_void_p
    good = dict(p=_params(), s=_state(), t=_trace(), slot=0, c=V(0x20000), q=V(0x21000))

    def call(**kw):
        a = dict(good)
        a.update(kw)
        ref = lambda x: None if x is None else ctypes.byref(x)   # noqa: E731
        rc = lib.astro_trace_state(ref(a['p']), ref(a['s']), ref(a['t']), a['slot'], a['c'], a['q'], None)
        return rc, lib.astro_trace_last_error().decode()

    noq = dict(t=_trace(q=None, nout=0), q=None)
    cases = [
        (dict(p=None), -10, 'params'), (dict(s=None), -2, 'state'), (dict(t=None), -140, 'trace is NULL'),
        (dict(p=_params(nships=3)), -11, 'nships'), (dict(p=_params(nships=0)), -11, 'nships'),
        (dict(p=_params(p_pad=0)), -13, 'p_pad'), (dict(p=_params(p_pad=17)), -13, 'p_pad'),
        (dict(p=_params(b_cap=0)), -15, 'b_cap'), (dict(p=_params(b_cap=65536)), -15, 'b_cap'),
        (dict(t=_trace(m=0)), -141, 'trace.m'), (dict(t=_trace(m=-2)), -141, 'trace.m'),
        (dict(t=_trace(ticks=0)), -142, 'trace.ticks'),
        (dict(t=_trace(nout=-1)), -143, 'nout'), (dict(t=_trace(nout=7)), -143, 'nout'),
        (dict(slot=-1), -144, 'slot'), (dict(slot=4), -144, 'slot'),
        (dict(s=_state(n_env=-1)), -3, 'n_env'),
        (dict(t=_trace(q=None)), -146, 'trace.q'), (dict(t=_trace(nout=0)), -146, 'trace.q'),
        (dict(q=None), -145, 'q is NULL'), (dict(t=_trace(q=None, nout=0)), -145, 'q given'),
        (dict(c=None), -147, 'control'),
        (dict(t=_trace(ids=None)), -148, 'trace array'), (dict(t=_trace(bullets=None)), -148, 'trace array'),
        (dict(t=_trace(done=None)), -148, 'trace array'), (dict(t=_trace(reward=None)), -148, 'trace array'),
        (dict(s=_state(ships=None)), -4, 'NULL'), (dict(s=_state(stream=None)), -4, 'NULL'),
        (dict(s=_state(hdr=None)), -4, 'NULL'),
        (dict(s=_state(state_f64=2)), -6, 'state_f64'),
        (dict(s=_state(bullets=0x4008)), -5, 'aligned'), (dict(s=_state(ships_b=0x2002)), -5, 'aligned'),
        (dict(s=_state(ships_b=0x2004, state_f64=1)), -5, 'aligned'), (dict(s=_state(hdr=0x5004)), -5, 'aligned'),
        (dict(t=_trace(ships=0x11008)), -149, 'trace arrays'), (dict(t=_trace(hdr=0x15004)), -149, 'trace arrays'),
        (dict(t=_trace(q=0x17002)), -149, 'trace arrays'), (dict(t=_trace(ids=0x10001)), -149, 'trace arrays'),
        (dict(t=_trace(ships_b=0x12004), s=_state(state_f64=1)), -149, 'trace arrays'),
        (dict(q=V(0x21002)), -150, 'q must be'),
    ]
    codes = set()
    for kw, code, word in cases:
        rc, msg = call(**kw)
        assert rc == code and word in msg, (kw, rc, msg)
        codes.add(rc)
    assert sorted(codes) == [-150, -149, -148, -147, -146, -145, -144, -143, -142, -141, -140, -15, -13, -11, -10, -6,
                             -5, -4, -3, -2]
    # what is accepted up to the launch is not run here: a ring without q passes every check before -148
    assert call(t=_trace(q=None, nout=0, ids=None), q=None)[0] == -148
    # float bearings are aligned to 4 bytes (q is misaligned in these calls: no call here may reach the launch)
    assert call(s=_state(ships_b=0x2004), t=_trace(ships_b=0x12004), q=V(0x21002))[0] == -150
    # no envs: nothing to do, whatever the arrays are -- but only after the scalar checks
    empty = _state(n_env=0, ships=None, hdr=None)
    assert call(s=empty, t=_trace(ids=None))[0] == 0 and call(s=empty, **noq)[0] == 0
    assert call(s=empty, slot=9)[0] == -144 and call(s=empty, c=None)[0] == -147
    # the order: each call breaks the rule of its code and of every later one
    bad_t = dict(m=0, ticks=0, nout=9, q=None, ids=None, ships=0x11008)
    worst = dict(s=_state(n_env=-1, ships=None, state_f64=2, hdr=0x5004), slot=-1, c=None, q=V(0x21002))
    assert call(p=_params(nships=3, p_pad=0, b_cap=0), t=_trace(**bad_t), **worst)[0] == -11
    assert call(p=_params(p_pad=0, b_cap=0), t=_trace(**bad_t), **worst)[0] == -13
    assert call(p=_params(b_cap=0), t=_trace(**bad_t), **worst)[0] == -15
    assert call(t=_trace(**bad_t), **worst)[0] == -141
    bad_t.update(m=3)
    assert call(t=_trace(**bad_t), **worst)[0] == -142
    bad_t.update(ticks=4)
    assert call(t=_trace(**bad_t), **worst)[0] == -143
    bad_t.update(nout=6)
    assert call(t=_trace(**bad_t), **worst)[0] == -144
    worst.update(slot=3)
    assert call(t=_trace(**bad_t), **worst)[0] == -3
    worst.update(s=_state(ships=None, state_f64=2, hdr=0x5004))
    assert call(t=_trace(**bad_t), **worst)[0] == -146
    bad_t.update(nout=0)
    assert call(t=_trace(**bad_t), **worst)[0] == -145
    worst.update(q=None)
    assert call(t=_trace(**bad_t), **worst)[0] == -147
    worst.update(c=V(0x20000))
    assert call(t=_trace(**bad_t), **worst)[0] == -148
    bad_t.update(ids=0x10000)
    assert call(t=_trace(**bad_t), **worst)[0] == -4
    worst.update(s=_state(state_f64=2, hdr=0x5004))
    assert call(t=_trace(**bad_t), **worst)[0] == -6
    worst.update(s=_state(hdr=0x5004))
    assert call(t=_trace(**bad_t), **worst)[0] == -5
    worst.update(s=_state())
    assert call(t=_trace(**bad_t), **worst)[0] == -149
    assert call(t=_trace(ships=0x11008), q=V(0x21002))[0] == -149


def test_result_argument_codes_without_gpu():
    """The same for astro_trace_result."""
    entry.build()
    lib = _lib.load_trace()
    V = ctypes.c_void_p
    good = dict(t=_trace(), slot=3, r=V(0x20000), d=V(0x21001), n=8, S=2)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        rc = lib.astro_trace_result(None if a['t'] is None else ctypes.byref(a['t']), a['slot'], a['r'], a['d'],
                                    a['n'], a['S'], None)
        return rc, lib.astro_trace_last_error().decode()

    cases = [
        (dict(t=None), -140, 'trace is NULL'), (dict(S=0), -11, 'nships'), (dict(S=3), -11, 'nships'),
        (dict(t=_trace(m=0)), -141, 'trace.m'), (dict(t=_trace(ticks=-1)), -142, 'trace.ticks'),
        (dict(slot=4), -144, 'slot'), (dict(slot=-1), -144, 'slot'), (dict(n=-1), -3, 'n_env'),
        (dict(r=None), -151, 'reward or done'), (dict(d=None), -151, 'reward or done'),
        (dict(t=_trace(ids=None)), -148, 'trace array'), (dict(t=_trace(reward=None)), -148, 'trace array'),
        (dict(t=_trace(done=None)), -148, 'trace array'),
        (dict(t=_trace(ids=0x10002)), -149, 'aligned'), (dict(t=_trace(reward=0x18001)), -149, 'aligned'),
        (dict(r=V(0x20002)), -152, 'reward must be'),
    ]
    codes = set()
    for kw, code, word in cases:
        rc, msg = call(**kw)
        assert rc == code and word in msg, (kw, rc, msg)
        codes.add(rc)
    assert sorted(codes) == [-152, -151, -149, -148, -144, -142, -141, -140, -11, -3]
    # nout is astro_trace_state's to check, and the arrays it alone writes are not looked at
    assert call(t=_trace(nout=9, ships=None, q=None), n=0)[0] == 0
    assert call(t=_trace(ids=None), n=0)[0] == 0 and call(n=0, r=None)[0] == -151
    # the order
    bad = dict(m=0, ticks=0, ids=None, reward=0x18001)
    worst = dict(slot=7, n=-1, r=None)
    assert call(t=_trace(**bad), S=5, **worst)[0] == -11
    assert call(t=_trace(**bad), **worst)[0] == -141
    bad.update(m=3)
    assert call(t=_trace(**bad), **worst)[0] == -142
    bad.update(ticks=4)
    assert call(t=_trace(**bad), **worst)[0] == -144
    worst.update(slot=0)
    assert call(t=_trace(**bad), **worst)[0] == -3
    worst.update(n=8)
    assert call(t=_trace(**bad), **worst)[0] == -151
    worst.update(r=V(0x20002))
    assert call(t=_trace(**bad), **worst)[0] == -148
    bad.update(ids=0x10000)
    assert call(t=_trace(**bad), **worst)[0] == -149
    bad.update(reward=0x18000)
    assert call(t=_trace(**bad), **worst)[0] == -152


# ---------------------------------------------------------------------------
# record.decode against play-throughs of the oracle

P_PAD, B_CAP = 4, 48


def play_through(config, seed, rng, max_ticks=100000):
    """One game of the oracle under random controls: [(state, control, reward, done)] per tick, with the
    reward and done ``BatchedEnv.step`` reports (done 1 collision, 2 timeout) in the dtypes ``core.play`` logs."""
    g = port.Game(config._replace(seed=seed))
    st = g.create()
    out = []
    for _ in range(max_ticks):
        ctl = rng.randint(0, 6, size=g.ns)
        nxt, rew = g.step(st, ctl)
        done = 0 if nxt is not None else (1 if rew.dtype.kind == 'i' else 2)
        out.append((st, ctl, rew, done))
        if nxt is None:
            return out
        st = nxt
    raise AssertionError('the game did not end')


def pack(games, S, dtype=np.float64, nout=0, garbage=7):
    """The ticks of ``games`` -- per env a list of (seed, play_through) played back to back -- in the ring's
    layout, one env per column; shorter columns end in slots of an env that goes on (never decoded here:
    callers cut at the shortest).  Dead rows hold ``garbage``: the decoder must not look at them."""
    m = len(games)
    cols = [[(seed, k, tick) for seed, ticks in col for k, tick in enumerate(ticks)] for col in games]
    T = min(len(c) for c in cols)
    ring = dict(ships=np.zeros((T, m, S, 4), dtype), ships_b=np.zeros((T, m, S), dtype),
                planets=np.full((T, m, P_PAD, 4), garbage, dtype), bullets=np.full((T, m, B_CAP, 4), garbage, dtype),
                hdr=np.zeros((T, m, 4), np.int32), control=np.zeros((T, m, S), np.int8),
                reward=np.zeros((T, m, S), np.float32), done=np.zeros((T, m), np.uint8))
    if nout:
        ring['q'] = np.random.RandomState(5).randn(T, m, S, nout).astype(np.float32)
    for j, col in enumerate(cols):
        for t, (seed, k, (st, ctl, rew, done)) in enumerate(col[:T]):
            npl, nb = st.planets.x.shape[0], st.bullets.x.shape[0]
            assert npl <= P_PAD and nb <= B_CAP
            ring['ships'][t, j, :, 0:2], ring['ships'][t, j, :, 2:4] = st.ships.x, st.ships.dx
            ring['ships_b'][t, j] = st.ships.b
            ring['planets'][t, j, :npl, 0:2], ring['planets'][t, j, :npl, 2:4] = st.planets.x, st.planets.dx
            ring['bullets'][t, j, :nb, 0:2], ring['bullets'][t, j, :nb, 2:4] = st.bullets.x, st.bullets.dx
            ring['hdr'][t, j] = (k, npl | (nb << 16), seed, 0)
            ring['control'][t, j] = ctl
            ring['reward'][t, j] = rew
            ring['done'][t, j] = done
    return ring, T


def same_array(got, want, what):
    assert type(got) is np.ndarray and got.dtype == want.dtype and got.shape == want.shape, \
        (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), what


def same_state(got, want, what):
    """Values, dtypes and shapes, with one exception that has no values: a bullet array WITHOUT ROWS.  The
    play-through keeps create()'s empty float32 arrays until the first shot; ``BatchedEnv.state_of``, whose
    results are pinned and whose construction the decoder shares (so that it equals ``logs.record_games``),
    gives every array of a stepped game as float64.  For such an array the decoder must follow state_of."""
    for part in ('ships', 'planets', 'bullets'):
        g, w = getattr(got, part), getattr(want, part)
        if part == 'bullets' and w.x.shape[0] == 0:
            rule = np.float32 if want.t == 0 else np.float64
            assert g.x.shape == g.dx.shape == (0, 2) and g.x.dtype == g.dx.dtype == rule and g.b is None, what
            continue
        same_array(g.x, w.x, (what, part, 'x'))
        same_array(g.dx, w.dx, (what, part, 'dx'))
        if w.b is None:
            assert g.b is None
        else:
            same_array(g.b, w.b, (what, part, 'b'))
    assert type(got.reload) is float and type(got.t) is float
    assert got.reload == want.reload and got.t == want.t, (what, got.reload, want.reload, got.t, want.t)


def same_tick(got, played, S, what, q=None):
    st, ctl, rew, done = played
    same_state(got.state, st, what)
    same_array(got.control, ctl.astype(np.int64), (what, 'control'))
    want = {0: np.zeros(S, np.float32), 1: rew.astype(np.int64), 2: rew.astype(np.float32)}[done]
    same_array(got.reward, want, (what, 'reward'))
    assert rew.dtype == (np.float32 if done != 1 else np.int64)      # what the oracle itself hands back
    assert type(got.bot_data) is list and len(got.bot_data) == S
    for s in range(S):
        if q is None or q[s] is None:
            assert got.bot_data[s] is None
        else:
            assert list(got.bot_data[s]) == ['q']
            same_array(got.bot_data[s]['q'], q[s], (what, 'q'))


def same_game(game, config, seed, ticks, S, what):
    assert game.config == config._replace(seed=seed) and type(game.config.seed) is int
    last = ticks[-1]
    want = None if max(last[2]) < 1 else int(np.argmax(last[2]))
    assert game.winner == want and (want is None or type(game.winner) is int), (what, game.winner, want)
    assert len(game.ticks) == len(ticks)
    for k, (got, played) in enumerate(zip(game.ticks, ticks)):
        same_tick(got, played, S, (what, k))


def find_game(config, rng, want_done, planets=None, lo=3, hi=400):
    """The first seed whose game under rng's controls ends the wanted way (None: any) within [lo, hi] ticks."""
    for seed in range(1000, 1400):
        if planets is not None and astro_amd.config.create_nplanets(config, seed) != planets:
            continue
        ticks = play_through(config, seed, rng, hi + 1)
        if want_done in (None, ticks[-1][3]) and lo <= len(ticks) <= hi:
            return seed, ticks
    raise AssertionError('no such game')


SHORT = DEFAULT_CONFIG._replace(max_time=3.0)           # 150 ticks at most


@pytest.fixture(scope='module')
def collision():
    return find_game(SHORT, np.random.RandomState(1), 1, lo=20)


def decode_all(ring, n, ids, config, S, **kw):
    return record.decode(ring, n, ids, _schedule.build(config), config, S, **kw)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_decode_a_collision(collision, dtype):
    seed, ticks = collision
    assert ticks[-1][3] == 1 and any(t[0].bullets.x.shape[0] for t in ticks)
    if dtype is np.float32:       # a float32 env holds the float32 rounding of every value
        r32 = lambda a: None if a is None else a.astype(np.float32).astype(a.dtype)     # noqa: E731
        ticks = [(port.State(*[port.Bodies(r32(b.x), r32(b.dx), r32(b.b)) for b in st[:3]], st.reload, st.t), c, r, d)
                 for st, c, r, d in ticks]
    ring, T = pack([[(seed, ticks)]], 2, dtype)
    finished, pending = decode_all(ring, T, [17], SHORT, 2)
    assert [i for i, _ in finished] == [17] and pending == {17: []}
    same_game(finished[0][1], SHORT, seed, ticks, 2, 'collision')
    assert finished[0][1].ticks[0].state.ships.x.dtype == np.float32
    assert finished[0][1].ticks[1].state.ships.x.dtype == np.float64
    assert finished[0][1].ticks[-1].reward.dtype == np.int64 and set(finished[0][1].ticks[-1].reward) <= {-1, 1}


def test_decode_a_solo_timeout():
    cfg = SOLO_CONFIG._replace(max_time=1.0)
    seed, ticks = find_game(cfg, np.random.RandomState(2), 2)
    assert len(ticks) == _schedule.build(cfg).timeout_tick + 1
    ring, T = pack([[(seed, ticks)]], 1)
    finished, _ = decode_all(ring, T, [0], cfg, 1)
    same_game(finished[0][1], cfg, seed, ticks, 1, 'timeout')
    game = finished[0][1]
    assert game.winner == 0 and game.ticks[-1].reward.dtype == np.float32 and game.ticks[-1].reward[0] == 1
    assert game.ticks[-1].control.shape == (1,)


def test_decode_a_one_planet_game():
    for cfg, S in ((SHORT, 2), (SOLO_EASY_CONFIG._replace(max_time=1.0), 1)):
        seed, ticks = find_game(cfg, np.random.RandomState(3), None, planets=1)
        ring, T = pack([[(seed, ticks)]], S)
        finished, _ = decode_all(ring, T, [4], cfg, S)
        same_game(finished[0][1], cfg, seed, ticks, S, 'one planet')
        late = finished[0][1].ticks[-1].state
        assert late.planets.x.dtype == np.float32 and late.planets.dx.dtype == np.float32
        assert late.planets.x.shape == (1, 2) and late.ships.x.dtype == np.float64


@pytest.fixture(scope='module')
def two_envs(collision):
    """Two envs, each playing games back to back (auto-reset) for at least 320 ticks -- a game takes 150 at
    most, so the trace holds two whole games of each: env 3 the collision game, a timeout and more; env 9
    others.  Every game has its own seed."""
    rng = np.random.RandomState(4)

    def fill(col, seed):
        while sum(len(t) for _, t in col) < 320:
            col.append((seed, play_through(SHORT, seed, rng)))
            seed += 1
        return col
    a = fill([collision, find_game(SHORT, rng, 2)], 77)
    b = fill([(5, play_through(SHORT, 5, rng)), find_game(SHORT, rng, 1, lo=20)], 12345678)
    return a, b


def test_decode_consecutive_games(two_envs):
    a, b = two_envs
    ring, T = pack([a, b], 2, nout=6)
    finished, pending = decode_all(ring, T, [3, 9], SHORT, 2)
    for env_id, col in ((3, a), (9, b)):
        mine = [g for i, g in finished if i == env_id]
        ends = np.cumsum([len(ticks) for _, ticks in col])
        whole = [k for k in range(len(col)) if ends[k] <= T]          # the games that fit the trace
        assert len(mine) == len(whole) >= 2 and len({g.config.seed for g in mine}) == len(mine)
        for k in whole:
            seed, ticks = col[k]
            same_game(mine[k], SHORT, seed, ticks, 2, (env_id, k))
            if k:      # the next game's first tick is its create state
                same_state(mine[k].ticks[0].state, port.Game(SHORT._replace(seed=seed)).create(), 'create')
                assert mine[k].ticks[0].state.t == 0.0 and mine[k].ticks[0].state.ships.x.dtype == np.float32
        assert len(pending[env_id]) == T - ends[whole[-1]]
    # slot order: a game that ends earlier comes first
    ends = [sum(len(t) for _, t in col[:k + 1]) for col in (a, b) for k in range(len(col))]
    assert len(finished) == sum(e <= T for e in ends)


def test_decode_q_and_played(two_envs):
    a, b = two_envs
    ring, T = pack([a, b], 2, nout=6)
    n = 40
    who = np.array([[True, False], [True, True]])
    played = [None if t % 5 == 4 else (True if t % 5 == 3 else ([True, False] if t % 5 == 2 else who))
              for t in range(n)]
    _, pending = decode_all(ring, n, [3, 9], SHORT, 2, played=played)
    flat = {3: [x for _, ticks in a for x in ticks], 9: [x for _, ticks in b for x in ticks]}
    for j, env_id in enumerate((3, 9)):
        assert len(pending[env_id]) == n
        for t, got in enumerate(pending[env_id]):
            p = played[t]
            mask = [False, False] if p is None else ([True, True] if p is True else list(np.broadcast_to(p, (2, 2))[j]))
            same_tick(got, flat[env_id][t], 2, (env_id, t), q=[ring['q'][t, j, s] if mask[s] else None for s in (0, 1)])
    # without played, and without q in the ring, bot_data is None
    _, pending = decode_all(ring, 5, [3, 9], SHORT, 2)
    assert all(tk.bot_data == [None, None] for tk in pending[3])
    noq = {k: v for k, v in ring.items() if k != 'q'}
    _, pending = decode_all(noq, 5, [3, 9], SHORT, 2, played=[True] * 5)
    assert all(tk.bot_data == [None, None] for tk in pending[9])


def test_decode_in_three_drains_equals_one(two_envs):
    a, b = two_envs
    ring, T = pack([a, b], 2, nout=3)
    whole, left = decode_all(ring, T, [3, 9], SHORT, 2, played=[True] * T)
    for cuts in ((1, T - 1), (37, 38), (len(a[0][1]), len(a[0][1]) + 1), (T // 3, 2 * T // 3)):
        pending, got = {}, []
        for lo, hi in zip((0,) + cuts, cuts + (T,)):
            part = {k: v[lo:hi] for k, v in ring.items()}
            fin, pending = decode_all(part, hi - lo, [3, 9], SHORT, 2, pending=pending, played=[True] * (hi - lo))
            got += fin
        assert [i for i, _ in got] == [i for i, _ in whole]
        for (_, g), (_, w) in zip(got, whole):
            assert g.config == w.config and g.winner == w.winner and len(g.ticks) == len(w.ticks)
            for x, y in zip(g.ticks, w.ticks):
                same_state(x.state, y.state, cuts)
                same_array(x.control, y.control, cuts), same_array(x.reward, y.reward, cuts)
                same_array(x.bot_data[1]['q'], y.bot_data[1]['q'], cuts)
        assert {i: len(v) for i, v in pending.items()} == {i: len(v) for i, v in left.items()}


def test_decode_a_game_already_running(collision):
    seed, ticks = collision
    start = 11
    ring, T = pack([[(seed, ticks)]], 2)
    late = {k: v[start:] for k, v in ring.items()}
    finished, _ = decode_all(late, T - start, [0], SHORT, 2)
    game = finished[0][1]
    assert len(game.ticks) == len(ticks) - start and game.config.seed == seed
    for k, got in enumerate(game.ticks):
        same_tick(got, ticks[start + k], 2, k)
    assert game.ticks[0].state.t > 0 and game.ticks[0].state.ships.x.dtype == np.float64
    # skip: an env whose slots are not wanted
    finished, pending = decode_all(ring, T, [0], SHORT, 2, skip={0})
    assert finished == [] and pending == {}


# ---------------------------------------------------------------------------
# logs

def test_log_round_trip_with_q(collision, tmp_path):
    seed, ticks = collision
    ring, T = pack([[(seed, ticks)]], 2, nout=6)
    finished, _ = decode_all(ring, T, [0], SHORT, 2, played=[[True, False]] * T)
    game = finished[0][1]
    path = str(tmp_path / 'sub' / '0_0.log')
    logs.save_log(path, game)
    back = logs.load_log(path)
    assert back.config == game.config and back.winner == game.winner and len(back.ticks) == len(game.ticks)
    for t, (x, y) in enumerate(zip(back.ticks, game.ticks)):
        assert list(x.bot_data[0]) == ['q'] and x.bot_data[1] is None
        assert np.array_equal(x.bot_data[0]['q'], ring['q'][t, 0, 0].astype(np.float64)) and x.bot_data[0]['q'].shape == (6,)
        assert np.array_equal(x.control, y.control) and np.array_equal(x.reward, y.reward)
        for part in ('ships', 'planets', 'bullets'):
            assert np.array_equal(getattr(x.state, part).x, getattr(y.state, part).x)
            assert np.array_equal(getattr(x.state, part).dx, getattr(y.state, part).dx)
        assert np.array_equal(x.state.ships.b, y.state.ships.b) and (x.state.reload, x.state.t) == (y.state.reload, y.state.t)

    def shape(o):
        """The key structure of a JSON value: keys and nesting, not the numbers."""
        if isinstance(o, dict):
            return {k: (o[k] if k == '_type' else None if k in ('_values', '_shape') else shape(o[k])) for k in o}
        if isinstance(o, list):
            return [shape(v) for v in o]
        return None if o is None else type(o).__name__

    with gzip.open(os.path.join(gio.GOLDEN, 'log_short_nothing.jsonl.gz'), 'rt') as f:
        ref_header, ref_tick = json.loads(next(f)), json.loads(next(f))
    with open(path) as f:
        header, tick = json.loads(next(f)), json.loads(next(f))
    assert list(header) == list(ref_header) and list(header['config']) == list(ref_header['config'])
    want = shape(ref_tick)
    assert want['bot_data'] == [None, None]
    want['bot_data'] = [{'q': {'_values': None, '_shape': None}}, None]       # the one difference
    assert shape(tick) == want


# ---------------------------------------------------------------------------
# Recorder's argument checks: before any device call

def _bare_env(S=2, n_env=300, p_pad=4, b_cap=32):
    """A BatchedEnv that was never initialised: the checks read its shape only."""
    env = BatchedEnv.__new__(BatchedEnv)
    env.S, env.n_env, env.p_pad, env.b_cap = S, n_env, p_pad, b_cap
    return env


def test_recorder_value_errors_before_the_device():
    env = _bare_env()
    assert astro_amd.Recorder is record.Recorder and astro_amd.record is record
    for ids, word in (([], 'empty'), ([3, 5, 3], 'twice'), ([0, 300], 'outside'), ([-1], 'outside'),
                      ([1.5], 'integers'), (['a'], 'integers')):
        with pytest.raises(ValueError, match=word):
            record.Recorder(env, ids)
        with pytest.raises(ValueError, match=word):
            record.check_ring(300, ids, 64, 2, 4, 32)
    for ticks in (0, -4):
        with pytest.raises(ValueError, match='ticks'):
            record.Recorder(env, [0], ticks=ticks)
    for q in (7, -1):
        with pytest.raises(ValueError, match='nout'):
            record.Recorder(env, [0], q=q)
    # a ring array of more than 2^31 - 1 elements: bullets [ticks][m][b_cap][4]
    big = _bare_env(n_env=1 << 20, b_cap=65535)
    with pytest.raises(ValueError, match='int32'):
        record.Recorder(big, range(8192), ticks=64)
    assert 64 * 8192 * 65535 * 4 > 2 ** 31 - 1 >= 64 * 128 * 65535 * 4 - 1
    ids = record.check_ring(1 << 20, range(127), 64, 2, 4, 65535, 6)
    assert ids.dtype == np.int32 and ids.tolist() == list(range(127))
    assert record.check_ring(300, np.array([299, 0, 7]), 1, 1, 1, 1).tolist() == [299, 0, 7]
    assert record.check_ring(300, torch.tensor([5, 2]), 1, 1, 1, 1).tolist() == [5, 2]
    # play_q and validate take the argument (and refuse what is not this env's recorder before they play)
    import inspect
    assert 'record' in inspect.signature(BatchedEnv.play_q).parameters
    assert 'record' in inspect.signature(astro_amd.QTrainer.validate).parameters
    assert list(inspect.signature(record.play).parameters)[:5] == ['env', 'env_ids', 'policy', 'games', 'max_ticks']
    for games, auto in ((0, True), (2, False)):
        e = _bare_env()
        e.auto_reset = auto
        with pytest.raises(ValueError):
            record.play(e, [0], None, games=games)
