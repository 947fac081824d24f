"""CPU-only checks of the seats library's host side (libastro_seats.so's
argument codes), of the reference fixture for non-default ScriptBot arguments
(tests/golden/script_args.npz), of ``league.Script`` / ``Seats`` / ``mutate`` /
``tune_script`` and of the argument rules of the new ``QTrainer(opponent=)``
forms that run before any device call."""
import ctypes

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
import astro_amd
from astro_amd import BatchedEnv, _lib, bots, league, train
from astro_amd.core import roll_ships
from tests import golden_io as gio
from tests.test_oracle_golden import _state_from_row
from tests.test_pool_host import _Buf, _bare_net, _c_spans

CFG = gio.configs()
ARG_SETS = [(0.0, 0.45), (0.3, 0.45), (0.1, 0.05), (0.1, 1.5), (-0.1, 0.9), (0.2371, 0.3119)]


def _bare_env(S=2, n_env=10, cfg='default'):
    """A BatchedEnv that was never initialised: the checks read S, n_env, hdr.device and config only."""
    env = BatchedEnv.__new__(BatchedEnv)
    env.S, env.n_env, env.hdr, env.config = S, n_env, torch.zeros(1), CFG[cfg]
    return env


# ---------------------------------------------------------------------------
# the fixture

def test_fixture_is_the_six_sets_and_differs_from_the_default():
    z = gio.load('script_args.npz')
    default = gio.load('script_controls.npz')['control']
    assert z['args'].tolist() == [list(a) for a in ARG_SETS]
    assert z['control'].shape == (6,) + default.shape and z['control'].dtype == np.int8
    for a in range(6):
        assert ((z['control'][a] < 0) == (default < 0)).all()           # the same ships exist
        assert int((z['control'][a] != default).sum()) >= 100, a


def test_host_scriptbot_equals_the_fixture_for_all_six_sets():
    tr = gio.Transitions('steps.npz')
    want = gio.load('script_args.npz')['control']
    checked = 0
    for name, idx in tr.groups():
        cfg = CFG[name]
        S = 1 if cfg.solo else 2
        players = [bots.ScriptBot(dict(avoid_distance=d, avoid_threshold=t), cfg) for d, t in ARG_SETS]
        for i in idx:
            state = _state_from_row(tr, i, S)
            views = [roll_ships(state, k) for k in range(S)]
            for a, bot in enumerate(players):
                got = [bot(v) for v in views]
                assert got == want[a, i, :S].tolist(), (name, i, a)
            checked += S
    assert checked > 15000


def test_mutate_reproduces_the_recorded_chain():
    z = gio.load('script_args.npz')
    chain = z['mutate_chain']
    random = np.random.RandomState(int(z['mutate_seed']))
    args = league.Script().args
    assert args == bots.ScriptBot.DEFAULT_ARGS and [args['avoid_distance'], args['avoid_threshold']] == chain[0].tolist()
    for want in chain[1:]:
        before = dict(args)
        new = league.mutate(args, float(z['mutate_scale']), random)
        assert args == before and new is not args                                   # a copy, as the reference's
        args = new
        assert [args['avoid_distance'], args['avoid_threshold']] == want.tolist()  # bit for bit
    assert len(chain) == 9


# ---------------------------------------------------------------------------
# the library's argument codes

def test_header_compiles_as_c_and_its_constants_are_the_bindings(tmp_path):
    from tests import test_libraries as libraries
    libraries.test_prototypes_agree_with_restype_and_argtypes('seats', tmp_path)
    libraries.test_header_constants_are_the_python_ones('seats', tmp_path)
    libraries.test_struct_layouts_are_the_ctypes_mirrors('seats', tmp_path)
    assert ctypes.sizeof(_lib.AstroSeat) == 32 and _lib.SEATS_MAX == 64
    assert libraries.run_c('seats', tmp_path, ['printf("%d\\n", ASTRO_SEATS_MAX);']) == [64]


def test_argument_codes_without_gpu():
    """Every argument code of astro_controls_seats, in the documented order, with
    no device present (the pointers are not memory)."""
    entry.build()
    lib = _lib.load_seats()
    V = ctypes.c_void_p

    def params(**kw):
        d = dict(nships=2, solo=0, p_pad=4, max_planets=4, b_cap=32)
        d.update(kw)
        return _lib.AstroParams(**d)

    def state(**kw):
        d = dict(ships=0x1000, ships_b=0x2000, planets=0x3000, bullets=0x4000, hdr=0x5000, n_env=100, state_f64=0)
        d.update(kw)
        return _lib.AstroState(**d)

    def seats(*rows):   # (ship, bot, lo, hi)
        return (_lib.AstroSeat * len(rows))(*[_lib.AstroSeat(r[0], r[1], r[2], r[3], 0.04, 0.45) for r in rows])

    good = dict(p=params(), s=state(), b=_lib.AstroPolicy(), t=seats((0, 1, 0, 100), (1, 2, 0, 50)), n=2, c=V(0x8000))

    def call(**kw):
        a = dict(good)
        a.update(kw)
        if 't' in kw and 'n' not in kw and a['t'] is not None:
            a['n'] = len(a['t'])
        rc = lib.astro_controls_seats(None if a['p'] is None else ctypes.byref(a['p']),
                                      None if a['s'] is None else ctypes.byref(a['s']),
                                      None if a['b'] is None else ctypes.byref(a['b']), a['t'], a['n'], a['c'], None)
        return rc, lib.astro_seats_last_error().decode()

    cases = [
        (dict(p=None), -10, 'params'), (dict(s=None), -2, 'state'), (dict(b=None), -140, 'base is NULL'),
        (dict(t=None), -141, 'seats is NULL'),
        (dict(p=params(nships=3)), -11, 'nships'), (dict(p=params(nships=0)), -11, 'nships'),
        (dict(p=params(p_pad=0)), -13, 'p_pad'), (dict(p=params(p_pad=17)), -13, 'p_pad'),
        (dict(p=params(b_cap=0)), -15, 'b_cap'), (dict(p=params(b_cap=65536)), -15, 'b_cap'),
        (dict(n=0), -142, 'nseats'), (dict(n=65), -142, 'nseats'), (dict(n=-1), -142, 'nseats'),
        (dict(s=state(n_env=-1)), -3, 'n_env'),
        (dict(t=seats((2, 1, 0, 1))), -143, 'seats[0].ship'), (dict(t=seats((0, 1, 0, 1), (-1, 1, 0, 1))), -143, 'seats[1]'),
        (dict(p=params(nships=1), t=seats((1, 1, 0, 1))), -143, 'ship'),
        (dict(t=seats((0, 3, 0, 1))), -144, 'seats[0].bot'), (dict(t=seats((0, 0, 0, 1), (1, -2, 0, 1))), -144, 'seats[1]'),
        (dict(t=seats((0, 1, -1, 1))), -145, 'lo <= hi'), (dict(t=seats((0, 1, 5, 4))), -145, 'lo <= hi'),
        (dict(t=seats((0, 1, 0, 101))), -145, 'n_env'),
        (dict(t=seats((0, 1, 0, 10), (0, 2, 9, 20))), -146, 'overlap'),
        (dict(t=seats((1, 0, 0, 10), (0, 0, 0, 10), (1, -1, 5, 6))), -146, 'seats[0] and seats[2]'),
        (dict(c=None), -147, 'control is NULL'),
        (dict(s=state(ships=None)), -4, 'NULL'), (dict(s=state(hdr=None)), -4, 'NULL'),
        (dict(s=state(bullets=0x4008)), -5, 'aligned'), (dict(s=state(hdr=0x5004)), -5, 'aligned'),
        (dict(s=state(state_f64=2)), -6, 'state_f64'),
    ]
    codes = set()
    for kw, code, word in cases:
        rc, msg = call(**kw)
        assert rc == code and word in msg, (kw, rc, msg)
        codes.add(rc)
    assert sorted(codes) == [-147, -146, -145, -144, -143, -142, -141, -140, -15, -13, -11, -10, -6, -5, -4, -3, -2]
    last = dict(s=state(state_f64=2))                                   # the last code: everything before it passed
    # what does not overlap: touching seats, empty seats anywhere, the same envs of the other ship
    assert call(t=seats((0, 1, 0, 50), (0, 1, 50, 100), (1, 1, 0, 100)), **last)[0] == -6
    assert call(t=seats((0, 1, 0, 100), (0, 1, 30, 30), (0, -1, 100, 100), (0, 2, 0, 0)), **last)[0] == -6
    # nothing to do returns 0 whatever the pointers are -- but only after the scalar checks
    empty = state(n_env=0, ships=None, hdr=None)
    assert call(s=empty, t=seats((0, 1, 0, 0), (1, 2, 0, 0)))[0] == 0
    assert call(s=empty, t=seats((0, 1, 0, 0)), c=None)[0] == -147
    assert call(s=empty)[0] == -145                                     # the good seats do not fit zero envs
    idle = dict(s=state(ships=None, state_f64=2))
    assert call(t=seats((0, 1, 7, 7), (1, -1, 0, 100), (0, -1, 50, 60), (1, 2, 100, 100)), **idle)[0] == 0
    assert call(t=seats((0, -1, 0, 100)), **idle)[0] == 0
    # a solo env; 64 seats
    assert call(p=params(nships=1), t=seats((0, 1, 0, 40), (0, 0, 40, 100)), **last)[0] == -6
    assert call(t=seats(*[(k % 2, k % 3, (k // 2) * 3, (k // 2) * 3 + 3) for k in range(64)]), **last)[0] == -6
    # the order: each call breaks the rule of its code and of every later one
    worst = dict(s=state(n_env=-1, ships=None, state_f64=2), c=None, n=0, t=seats((5, 9, 3, 2), (5, 9, 3, 2)))
    assert call(p=params(nships=3, p_pad=0, b_cap=0), **worst)[0] == -11
    assert call(p=params(p_pad=0, b_cap=0), **worst)[0] == -13
    assert call(p=params(b_cap=0), **worst)[0] == -15
    assert call(**worst)[0] == -142
    worst.update(n=2)
    assert call(**worst)[0] == -3
    worst.update(s=state(n_env=10, ships=None, state_f64=2))
    assert call(**worst)[0] == -143
    worst.update(t=seats((0, 9, 3, 2), (0, 9, 3, 2)))
    assert call(**worst)[0] == -144
    worst.update(t=seats((0, 1, 3, 2), (0, 1, 3, 2)))
    assert call(**worst)[0] == -145
    worst.update(t=seats((0, 1, 2, 5), (0, 1, 4, 6)))
    assert call(**worst)[0] == -146
    worst.update(t=seats((0, 1, 2, 5), (1, 1, 4, 6)))
    assert call(**worst)[0] == -147
    worst.update(c=V(0x8000))
    assert call(**worst)[0] == -4
    worst.update(s=state(n_env=10, planets=0x3004, state_f64=2))
    assert call(**worst)[0] == -5
    worst.update(s=state(n_env=10, state_f64=2))
    assert call(**worst)[0] == -6


# ---------------------------------------------------------------------------
# league.Script and league.Seats

def test_script_is_a_checked_immutable_value():
    s = league.Script()
    assert s.args == dict(avoid_distance=0.1, avoid_threshold=0.45) == bots.ScriptBot.DEFAULT_ARGS
    t = league.Script(0.3, avoid_threshold=1)
    assert t.args == dict(avoid_distance=0.3, avoid_threshold=1.0) and type(t.avoid_threshold) is float
    assert t == league.Script(0.3, 1.0) and t != s and hash(t) == hash(league.Script(0.3, 1.0)) and 'Script(' in repr(t)
    assert astro_amd.Script is league.Script and astro_amd.Seats is league.Seats
    assert astro_amd.mutate is league.mutate and astro_amd.tune_script is league.tune_script
    for name in ('avoid_distance', 'avoid_threshold', 'other'):
        with pytest.raises(AttributeError):
            setattr(s, name, 1.0)
    for bad in (('a', 0.45), (0.1, None), (float('nan'), 0.45), (0.1, float('inf')), (True, 0.45)):
        with pytest.raises(ValueError, match='finite numbers'):
            league.Script(*bad)


def _c_seats(seats):
    return [(s.ship, s.bot, s.lo, s.hi, s.script_r2, s.script_threshold) for s in seats._seats]


def test_seats_is_checked_and_immutable():
    env = _bare_env()
    c = env.config
    a, b = _bare_net(), _bare_net()
    odd = league.Script(0.3, 0.9)
    r2 = lambda d: (c.planet_radius + c.ship_radius + d) ** 2   # noqa: E731
    seats = league.Seats(env, [a, 'script', odd, 'nothing', 'random', b],
                         [(0, 0, 10, 0), (1, 0, 2, 1), (1, 2, 4, 2), (1, 4, 5, 3), (1, 5, 6, 4), (1, 6, 6, 2),
                          (1, 6, 8, None), (1, 8, 10, 5)])
    assert seats.players == (a, league.Script(), odd, 'nothing', 'random', b) and len(seats.spans) == 8
    assert seats.spans[6] == (1, 6, 8, None) and not seats.covered and seats.nout == 6
    assert (seats.n_env, seats.S, seats.device) == (10, 2, torch.device('cpu'))
    assert type(seats.pool) is league.Pool and seats.pool.nets == (a, b)
    assert seats.pool.spans == ((0, 0, 10, 0), (1, 6, 8, None), (1, 8, 10, 1))
    assert _c_seats(seats) == [(1, 1, 0, 2, r2(0.1), 0.45), (1, 1, 2, 4, r2(0.3), 0.9), (1, 0, 4, 5, r2(0.1), 0.45),
                               (1, 2, 5, 6, r2(0.1), 0.45), (1, 1, 6, 6, r2(0.3), 0.9)]
    for name in ('spans', 'players', 'pool', 'covered', 'other'):
        with pytest.raises(AttributeError):
            setattr(seats, name, ())
    # scripted players only: no pool, no nout; a span without a player is a skipped seat
    bare = league.Seats(env, ['script', odd], [(0, 0, 10, 0), (1, 0, 5, 1), (1, 5, 10, None)])
    assert bare.pool is None and bare.nout is None and not bare.covered
    assert [s[:4] for s in _c_seats(bare)] == [(0, 1, 0, 10), (1, 1, 0, 5), (1, -1, 5, 10)]
    assert league.Seats(env, ['script', odd], [(1, 5, 10, 1), (0, 0, 10, 0), (1, 5, 5, None), (1, 0, 5, 0)]).covered
    assert not league.Seats(env, ['script'], [(0, 0, 10, 0)]).covered
    assert not league.Seats(env, ['script'], [(0, 0, 10, 0), (1, 1, 10, 0)]).covered
    assert league.Seats(_bare_env(S=1, cfg='solo'), ['script'], [(0, 0, 10, 0)]).covered
    # a network that plays twice is one network of the pool
    twice = league.Seats(env, [a, 'nothing', a], [(0, 0, 10, 0), (1, 0, 5, 2), (1, 5, 10, 1)])
    assert twice.pool.nets == (a,) and twice.pool.spans == ((0, 0, 10, 0), (1, 0, 5, 0)) and twice.covered
    # the limits: 64 scripted seats next to 64 network spans
    many = [(k % 2, (k // 2) * 3, (k // 2) * 3 + 3, k % 2) for k in range(128)]
    big = league.Seats(_bare_env(n_env=192), [a, 'script'], many)
    assert len(big._seats) == 64 and len(big.pool.spans) == 64 and big.covered
    bad = [
        (([], [(0, 0, 10, 0)]), 'at least one player'),
        ((['scripted'], [(0, 0, 10, 0)]), 'a player is'), (([None], [(0, 0, 10, 0)]), 'a player is'),
        (([dict(avoid_distance=0.1)], [(0, 0, 10, 0)]), 'a player is'),
        (([a, _bare_net(weights=torch.zeros(1, device='meta'))], [(0, 0, 10, 0), (1, 0, 10, 1)]), 'env on'),
        (([a, _bare_net(nships=1)], [(0, 0, 10, 0), (1, 0, 10, 1)]), 'ships'),
        (([a, _bare_net(nout=3)], [(0, 0, 10, 0), (1, 0, 10, 1)]), 'nout'),
        ((['script'], []), 'at least one span'),
        ((['script'], [(0, 0, 0, 0)] * 65), 'at most 64 scripted seats'),
        (([a], [(0, 0, 0, 0)] * 65), 'spans'), (([_bare_net() for _ in range(33)], [(0, 0, 0, k) for k in range(33)]), 'networks'),
        ((['script'], [(0, 0, 10)]), 'span is'), ((['script'], [(0, 0, 10, 'a')]), 'span is'),
        ((['script'], [(0, 0.5, 10, 0)]), 'span is'), ((['script'], [(0, 0, 10, True)]), 'span is'), ((['script'], [7]), 'span is'),
        ((['script'], [(2, 0, 10, 0)]), 'ship'), ((['script'], [(-1, 0, 10, 0)]), 'ship'),
        ((['script'], [(0, 0, 10, 1)]), 'player'), ((['script'], [(0, 0, 10, -1)]), 'player'),
        ((['script'], [(0, -1, 10, 0)]), 'lo <= hi'), ((['script'], [(0, 6, 5, 0)]), 'lo <= hi'),
        ((['script'], [(0, 0, 11, 0)]), 'lo <= hi'),
        ((['script', a], [(0, 0, 6, 0), (0, 5, 10, 1)]), 'overlap'), ((['script'], [(1, 0, 10, 0), (1, 3, 4, None)]), 'overlap'),
    ]
    for (players, spans), word in bad:
        with pytest.raises(ValueError, match=word):
            league.Seats(env, players, spans)
    with pytest.raises(ValueError, match='ship'):
        league.Seats(_bare_env(S=1, cfg='solo'), ['script'], [(1, 0, 10, 0)])


def test_seats_of_networks_only_builds_the_pools_tables():
    env = _bare_env()
    a, b, c = _bare_net(), _bare_net(), _bare_net()
    spans = [(0, 0, 10, 0), (1, 0, 1, 1), (1, 1, 4, 0), (1, 4, 4, 2), (1, 4, 8, None), (1, 8, 10, 2)]
    seats, pool = league.Seats(env, [a, b, c], spans), league.Pool(env, [a, b, c], spans)
    assert seats._seats is None and seats.pool.nets == pool.nets and seats.pool.spans == pool.spans == seats.spans
    assert _c_spans(seats.pool) == _c_spans(pool) and seats.covered == pool.covered and seats.nout == pool.nout
    assert [(n.weights, n.nships, n.nout) for n in seats.pool._nets] == [(n.weights, n.nships, n.nout) for n in pool._nets]
    for N, K in ((10, 3), (7, 4), (100, 8)):
        env, rivals = _bare_env(n_env=N), [_bare_net() for _ in range(K)]
        s, p = league.Seats.versus(env, a, rivals), league.Pool.versus(env, a, rivals)
        assert s._seats is None and s.spans == p.spans == s.pool.spans and _c_spans(s.pool) == _c_spans(p) and s.covered
    for N, M in ((96, 3), (7, 3), (31, 6)):
        env, nets = _bare_env(n_env=N), [_bare_net() for _ in range(M)]
        s, p = league.Seats.pairings(env, nets), league.Pool.pairings(env, nets)
        assert s._seats is None and s.spans == p.spans and _c_spans(s.pool) == _c_spans(p) and s.pool.nets == p.nets


def test_seats_versus_and_pairings_blocks():
    a = _bare_net()
    odd = league.Script(0.0, 0.2)
    s = league.Seats.versus(_bare_env(n_env=10), a, ['script', a, odd])
    assert s.spans == ((0, 0, 10, 0), (1, 0, 3, 1), (1, 3, 6, 2), (1, 6, 10, 3)) and s.covered
    assert s.pool.spans == ((0, 0, 10, 0), (1, 3, 6, 0)) and [x[:4] for x in _c_seats(s)] == [(1, 1, 0, 3), (1, 1, 6, 10)]
    s = league.Seats.versus(_bare_env(n_env=10), odd, ['script'])
    assert s.pool is None and [x[:4] for x in _c_seats(s)] == [(0, 1, 0, 10), (1, 1, 0, 10)]
    assert _c_seats(s)[0][5] == 0.2 and _c_seats(s)[1][5] == 0.45
    with pytest.raises(ValueError, match='at least one rival'):
        league.Seats.versus(_bare_env(), a, [])
    with pytest.raises(ValueError, match='two-ship'):
        league.Seats.versus(_bare_env(S=1, cfg='solo'), 'script', ['script'])
    players = [a, 'nothing', odd]
    for N in (96, 7, 6):
        s = league.Seats.pairings(_bare_env(n_env=N), players)
        for j, (x, y) in enumerate(league.Pool.pairs(3)):
            lo, hi = j * N // 6, (j + 1) * N // 6
            assert hi > lo and s.spans[2 * j] == (0, lo, hi, x) and s.spans[2 * j + 1] == (1, lo, hi, y)
        assert s.covered and len(s._seats) == 8 and len(s.pool.spans) == 4
    for N, M, word in ((5, 3, 'at least 6 envs'), (100, 1, 'at least 2 players')):
        with pytest.raises(ValueError, match=word):
            league.Seats.pairings(_bare_env(n_env=N), players[:M])
    with pytest.raises(ValueError, match='two-ship'):
        league.Seats.pairings(_bare_env(S=1, cfg='solo'), ['script', 'nothing'])
    with pytest.raises(ValueError, match='a player is'):
        league.tournament(_bare_env(n_env=100), [a, 'scripted'])
    # Pool goes on rejecting what is no network
    with pytest.raises(ValueError, match='QNetwork'):
        league.Pool(_bare_env(), [a, odd], [(0, 0, 10, 0)])


def test_seats_form_value_errors():
    """What the env checks before any device call when it is handed a Seats."""
    env, a = _bare_env(), _bare_net()
    env.device = torch.device('cpu')
    full = league.Seats.versus(env, a, ['script'])
    part = league.Seats(env, [a, 'script'], [(0, 0, 10, 0), (1, 0, 9, 1)])
    bare = league.Seats.versus(env, 'script', ['nothing'])
    assert env._per_ship(full) is None and env._with_opponent(full, None) == (full, None)
    for call in (lambda: env.rollout_q(part, 1), lambda: env.play_q(part)):
        with pytest.raises(ValueError, match='uncovered'):
            call()
    for opponent in ('script', a):
        with pytest.raises(ValueError):
            env.play_q(full, opponent=opponent)
    for call in (lambda: env.qvalues(bare), lambda: env.qcontrols(bare, q_out=torch.zeros(10, 2, 6))):
        with pytest.raises(ValueError, match='no network'):
            call()
    other = _bare_env(n_env=11)
    other.device = torch.device('cpu')
    for call in (lambda: other.seat_controls(full), lambda: other.qvalues(full, out=torch.zeros(11, 2, 6)),
                 lambda: other.qcontrols(bare)):
        with pytest.raises(ValueError, match='made for 10 envs'):
            call()
    with pytest.raises(ValueError, match='league.Seats'):
        env.seat_controls(league.Pool.versus(env, a, [a]))
    for out in (torch.zeros(10, 2), torch.zeros(9, 2, dtype=torch.int8), torch.zeros(10, 4, dtype=torch.int8)[:, ::2]):
        with pytest.raises(ValueError, match='out must be'):
            env.seat_controls(full, out=out)


def test_tune_script_value_errors():
    env = _bare_env()
    ok = dict(max_trials=10, threshold=0.9, max_mutations=1, scale=0.05)
    bad = [(dict(max_trials=0), 'max_trials'), (dict(max_trials=2.0), 'max_trials'), (dict(max_trials=True), 'max_trials'),
           (dict(max_mutations=-1), 'max_mutations'), (dict(max_mutations='1'), 'max_mutations'),
           (dict(candidates=0), 'candidates'), (dict(candidates=11), 'at least 11 envs'),
           (dict(threshold=0.4), 'threshold'), (dict(threshold=1.0), 'threshold'), (dict(threshold=None), 'threshold'),
           (dict(scale='x'), 'scale'), (dict(scale=float('nan')), 'scale'),
           (dict(args=dict(avoid_distance='a')), 'finite numbers')]
    for kw, word in bad:
        with pytest.raises(ValueError, match=word):
            league.tune_script(env, **dict(ok, **kw))
    with pytest.raises(ValueError, match='at most 63 candidates'):
        league.tune_script(_bare_env(n_env=100), **dict(ok, candidates=64))
    with pytest.raises(ValueError, match='two-ship'):
        league.tune_script(_bare_env(S=1, cfg='solo'), **ok)
    # no round: the arguments come back, and nothing touches the device
    assert league.tune_script(env, **dict(ok, max_mutations=0)) == (league.Script().args, [])
    assert league.tune_script(env, args=dict(avoid_distance=0.2), **dict(ok, max_mutations=0))[0] \
        == dict(avoid_distance=0.2, avoid_threshold=0.45)


def test_qtrainer_ladder_value_errors():
    env, a, b = _bare_env(), _bare_net(), _bare_net()
    a.clone = lambda: _bare_net()
    mk = lambda **kw: train.QTrainer(env, a, _Buf(), None, **kw)   # noqa: E731
    odd = league.Script(0.3, 0.9)
    t = mk(opponent=odd)
    assert t.ladder == (odd,) and t._bot is None and t.rival is None and t.rivals is None and t.rival_every is None
    assert type(t._acting) is league.Seats and t._acting.players == (a, odd) and t._acting.covered
    t = mk(opponent=['script', b, odd])
    assert t.ladder == ('script', b, odd) and t._acting.players == (a, league.Script(), b, odd)
    assert t._acting.spans == ((0, 0, 10, 0), (1, 0, 3, 1), (1, 3, 6, 2), (1, 6, 10, 3))
    assert mk().ladder is None and mk(opponent='script').ladder is None and mk(opponent='script')._bot == 'script'
    for opponent in (odd, ['script'], ('nothing', b)):
        with pytest.raises(ValueError, match="pool_size goes with opponent='pool'"):
            mk(opponent=opponent, pool_size=2)
        with pytest.raises(ValueError, match='opponent_sync goes with'):
            mk(opponent=opponent, opponent_sync=2)
    with pytest.raises(ValueError, match='at least one rival'):
        mk(opponent=[])
    with pytest.raises(ValueError, match='a player is'):
        mk(opponent=['script', 'pool'])
    with pytest.raises(ValueError, match='a player is'):
        mk(opponent=[dict(avoid_distance=0.1)])
    with pytest.raises(ValueError, match='nout'):
        mk(opponent=[_bare_net(nout=3)])
    with pytest.raises(ValueError, match='two-ship'):
        solo = _bare_net(nships=1)
        train.QTrainer(_bare_env(S=1, cfg='solo'), solo, type('B', (), dict(n_env=10, nships=1))(), None, opponent=odd)
