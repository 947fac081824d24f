"""CPU-only checks of the network-pool library's host side
(libastro_qpool.so's argument codes), of ``league.Pool`` and its two constructors,
and of the argument rules of the pool form and of QTrainer(opponent='pool')
that run before any device call."""
import ctypes

import pytest
import torch

import __graft_entry__ as entry
import astro_amd
from astro_amd import BatchedEnv, _lib, league, qnet, train
from tests import test_libraries as libraries


def test_header_compiles_as_c_and_its_constants_are_the_bindings(tmp_path):
    """The redeclared prototype, the limits (32, 64) and AstroQSpan (16 bytes): the qpool row's prototype,
    constants and layout cases."""
    libraries.test_prototypes_agree_with_restype_and_argtypes('qpool', tmp_path)
    libraries.test_header_constants_are_the_python_ones('qpool', tmp_path)
    libraries.test_struct_layouts_are_the_ctypes_mirrors('qpool', tmp_path)
    assert [f[0] for f in _lib.AstroQSpan._fields_] == ['ship', 'net', 'lo', 'hi']


def test_argument_codes_without_gpu():
    """Every argument code of astro_qvalues_pool, in the documented order, with
    no device present (the pointers are not memory)."""
    entry.build()
    lib = _lib.load_qpool()
    V = ctypes.c_void_p

    def params(**kw):
        d = dict(nships=2, solo=0, p_pad=4, max_planets=4, b_cap=32)
        d.update(kw)
        return _lib.AstroParams(**d)

    def state(**kw):
        d = dict(ships=0x1000, ships_b=0x2000, planets=0x3000, bullets=0x4000, hdr=0x5000, n_env=100, state_f64=0)
        d.update(kw)
        return _lib.AstroState(**d)

    def net(**kw):
        d = dict(weights=0x6000, nships=2, nout=6)
        d.update(kw)
        return _lib.AstroQNet(**d)

    def nets(*ns):
        return (_lib.AstroQNet * len(ns))(*ns)

    def spans(*rows):
        return (_lib.AstroQSpan * len(rows))(*[_lib.AstroQSpan(*r) for r in rows])

    # (ship, net, lo, hi)
    good = dict(p=params(), s=state(), n=nets(net(), net()), nn=2, sp=spans((0, 0, 0, 100), (1, 1, 0, 50)), ns=2,
                q=V(0x7000), c=V(0x8000), eps=0.0, mb=0)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        if 'sp' in kw and 'ns' not in kw and a['sp'] is not None:
            a['ns'] = len(a['sp'])
        if 'n' in kw and 'nn' not in kw and a['n'] is not None:
            a['nn'] = len(a['n'])
        rc = lib.astro_qvalues_pool(None if a['p'] is None else ctypes.byref(a['p']),
                                    None if a['s'] is None else ctypes.byref(a['s']), a['n'], a['nn'], a['sp'], a['ns'],
                                    a['q'], a['c'], None, a['eps'], a['mb'], None)
        return rc, lib.astro_qpool_last_error().decode()

    nan = float('nan')
    cases = [
        (dict(p=None), -10, 'params'), (dict(s=None), -2, 'state'), (dict(n=None), -120, 'nets is NULL'),
        (dict(sp=None), -130, 'spans is NULL'),
        (dict(p=params(nships=3)), -11, 'nships'), (dict(p=params(nships=0)), -11, 'nships'),
        (dict(p=params(p_pad=0)), -13, 'p_pad'), (dict(p=params(p_pad=17)), -13, 'p_pad'),
        (dict(p=params(b_cap=0)), -15, 'b_cap'), (dict(p=params(b_cap=65536)), -15, 'b_cap'),
        (dict(nn=0), -131, 'nnets'), (dict(nn=33), -131, 'nnets'), (dict(nn=-1), -131, 'nnets'),
        (dict(ns=0), -132, 'nspans'), (dict(ns=65), -132, 'nspans'), (dict(ns=-2), -132, 'nspans'),
        (dict(s=state(n_env=-1)), -3, 'n_env'),
        (dict(sp=spans((2, 0, 0, 1))), -133, 'spans[0].ship'), (dict(sp=spans((0, 0, 0, 1), (-1, 0, 0, 1))), -133, 'spans[1]'),
        (dict(p=params(nships=1), n=nets(net(nships=1)), sp=spans((1, 0, 0, 1))), -133, 'ship'),
        (dict(sp=spans((0, 2, 0, 1))), -134, 'spans[0].net'), (dict(sp=spans((0, 0, 0, 1), (1, -2, 0, 1))), -134, 'spans[1]'),
        (dict(sp=spans((0, 0, -1, 1))), -135, 'lo <= hi'), (dict(sp=spans((0, 0, 5, 4))), -135, 'lo <= hi'),
        (dict(sp=spans((0, 0, 0, 101))), -135, 'n_env'), (dict(sp=spans((0, -1, 0, 101))), -135, 'spans[0]'),
        (dict(sp=spans((0, 0, 0, 10), (0, 1, 9, 20))), -136, 'overlap'),
        (dict(sp=spans((1, 0, 0, 10), (0, 0, 0, 10), (1, -1, 5, 6))), -136, 'spans[0] and spans[2]'),
        (dict(sp=spans((0, 0, 10, 20), (0, 1, 0, 11))), -136, 'overlap'),
        (dict(n=nets(net(nships=1), net())), -101, 'nets[0].nships'), (dict(n=nets(net(), net(nships=1))), -101, 'nets[1]'),
        (dict(n=nets(net(nout=0), net())), -102, 'nets[0].nout'), (dict(n=nets(net(), net(nout=7))), -102, 'nets[1]'),
        (dict(n=nets(net(nout=6), net(nout=3))), -122, 'differ'),
        (dict(q=None, c=None), -103, 'both NULL'),
        (dict(eps=-0.5), -104, 'epsilon'), (dict(eps=1.0001), -104, 'epsilon'), (dict(eps=nan), -104, 'epsilon'),
        (dict(mb=-1), -123, 'max_blocks'),
        (dict(n=nets(net(weights=None), net())), -105, 'nets[0]'), (dict(n=nets(net(), net(weights=0x6002))), -105, 'nets[1]'),
        (dict(s=state(ships=None)), -4, 'NULL'), (dict(s=state(hdr=None)), -4, 'NULL'),
        (dict(s=state(bullets=0x4008)), -5, 'aligned'), (dict(s=state(ships=0x1004)), -5, 'aligned'),
        (dict(s=state(state_f64=2)), -6, 'state_f64'),
        (dict(q=V(0x7002)), -106, 'q must be'),
    ]
    codes = set()
    for kw, code, word in cases:
        rc, msg = call(**kw)
        assert rc == code and word in msg, (kw, rc, msg)
        codes.add(rc)
    assert sorted(codes) == [-136, -135, -134, -133, -132, -131, -130, -123, -122, -120, -106, -105, -104, -103, -102,
                             -101, -15, -13, -11, -10, -6, -5, -4, -3, -2]
    # what does not overlap: touching spans, empty spans anywhere, the same envs of the other ship
    bad_q = dict(q=V(0x7002))                                       # the last code: everything before it passed
    assert call(sp=spans((0, 0, 0, 50), (0, 1, 50, 100), (1, 1, 0, 100)), **bad_q)[0] == -106
    assert call(sp=spans((0, 0, 0, 100), (0, 1, 30, 30), (0, -1, 100, 100), (0, 1, 0, 0)), **bad_q)[0] == -106
    # nothing to do returns 0 whatever the pointers are -- but only after the scalar checks: no envs,
    empty = state(n_env=0, ships=None, hdr=None)
    none_left = dict(s=empty, sp=spans((0, 0, 0, 0), (1, 1, 0, 0)), n=nets(net(weights=None), net(weights=None)))
    assert call(**none_left)[0] == 0
    assert call(mb=-1, **none_left)[0] == -123 and call(eps=nan, **none_left)[0] == -104
    assert call(s=empty)[0] == -135                                 # the good spans do not fit zero envs
    # every span empty or skipped
    idle = dict(s=state(ships=None, state_f64=2), n=nets(net(weights=None), net(weights=0x6002)), q=V(0x7002))
    assert call(sp=spans((0, 0, 7, 7), (1, -1, 0, 100), (0, -1, 50, 60), (1, 1, 100, 100)), **idle)[0] == 0
    assert call(sp=spans((0, -1, 0, 100)), **idle)[0] == 0
    # a network that no span names is not looked at; one that only an empty span names is
    assert call(sp=spans((0, 0, 0, 100)), n=nets(net(), net(nships=1, nout=9, weights=None)), **bad_q)[0] == -106
    assert call(sp=spans((0, 0, 0, 100), (1, 1, 3, 3)), n=nets(net(), net(nships=1)))[0] == -101
    assert call(sp=spans((0, 1, 0, 100), (1, 1, 0, 100)), n=nets(net(nout=3), net(nout=5)), **bad_q)[0] == -106
    # a solo env
    solo = params(nships=1)
    assert call(p=solo, n=nets(net(nships=1), net(nships=1)), sp=spans((0, 0, 0, 40), (0, 1, 40, 100)), **bad_q)[0] == -106
    # 32 networks and 64 spans are accepted
    many = spans(*[(k % 2, k // 2, (k // 2) * 3, (k // 2) * 3 + 3) for k in range(64)])
    assert call(n=nets(*[net() for _ in range(32)]), sp=many, **bad_q)[0] == -106
    # the order: each call breaks the rule of its code and of every later one
    worst = dict(s=state(n_env=-1, ships=None, state_f64=2), q=None, c=None, eps=nan, mb=-1, nn=0, ns=0,
                 sp=spans((5, 9, 3, 2), (5, 9, 3, 2)), n=nets(net(nships=1, nout=0, weights=None), net(nout=3)))
    assert call(p=params(nships=3, p_pad=0, b_cap=0), **worst)[0] == -11
    assert call(p=params(p_pad=0, b_cap=0), **worst)[0] == -13
    assert call(p=params(b_cap=0), **worst)[0] == -15
    assert call(**worst)[0] == -131
    worst.update(nn=2)
    assert call(**worst)[0] == -132
    worst.update(ns=2)
    assert call(**worst)[0] == -3
    worst.update(s=state(n_env=10, ships=None, state_f64=2))
    assert call(**worst)[0] == -133
    worst.update(sp=spans((0, 9, 3, 2), (0, 9, 3, 2)))
    assert call(**worst)[0] == -134
    worst.update(sp=spans((0, 0, 3, 2), (0, 1, 3, 2)))
    assert call(**worst)[0] == -135
    worst.update(sp=spans((0, 0, 2, 5), (0, 1, 4, 6)))
    assert call(**worst)[0] == -136
    worst.update(sp=spans((0, 0, 2, 5), (1, 1, 4, 6)))
    assert call(**worst)[0] == -101
    worst.update(n=nets(net(nout=0, weights=None), net(nout=3)))
    assert call(**worst)[0] == -102
    worst.update(n=nets(net(nout=2, weights=None), net(nout=3)))
    assert call(**worst)[0] == -122
    worst.update(n=nets(net(weights=None), net()))
    assert call(**worst)[0] == -103
    worst.update(q=V(0x7002))
    assert call(**worst)[0] == -104
    worst.update(eps=0.5)
    assert call(**worst)[0] == -123
    worst.update(mb=3)
    assert call(**worst)[0] == -105
    worst.update(n=nets(net(), net()))
    assert call(**worst)[0] == -4
    worst.update(s=state(n_env=10, planets=0x3004, state_f64=2))
    assert call(**worst)[0] == -5
    worst.update(s=state(n_env=10, state_f64=2))
    assert call(**worst)[0] == -6
    worst.update(s=state(n_env=10))
    assert call(**worst)[0] == -106


# ---------------------------------------------------------------------------
# league.Pool

def _bare_env(S=2, n_env=10):
    """A BatchedEnv that was never initialised: the argument checks read S, n_env and hdr.device only."""
    env = BatchedEnv.__new__(BatchedEnv)
    env.S, env.n_env, env.hdr = S, n_env, torch.zeros(1)
    return env


def _bare_net(nships=2, nout=6, weights=None):
    """A QNetwork without device storage, for the checks that read its shape, its device and its struct."""
    n = qnet.QNetwork.__new__(qnet.QNetwork)
    n.nships, n.nout, n.weights = nships, nout, torch.zeros(1) if weights is None else weights
    n.c = _lib.AstroQNet(weights=0x6000, nships=nships, nout=nout)
    return n


def _c_spans(pool):
    return [(s.ship, s.net, s.lo, s.hi) for s in pool._spans]


def test_pool_is_checked_and_immutable():
    env = _bare_env()
    a, b, c = _bare_net(), _bare_net(), _bare_net()
    pool = league.Pool(env, [a, b, c], [(0, 0, 10, 0), (1, 0, 1, 1), (1, 1, 4, 0), (1, 4, 4, 2), (1, 4, 8, None),
                                       (1, 8, 10, 2)])
    assert pool.nets == (a, b, c) and pool.spans[4] == (1, 4, 8, None) and len(pool.spans) == 6
    assert (pool.n_env, pool.S, pool.nout, pool.device) == (10, 2, 6, torch.device('cpu'))
    assert not pool.covered
    assert _c_spans(pool) == [(0, 0, 0, 10), (1, 1, 0, 1), (1, 0, 1, 4), (1, 2, 4, 4), (1, -1, 4, 8), (1, 2, 8, 10)]
    assert [(n.weights, n.nships, n.nout) for n in pool._nets] == [(0x6000, 2, 6)] * 3
    assert astro_amd.Pool is league.Pool and astro_amd.tournament is league.tournament
    for name in ('spans', 'nets', 'covered', 'other'):
        with pytest.raises(AttributeError):
            setattr(pool, name, ())
    # covered: every ship of every env, whatever the order of the spans and with empty ones between
    assert league.Pool(env, [a, b], [(1, 5, 10, 1), (0, 0, 10, 0), (1, 5, 5, None), (1, 0, 5, 0)]).covered
    assert not league.Pool(env, [a], [(0, 0, 10, 0)]).covered                      # ship 1 has nobody
    assert not league.Pool(env, [a], [(0, 0, 10, 0), (1, 0, 9, 0)]).covered
    assert not league.Pool(env, [a], [(0, 0, 10, 0), (1, 1, 10, 0)]).covered
    assert not league.Pool(env, [a], [(0, 0, 10, 0), (1, 0, 4, 0), (1, 5, 10, 0)]).covered
    assert league.Pool(_bare_env(S=1), [_bare_net(nships=1)], [(0, 0, 10, 0)]).covered
    many = [(k % 2, (k // 2) * 3, (k // 2) * 3 + 3, k // 2) for k in range(64)]
    assert len(league.Pool(_bare_env(n_env=96), [_bare_net() for _ in range(32)], many).spans) == 64
    bad = [
        (([], [(0, 0, 10, 0)]), 'networks'), (([a] * 33, [(0, 0, 10, 0)]), 'networks'),
        (([a, 'script'], [(0, 0, 10, 0)]), 'QNetwork'), (([a, None], [(0, 0, 10, 0)]), 'QNetwork'),
        (([a, _bare_net(weights=torch.zeros(1, device='meta'))], [(0, 0, 10, 0)]), 'env on'),
        (([a, _bare_net(nships=1)], [(0, 0, 10, 0)]), 'ships'), (([a, _bare_net(nout=3)], [(0, 0, 10, 0)]), 'nout'),
        (([a], []), 'spans'), (([a], [(0, 0, 0, 0)] * 65), 'spans'),
        (([a], [(0, 0, 10)]), 'span is'), (([a], [(0, 0, 10, 'a')]), 'span is'), (([a], [(0, 0.5, 10, 0)]), 'span is'),
        (([a], [(0, 0, 10, True)]), 'span is'), (([a], [7]), 'span is'),
        (([a], [(2, 0, 10, 0)]), 'ship'), (([a], [(-1, 0, 10, 0)]), 'ship'),
        (([a], [(0, 0, 10, 1)]), 'network'), (([a], [(0, 0, 10, -1)]), 'network'),
        (([a], [(0, -1, 10, 0)]), 'lo <= hi'), (([a], [(0, 6, 5, 0)]), 'lo <= hi'), (([a], [(0, 0, 11, 0)]), 'lo <= hi'),
        (([a], [(0, 0, 6, 0), (0, 5, 10, 0)]), 'overlap'), (([a], [(1, 0, 10, 0), (1, 3, 4, None)]), 'overlap'),
    ]
    for (nets_, spans_), word in bad:
        with pytest.raises(ValueError, match=word):
            league.Pool(env, nets_, spans_)
    with pytest.raises(ValueError, match='ship'):
        league.Pool(_bare_env(S=1), [_bare_net(nships=1)], [(1, 0, 10, 0)])


def test_pool_versus_blocks():
    a = _bare_net()
    for N, K in ((10, 1), (10, 3), (64, 2), (7, 4), (100, 8), (3, 5), (65536, 31)):
        env, rivals = _bare_env(n_env=N), [_bare_net() for _ in range(K)]
        pool = league.Pool.versus(env, a, rivals)
        assert pool.nets == (a,) + tuple(rivals) and pool.covered
        assert pool.spans[0] == (0, 0, N, 0)
        blocks = pool.spans[1:]
        assert [sp[0] for sp in blocks] == [1] * K and [sp[3] for sp in blocks] == list(range(1, K + 1))
        assert blocks[0][1] == 0 and blocks[-1][2] == N
        assert all(x[2] == y[1] for x, y in zip(blocks, blocks[1:]))                # consecutive
        sizes = [hi - lo for _, lo, hi, _ in blocks]
        assert max(sizes) - min(sizes) <= 1 and sum(sizes) == N
        assert [(lo, hi) for _, lo, hi, _ in blocks] == [(j * N // K, (j + 1) * N // K) for j in range(K)]
    assert league.Pool.versus(_bare_env(n_env=10), a, [a, a, a]).spans[1:] == ((1, 0, 3, 1), (1, 3, 6, 2), (1, 6, 10, 3))
    for rivals in ([], [a] * 32):
        with pytest.raises(ValueError, match='rivals'):
            league.Pool.versus(_bare_env(), a, rivals)
    with pytest.raises(ValueError, match='two-ship'):
        league.Pool.versus(_bare_env(S=1), _bare_net(nships=1), [_bare_net(nships=1)])
    with pytest.raises(ValueError, match='nout'):
        league.Pool.versus(_bare_env(), a, [_bare_net(nout=3)])


def test_pool_pairings_blocks():
    nets = [_bare_net() for _ in range(6)]
    assert league.Pool.pairs(3) == [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)]
    for N, M in ((96, 3), (100, 3), (7, 3), (6, 3), (2, 2), (50, 4), (31, 6), (30, 6)):
        pool = league.Pool.pairings(_bare_env(n_env=N), nets[:M])
        pairs = league.Pool.pairs(M)
        P = M * (M - 1)
        assert len(pairs) == P and len(pool.spans) == 2 * P and pool.covered and pool.nets == tuple(nets[:M])
        for j, (a, b) in enumerate(pairs):
            lo, hi = j * N // P, (j + 1) * N // P
            assert hi > lo
            assert pool.spans[2 * j] == (0, lo, hi, a) and pool.spans[2 * j + 1] == (1, lo, hi, b)
    assert [sp[1:3] for sp in league.Pool.pairings(_bare_env(n_env=7), nets[:3]).spans[::2]] \
        == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 7)]
    for N, M, word in ((5, 3, 'at least 6 envs'), (1, 2, 'at least 2 envs'), (100, 1, 'networks'), (100, 0, 'networks')):
        with pytest.raises(ValueError, match=word):
            league.Pool.pairings(_bare_env(n_env=N), nets[:M])
    with pytest.raises(ValueError, match='networks'):
        league.Pool.pairings(_bare_env(n_env=100), nets + [_bare_net()])
    with pytest.raises(ValueError, match='two-ship'):
        league.Pool.pairings(_bare_env(S=1), [_bare_net(nships=1)] * 2)
    with pytest.raises(ValueError):
        league.tournament(_bare_env(n_env=5), nets[:3])


def test_pool_form_value_errors():
    """What the env checks before any device call when it is handed a Pool."""
    env, a, b = _bare_env(), _bare_net(), _bare_net()
    full = league.Pool.versus(env, a, [b])
    part = league.Pool(env, [a, b], [(0, 0, 10, 0), (1, 0, 9, 1)])
    assert env._per_ship(full) is None and env._with_opponent(full, None) == (full, None)
    for call in (lambda: env.rollout_q(part, 1), lambda: env.play_q(part)):
        with pytest.raises(ValueError, match='uncovered'):
            call()
    for opponent in ('script', b):
        with pytest.raises(ValueError, match='Pool'):
            env._with_opponent(full, opponent)
        with pytest.raises(ValueError):
            env.play_q(full, opponent=opponent)
    # a pool made for another shape
    other = _bare_env(n_env=11)
    other.device = torch.device('cpu')
    for call in (lambda: other.qvalues(full, out=torch.zeros(11, 2, 6)), lambda: other._qvalues_pool(full, None, None, None, 0.0)):
        with pytest.raises(ValueError, match='made for 10 envs'):
            call()


class _Buf:
    n_env, nships = 10, 2


def test_qtrainer_pool_value_errors():
    env, a, b = _bare_env(), _bare_net(), _bare_net()
    a.clone = lambda: _bare_net()
    mk = lambda **kw: train.QTrainer(env, a, _Buf(), None, **kw)   # noqa: E731
    for kw in (dict(pool_size=2), dict(opponent='snapshot', opponent_sync=2, pool_size=2),
               dict(opponent='script', pool_size=1), dict(opponent=b, pool_size=3)):
        with pytest.raises(ValueError, match="pool_size goes with opponent='pool'"):
            mk(**kw)
    for kw in (dict(opponent='pool', pool_size=2), dict(opponent='pool', pool_size=2, opponent_sync=0),
               dict(opponent='pool', pool_size=2, opponent_sync=2.0), dict(opponent='pool', pool_size=2, opponent_sync=True)):
        with pytest.raises(ValueError, match='opponent_sync'):
            mk(**kw)
    for size in (None, 0, -1, 32, 2.0, True, '2'):
        with pytest.raises(ValueError, match='pool_size'):
            mk(opponent='pool', pool_size=size, opponent_sync=1)
    with pytest.raises(ValueError, match='two-ship'):
        solo = _bare_net(nships=1)
        solo.clone = lambda: _bare_net(nships=1)
        train.QTrainer(_bare_env(S=1), solo, type('B', (), dict(n_env=10, nships=1))(), None, opponent='pool',
                       pool_size=2, opponent_sync=1)
    with pytest.raises(ValueError, match='opponent'):
        env._check_opponent('pool')                                  # a trainer's word, not an env's
    t = mk(opponent='pool', pool_size=3, opponent_sync=5)
    assert len(t.rivals) == 3 and t.rival is None and t.rival_every == 5 and t._bot is None
    assert type(t._acting) is league.Pool and t._acting.nets == (a,) + tuple(t.rivals) and t._acting.covered
    assert t._acting.spans == ((0, 0, 10, 0), (1, 0, 3, 1), (1, 3, 6, 2), (1, 6, 10, 3))
    assert mk().rivals is None and mk(opponent='snapshot', opponent_sync=1).rivals is None
    names = train.QTrainer.__init__.__code__.co_varnames
    assert names[12:15] == ('opponent', 'opponent_sync', 'pool_size')
