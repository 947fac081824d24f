"""CPU-only checks of the per-ship Q-network library's host side
(libastro_qduel.so's argument codes), of astro_amd/league.py's statistics, and of the
argument checks of the per-ship form and of QTrainer(opponent=...) that run
before any device call."""
import ctypes
import fractions
import math

import pytest
import torch

import __graft_entry__ as entry
import astro_amd
from astro_amd import BatchedEnv, _lib, league, qnet, train


def test_argument_codes_without_gpu():
    """Every argument code of astro_qvalues_ships, in the documented order,
    with no device present (the pointers are not memory)."""
    entry.build()
    lib = _lib.load_qduel()
    V = ctypes.c_void_p
    Nets = ctypes.POINTER(_lib.AstroQNet) * 2

    def params(**kw):
        d = dict(nships=2, solo=0, p_pad=4, max_planets=4, b_cap=32)
        d.update(kw)
        return _lib.AstroParams(**d)

    def state(**kw):
        d = dict(ships=0x1000, ships_b=0x2000, planets=0x3000, bullets=0x4000, hdr=0x5000, n_env=1, state_f64=0)
        d.update(kw)
        return _lib.AstroState(**d)

    def net(**kw):
        d = dict(weights=0x6000, nships=2, nout=6)
        d.update(kw)
        return _lib.AstroQNet(**d)

    keep = []

    def nets(a, b):
        arr = Nets()
        for k, n in enumerate((a, b)):
            if n is not None:
                keep.append(n)
                arr[k] = ctypes.pointer(n)
        return arr

    good = dict(p=params(), s=state(), n=nets(net(), net()), q=V(0x7000), c=V(0x8000), eps=0.0, mb=0)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        rc = lib.astro_qvalues_ships(None if a['p'] is None else ctypes.byref(a['p']),
                                     None if a['s'] is None else ctypes.byref(a['s']), a['n'], a['q'], a['c'], None,
                                     a['eps'], a['mb'], None)
        return rc, lib.astro_qduel_last_error().decode()

    nan = float('nan')
    cases = [
        (dict(p=None), -10, 'params'), (dict(s=None), -2, 'state'), (dict(n=None), -120, 'nets is NULL'),
        (dict(p=params(nships=3)), -11, 'nships'), (dict(p=params(nships=0)), -11, 'nships'),
        (dict(p=params(p_pad=0)), -13, 'p_pad'), (dict(p=params(p_pad=17)), -13, 'p_pad'),
        (dict(p=params(b_cap=0)), -15, 'b_cap'), (dict(p=params(b_cap=65536)), -15, 'b_cap'),
        (dict(n=nets(None, None)), -121, 'every net is NULL'),
        (dict(p=params(nships=1), n=nets(None, net(nships=1))), -121, 'every net is NULL'),
        (dict(n=nets(net(nships=1), None)), -101, 'nships'), (dict(n=nets(net(), net(nships=1))), -101, 'nets[1]'),
        (dict(n=nets(net(nout=0), None)), -102, 'nout'), (dict(n=nets(None, net(nout=7))), -102, 'nets[1]'),
        (dict(n=nets(net(nout=6), net(nout=3))), -122, 'differ'),
        (dict(q=None, c=None), -103, 'both NULL'),
        (dict(eps=-0.5), -104, 'epsilon'), (dict(eps=1.0001), -104, 'epsilon'), (dict(eps=nan), -104, 'epsilon'),
        (dict(mb=-1), -123, 'max_blocks'),
        (dict(s=state(n_env=-1)), -3, 'n_env'),
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
    assert sorted(codes) == [-123, -122, -121, -120, -106, -105, -104, -103, -102, -101, -15, -13, -11, -10, -6, -5,
                             -4, -3, -2]
    # no envs: nothing to do, whatever the pointers are -- but only after the scalar checks
    empty = state(n_env=0, ships=None, hdr=None)
    assert call(s=empty, n=nets(net(weights=None), None))[0] == 0
    assert call(s=empty, mb=-1)[0] == -123 and call(s=empty, eps=nan)[0] == -104
    # the order: each call breaks the rule of its code and of every later one
    worst = dict(s=state(n_env=-1, ships=None, state_f64=2), q=None, c=None, eps=nan, mb=-1)
    assert call(p=params(nships=3, p_pad=0, b_cap=0), n=nets(None, None), **worst)[0] == -11
    assert call(p=params(p_pad=0, b_cap=0), n=nets(None, None), **worst)[0] == -13
    assert call(p=params(b_cap=0), n=nets(None, None), **worst)[0] == -15
    assert call(n=nets(None, None), **worst)[0] == -121
    assert call(n=nets(net(nships=1, nout=0), net(nout=3, weights=None)), **worst)[0] == -101
    assert call(n=nets(net(nout=0), net(nout=3, weights=None)), **worst)[0] == -102
    assert call(n=nets(net(nout=2), net(nout=3, weights=None)), **worst)[0] == -122
    assert call(n=nets(net(), net(weights=None)), **worst)[0] == -103
    worst.update(q=V(0x7002))
    assert call(n=nets(net(), net(weights=None)), **worst)[0] == -104
    worst.update(eps=0.5)
    assert call(n=nets(net(), net(weights=None)), **worst)[0] == -123
    worst.update(mb=3)
    assert call(n=nets(net(), net(weights=None)), **worst)[0] == -3
    assert call(n=nets(net(), net(weights=None)), s=state(ships=None, state_f64=2), q=V(0x7002))[0] == -105
    assert call(s=state(ships=None, planets=0x3004, state_f64=2), q=V(0x7002))[0] == -4
    assert call(s=state(planets=0x3004, state_f64=2), q=V(0x7002))[0] == -5
    assert call(s=state(state_f64=2), q=V(0x7002))[0] == -6
    # a solo env reads nets[0] only: a second entry is neither needed nor looked at
    solo = params(nships=1)
    assert call(p=solo, n=nets(net(nships=1), net(nships=2, nout=9)), q=V(0x7002))[0] == -106
    # a skipped ship's net is not looked at either: one network is enough
    assert call(n=nets(None, net()), q=V(0x7002))[0] == -106 and call(n=nets(net(), None), q=V(0x7002))[0] == -106


# ---------------------------------------------------------------------------
# league.py

def test_p_better_values_and_symmetry():
    assert league.p_better(0, 0) == 0.5 and league.p_better(1, 0) == 0.75 and league.p_better(3, 1) == 0.8125
    assert league.p_better(0, 1) == 0.25 and league.p_better(0, 3) == 0.0625 and league.p_better(2, 0) == 0.875
    for w in range(0, 40):
        for l in range(0, 40):
            p = league.p_better(w, l)
            assert p + league.p_better(l, w) == 1 and 0 < p < 1
            # the exact rational: P(Binomial(w + l + 1, 1/2) <= w)
            n = w + l + 1
            exact = fractions.Fraction(sum(math.comb(n, k) for k in range(w + 1)), 2 ** n)
            assert abs(fractions.Fraction(p) - exact) <= fractions.Fraction(1, 2 ** 53)
            if w > l:
                assert p > 0.5 and p > league.p_better(w - 1, l)
    for w, l in ((3000, 2800), (2800, 3000), (5000, 0), (0, 5000), (4096, 4096)):      # large counts neither overflow
        p = league.p_better(w, l)                                                      # nor lose the symmetry
        assert 0 <= p <= 1 and p + league.p_better(l, w) == 1
    assert league.p_better(3000, 2800) > 0.99 and league.p_better(4096, 4096) == 0.5 and league.p_better(5000, 0) == 1.0
    for bad in ((-1, 0), (0, -1), (1.5, 0)):
        with pytest.raises(ValueError):
            league.p_better(*bad)
    assert astro_amd.p_better is league.p_better and astro_amd.find_better is league.find_better
    assert astro_amd.compare is league.compare and astro_amd.league is league


def test_p_better_equals_the_beta_posterior():
    stats = pytest.importorskip('scipy.stats')
    for w in range(31):
        for l in range(31):
            assert abs(league.p_better(w, l) - (1 - stats.beta.cdf(0.5, 1 + w, 1 + l))) <= 1e-12, (w, l)


def _counted(seq):
    taken = []

    def gen():
        for x in seq:
            taken.append(x)
            yield x
    return gen(), taken


def test_find_better():
    # a sure winner returns early: p_better(4, 0) = 31/32 < 0.98 < 63/64 = p_better(5, 0), so after five games
    assert league.p_better(4, 0) == 31 / 32 and league.p_better(5, 0) == 63 / 64
    g, taken = _counted([0] * 100)
    assert league.find_better(g, 100, 0.98) == 0 and len(taken) == 5
    g, taken = _counted([1] * 100)
    assert league.find_better(g, 100, 0.98) == 1 and len(taken) == 5
    g, taken = _counted([None, 1, None, 1, 1, 0, 1, 1, 1, 1, 1] + [1] * 50)
    assert league.find_better(g, 100, 0.9) == 1 and len(taken) < 20
    # alternating winners: neither side can reach the threshold within max_trials, and that is seen
    # before the sequence (or even max_trials) is exhausted
    g, taken = _counted([0, 1] * 50)
    assert league.find_better(g, 20, 0.999) is None
    assert 0 < len(taken) < 20
    n = len(taken)
    w0, w1 = taken.count(0), taken.count(1)
    left = 20 - n
    assert league.p_better(w0 + left, w1) < 0.999 and 1 - league.p_better(w0, w1 + left) < 0.999
    # ... and one game earlier it was still open
    w0e, w1e = taken[:-1].count(0), taken[:-1].count(1)
    assert not (league.p_better(w0e + left + 1, w1e) < 0.999 and 1 - league.p_better(w0e, w1e + left + 1) < 0.999)
    # games without a winner count as trials only
    g, taken = _counted([None] * 100)
    assert league.find_better(g, 10, 0.9) is None and len(taken) < 10
    # a sequence that ends undecided
    assert league.find_better(iter([0, 1, 0]), 1000, 0.99) is None
    assert league.find_better(iter([]), 10, 0.9) is None


# ---------------------------------------------------------------------------
# argument checks that run before any device call

def _bare_env(S=2, n_env=4):
    """A BatchedEnv that was never initialised: the argument checks read S, n_env and hdr.device only."""
    env = BatchedEnv.__new__(BatchedEnv)
    env.S, env.n_env, env.hdr = S, n_env, torch.zeros(1)
    return env


def _bare_net(nships=2, nout=6, weights=None):
    """A QNetwork without device storage, for the checks that read its shape and its device."""
    n = qnet.QNetwork.__new__(qnet.QNetwork)
    n.nships, n.nout, n.weights = nships, nout, torch.zeros(1) if weights is None else weights
    return n


def test_per_ship_form_value_errors():
    env = _bare_env()
    a, b = _bare_net(), _bare_net()
    assert env._per_ship(a) is None                                    # one network: today's path
    assert env._per_ship((a, b)) == (a, b) and env._per_ship([a, None]) == (a, None)
    assert env._per_ship((None, b)) == (None, b)
    for bad, word in (((a,), 'entries'), ((a, b, a), 'entries'), ((), 'entries'), ((None, None), 'at least one'),
                      ((a, 'script'), 'QNetwork or None'), ((a, _bare_net(nships=1)), 'ships'),
                      ((_bare_net(nships=1), None), 'ships'), ((a, _bare_net(nout=3)), 'nout'),
                      ((a, _bare_net(weights=torch.zeros(1, device='meta'))), 'env on')):
        with pytest.raises(ValueError, match=word):
            env._per_ship(bad)
        for call in (lambda: env.qvalues(bad), lambda: env.qcontrols(bad), lambda: env.rollout_q(bad, 1),
                     lambda: env.play_q(bad)):
            with pytest.raises(ValueError):
                call()
    solo = _bare_env(S=1)
    assert solo._per_ship((_bare_net(nships=1),)) is not None
    with pytest.raises(ValueError, match='entries'):
        solo._per_ship((_bare_net(nships=1), None))
    # opponent: a name or a QNetwork, two ships, and not together with the per-ship form
    env._check_opponent(None), env._check_opponent('script'), env._check_opponent(b)
    for bad in ('snapshot', 'bot', 3, (a, b)):
        with pytest.raises(ValueError, match='opponent'):
            env._check_opponent(bad)
    with pytest.raises(ValueError, match='opponent'):
        solo._check_opponent('script')
    with pytest.raises(ValueError, match='opponent'):
        solo._check_opponent(_bare_net(nships=1))
    assert env._with_opponent(a, None) == (a, None) and env._with_opponent(a, 'random') == ((a, None), 'random')
    assert env._with_opponent(a, b) == ((a, b), None)
    with pytest.raises(ValueError, match='per-ship'):
        env._with_opponent((a, b), 'script')
    for call in (lambda: env.rollout_q((a, None), 1), lambda: env.play_q((None, b)),
                 lambda: env.rollout_q(a, 1, opponent=_bare_net(nout=3)), lambda: env.play_q(a, opponent='bot')):
        with pytest.raises(ValueError):
            call()


class _Buf:
    n_env, nships = 4, 2


def test_qtrainer_opponent_value_errors():
    env, a, b = _bare_env(), _bare_net(), _bare_net()
    mk = lambda **kw: train.QTrainer(env, a, _Buf(), None, **kw)   # noqa: E731
    for kw in (dict(opponent='snapshot'), dict(opponent='snapshot', opponent_sync=0),
               dict(opponent='snapshot', opponent_sync=-3), dict(opponent='snapshot', opponent_sync=2.0),
               dict(opponent='snapshot', opponent_sync=True), dict(opponent='snapshot', opponent_sync='2')):
        with pytest.raises(ValueError, match='opponent_sync'):
            mk(**kw)
    for kw in (dict(opponent_sync=2), dict(opponent='script', opponent_sync=2), dict(opponent=b, opponent_sync=1)):
        with pytest.raises(ValueError, match='snapshot'):
            mk(**kw)
    for kw in (dict(opponent='bot'), dict(opponent=7), dict(opponent=_bare_net(nout=3)),
               dict(opponent=_bare_net(nships=1))):
        with pytest.raises(ValueError):
            mk(**kw)
    with pytest.raises(ValueError, match='two-ship'):
        train.QTrainer(_bare_env(S=1), _bare_net(nships=1), type('B', (), dict(n_env=4, nships=1))(), None,
                       opponent='snapshot', opponent_sync=1)
    # what is accepted, and what tick() will act with
    t = mk(opponent=b)
    assert t.rival is b and t._acting == (a, b) and t._bot is None and t.rival_every is None
    t = mk(opponent='script')
    assert t.rival is None and t._acting == (a, None) and t._bot == 'script'
    t = mk()
    assert t.rival is None and t._acting is a and t._bot is None
    names = train.QTrainer.__init__.__code__.co_varnames
    assert names[12:14] == ('opponent', 'opponent_sync')
