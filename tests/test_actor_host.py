"""CPU-only checks of the actor library's host side: astro_amd/actor.py's numpy
models against the reference's own EpsilonGreedy (counts in
tests/golden/explore.npz, tools/gen_golden.py: gen_explore) and a hand-written
schedule of game ends, and libastro_actor.so's argument checks."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest

import __graft_entry__
from astro_amd import _lib, actor
from tests import actor_util as au
from tests import golden_io as gio
from tests import test_libraries as libraries


def test_header_compiles_as_c_and_matches_the_ctypes_layout(tmp_path):
    """Both structs, the ABI number and ASTRO_EXPLORE_ONE == 2^53: the actor row's layout and constants cases."""
    libraries.test_struct_layouts_are_the_ctypes_mirrors('actor', tmp_path)
    libraries.test_header_constants_are_the_python_ones('actor', tmp_path)


def _explore(**kw):
    a = dict(policy=0x10000, stay_out=1 << 52, stay_in=1 << 51, seed=3, env_offset=0, nrandom=5, reserved=0)
    a.update(kw)
    return _lib.AstroExplore(**a)


def _episodes(**kw):
    a = dict(length=0x10000, got=0x20000, winner=0x30000, ticks=0x40000, wins=0x50000, finished=0x60000,
             tick_sum=0x70000, n_env=40, nships=2, games=2, reserved=0)
    a.update(kw)
    return _lib.AstroEpisodes(**a)


def test_bad_arguments_without_gpu():
    """Every bad argument has its own negative code and a message, and is
    rejected before the device is touched (the pointers are not memory)."""
    __graft_entry__.build()
    lib = _lib.load_actor()
    P = ctypes.c_void_p

    def explore(p=None, s=None, ex=None, control=P(0x1000), null=()):
        p = _lib.AstroParams(nships=2) if p is None else p
        s = _lib.AstroState(hdr=0x90000, n_env=40) if s is None else s
        ex = _explore() if ex is None else ex
        rc = lib.astro_explore(None if 'p' in null else ctypes.byref(p), None if 's' in null else ctypes.byref(s),
                               None if 'ex' in null else ctypes.byref(ex), 7, control, None)
        return rc, lib.astro_actor_last_error().decode()

    def episodes(ep=None, reward=P(0x1000), done=P(0x2000), null=False):
        ep = _episodes() if ep is None else ep
        rc = lib.astro_episodes(None if null else ctypes.byref(ep), reward, done, None)
        return rc, lib.astro_actor_last_error().decode()

    cases = [
        (explore, dict(null=('p',)), -100, 'NULL'), (explore, dict(null=('s',)), -100, 'NULL'),
        (explore, dict(null=('ex',)), -100, 'NULL'), (episodes, dict(null=True), -100, 'ep is NULL'),
        (explore, dict(p=_lib.AstroParams(nships=0)), -101, 'nships'),
        (explore, dict(p=_lib.AstroParams(nships=3)), -101, 'nships'),
        (episodes, dict(ep=_episodes(nships=3)), -101, 'nships'),
        (explore, dict(s=_lib.AstroState(hdr=0x90000, n_env=0)), -102, 'n_env'),
        (episodes, dict(ep=_episodes(n_env=0)), -102, 'n_env'),
        (explore, dict(ex=_explore(nrandom=0)), -103, 'nrandom'), (explore, dict(ex=_explore(nrandom=7)), -103, 'nrandom'),
        (explore, dict(ex=_explore(stay_out=(1 << 53) + 1)), -104, '2^53'),
        (explore, dict(ex=_explore(stay_in=(1 << 53) + 1)), -104, '2^53'),
        (episodes, dict(ep=_episodes(games=0)), -105, 'games'), (episodes, dict(ep=_episodes(games=-1)), -105, 'games'),
        (explore, dict(s=_lib.AstroState(hdr=0x90000, n_env=2 ** 30)), -106, 'int32'),
        (episodes, dict(ep=_episodes(n_env=2 ** 30, games=2)), -106, 'int32'),
        (explore, dict(s=_lib.AstroState(hdr=None, n_env=40)), -108, 'NULL'),
        (explore, dict(ex=_explore(policy=None)), -108, 'NULL'),
        (episodes, dict(ep=_episodes(winner=None)), -108, 'NULL'), (episodes, dict(ep=_episodes(tick_sum=None)), -108, 'NULL'),
        (explore, dict(s=_lib.AstroState(hdr=0x90008, n_env=40)), -109, 'aligned'),
        (episodes, dict(ep=_episodes(tick_sum=0x70004)), -109, 'aligned'),
        (episodes, dict(ep=_episodes(length=0x10002)), -109, 'aligned'),
        (explore, dict(control=None), -112, 'control is NULL'),
        (episodes, dict(reward=None), -112, 'reward or done'), (episodes, dict(done=None), -112, 'reward or done'),
        (episodes, dict(reward=P(0x1002)), -119, 'aligned'),
    ]
    codes = set()
    for fn, kw, code, word in cases:
        rc, msg = fn(**kw)
        assert rc == code and word in msg, (fn.__name__, kw, rc, msg)
        codes.add(rc)
    assert sorted(codes) == [-119, -112, -109, -108, -106, -105, -104, -103, -102, -101, -100]
    # the bounds themselves pass the scalar checks (and stop at the next one)
    assert explore(ex=_explore(nrandom=1, stay_out=1 << 53, stay_in=0), control=None)[0] == -112
    assert explore(ex=_explore(nrandom=6), control=None)[0] == -112
    # the documented order: scalars before pointers
    assert explore(ex=_explore(nrandom=9, policy=None), control=None)[0] == -103
    assert episodes(ep=_episodes(games=0, winner=None), reward=None)[0] == -105


def test_thresholds():
    so, si = actor.thresholds(0.02, 1.0, 0.1)
    # independently: exp by its series in exact rationals, to far below one unit of 2^-53
    def exp_neg(x, terms=40):
        x = Fraction(x)
        return sum((-x) ** k / math.factorial(k) for k in range(terms))
    for got, t in ((so, 1.0), (si, 0.1)):
        exact = exp_neg(Fraction(0.02 / t)) * 2 ** 53      # of the float64 quotient, exactly
        # both probabilities are in [0.5, 1), where a float64 is a whole number of 2^-53: the
        # ceiling adds nothing, and math.exp's error (below one unit in the last place) is all there is
        assert abs(got - exact) < 1, (got, float(exact))
        assert got == Fraction(math.exp(-0.02 / t)) * 2 ** 53
    assert (so, si) == (8828844759706715, 7374471028957529)
    assert actor.thresholds(0.02, float('inf'), float('inf')) == (1 << 53, 1 << 53)
    assert actor.thresholds(0.02, 0.0, 1e-9) == (0, 0)
    ts = [1e-3, 1e-2, 0.1, 0.5, 1.0, 10.0, 1e6, float('inf')]
    stays = [actor.thresholds(0.02, t, t)[0] for t in ts]
    assert stays == sorted(stays) and len(set(stays)) == len(stays) and stays[-1] == 1 << 53
    with pytest.raises(ValueError):
        actor.thresholds(0.0, 1.0, 0.1)
    with pytest.raises(ValueError):
        actor.thresholds(0.02, -1.0, 0.1)


P_IN, P_OUT = 1 - math.exp(-0.02), 1 - math.exp(-0.2)


def _five_checks(c, what):
    """entries / out ticks ~ 1 - exp(-dt / t_in), exits / in ticks ~ 1 - exp(-dt / t_out),
    entered controls uniform on 0..4, never 5, no transition on a t = 0 tick."""
    def band(hits, n, p):
        return abs(hits - n * p) <= 5 * math.sqrt(n * p * (1 - p))
    assert band(c['entries'], c['out_ticks'], P_IN), (what, c['entries'], c['out_ticks'])
    assert band(c['exits'], c['in_ticks'], P_OUT), (what, c['exits'], c['in_ticks'])
    assert int(c['hist'][:5].sum()) == c['entries']
    for k in range(5):
        assert band(int(c['hist'][k]), c['entries'], 0.2), (what, k, c['hist'])
    assert c['hist'][5] == 0
    assert c['t0_ticks'] > 0 and c['t0_transitions'] == 0
    # these bands exclude the other readings: an independent coin (the state
    # would move with epsilon = 0.1 and 1 - epsilon per tick) and a draw among 6 controls
    for n, p, wrong in ((c['out_ticks'], P_IN, 0.1), (c['in_ticks'], P_OUT, 0.9), (c['entries'], 0.2, 1 / 6)):
        assert abs(n * wrong - n * p) > 5 * math.sqrt(n * p * (1 - p)) + 5 * math.sqrt(n * wrong * (1 - wrong)), what


def test_reference_counts():
    """The reference's own EpsilonGreedy(1.0, 0.1), seeds 0..7, 200,000 ticks each."""
    z = gio.load('explore.npz')
    assert int(z['seeds']) == 8 and int(z['ticks']) == 200000 and int(z['game']) == 1500 and float(z['dt']) == 0.02
    c = {k: int(z[k].sum()) for k in ('out_ticks', 'entries', 'in_ticks', 'exits', 't0_ticks', 't0_transitions')}
    c['hist'] = z['hist'].sum(0)
    assert c['out_ticks'] + c['in_ticks'] + c['t0_ticks'] == 8 * 200000
    _five_checks(c, 'reference')


def test_explore_host_has_the_reference_statistics():
    """explore_host at the same length: 8 ships (4 envs of 2), 200,000 calls,
    the tick back at 0 every 1,500."""
    z = gio.load('explore.npz')
    ticks, game = int(z['ticks']), int(z['game'])
    so, si = actor.thresholds(float(z['dt']), float(z['t_in']), float(z['t_out']))
    policy = np.full((4, 2), -1, np.int8)
    control = np.zeros((4, 2), np.int8)
    tally = au.Tally()
    tick = np.zeros(4, np.int64)
    for k in range(ticks):
        tick[:] = k % game
        before = policy.copy()
        control[:] = 9
        actor.explore_host(policy, tick, control, k, so, si, seed=5, env_offset=3, nrandom=5)
        tally.add(before, policy, tick)
        assert ((control == 9) == (policy < 0)).all() and (control[policy >= 0] == policy[policy >= 0]).all()
    c = {k: getattr(tally, k) for k in ('out_ticks', 'entries', 'in_ticks', 'exits', 't0_ticks', 't0_transitions', 'hist')}
    assert c['out_ticks'] + c['in_ticks'] + c['t0_ticks'] == 8 * ticks
    _five_checks(c, 'explore_host')


def test_explore_host_edges():
    """Thresholds 2^53 and 0, nrandom 1 and 6, one transition per call, shards."""
    N, S = 50, 2
    tick = np.ones(N, np.int64)
    pol, ctl = np.full((N, S), -1, np.int8), np.full((N, S), 9, np.int8)
    actor.explore_host(pol, tick, ctl, 0, 1 << 53, 0, nrandom=5)
    assert (pol == -1).all() and (ctl == 9).all()                  # never enters
    actor.explore_host(pol, tick, ctl, 1, 0, 0, nrandom=6)
    assert (pol >= 0).all() and set(np.unique(pol)) == set(range(6)) and (ctl == pol).all()   # enters, and does not leave at once
    was = pol.copy()
    actor.explore_host(pol, np.zeros(N, np.int64), ctl, 2, 0, 0)
    assert (pol == was).all()                                      # tick 0: nothing moves
    actor.explore_host(pol, tick, ctl, 2, 0, 0)
    assert (pol == -1).all() and (ctl == was).all()                # leaves; the controls stay what they were
    actor.explore_host(pol, tick, ctl, 3, 0, 0, nrandom=1)
    assert (pol == 0).all()
    # a word equal to the threshold moves the state, a word one below it does not
    from astro_amd import replay
    k = (replay.random_words(np.arange(N * S, dtype=np.uint64), 21, 5) >> np.uint64(11)).reshape(N, S)
    kj = int(k[17, 1])
    for held in (False, True):
        for stay, moves in ((kj, True), (kj + 1, False)):
            pol = np.full((N, S), 3 if held else -1, np.int8)
            actor.explore_host(pol, tick, ctl, 5, *((actor.ONE, stay) if held else (stay, actor.ONE)), seed=21)
            assert (pol[17, 1] >= 0) == (held != moves)
            assert int(((pol >= 0) != held).sum()) == int((k >= np.uint64(stay)).sum())
    # two half batches with env_offset equal the whole
    so, si = actor.thresholds(0.02, 0.05, 0.05)
    whole = np.full((N, S), -1, np.int8)
    a, b = whole[:20].copy(), whole[20:].copy()
    for k in range(50):
        actor.explore_host(whole, tick, np.zeros((N, S), np.int8), k, so, si, seed=9, env_offset=100)
        actor.explore_host(a, tick[:20], np.zeros((20, S), np.int8), k, so, si, seed=9, env_offset=100)
        actor.explore_host(b, tick[20:], np.zeros((30, S), np.int8), k, so, si, seed=9, env_offset=120)
    assert (whole >= 0).any() and (whole < 0).any() and np.array_equal(whole, np.concatenate([a, b]))


def test_episodes_host_on_the_designed_schedule():
    """Two games per env: a win, a loss, a timeout, a tie at reward 1 (the first
    maximal ship), a game after ``games`` is full -- against values written by hand."""
    reward, done = au.schedule(6)
    h = actor.new_episodes_host(6, 2, au.GAMES)
    for t in range(au.T_DESIGNED):
        actor.episodes_host(h, reward[t], done[t])
    au.check_expect(h)
    assert (h['finished'] == h['got']).all() and (h['wins'].sum(1) <= h['finished']).all()
    # S = 1: the solo game's timeout reward 1 is a win of ship 0, a crash is none
    h = actor.new_episodes_host(2, 1, 1)
    actor.episodes_host(h, np.array([[1.0], [-1.0]], np.float32), np.array([2, 1], np.uint8))
    assert h['winner'].tolist() == [[0], [-1]] and h['ticks'].tolist() == [[1], [1]] and h['wins'].tolist() == [[1], [0]]


def test_python_surface():
    import astro_amd
    from astro_amd import train
    assert astro_amd.EpsilonGreedy is actor.EpsilonGreedy and astro_amd.Episodes is actor.Episodes
    assert astro_amd.QTrainer is train.QTrainer
    for name in ('play_q', 'qcontrols', 'rollout_q'):
        assert 'explore' in getattr(astro_amd.BatchedEnv, name).__code__.co_varnames
