"""Scripted seats on the device (astro_controls_seats, include/astro_seats.h)
and what is built on them: ``BatchedEnv.seat_controls``, the ``league.Seats``
form of ``qcontrols`` / ``play_q``, ``league.tournament`` with scripted
members, ``league.tune_script`` and ``QTrainer`` with a ladder.

Two yardsticks: the reference ScriptBot's decisions for the default and six
other argument sets (tests/golden/script_controls.npz, script_args.npz), and
astro_controls itself -- every covered byte must equal ``env.controls`` with
that seat's bot and arguments.
"""
import numpy as np
import pytest
import torch

from astro_amd import BatchedEnv, DEFAULT_CONFIG, SOLO_CONFIG, actor, league, qnet, replay, train
from tests import golden_io as gio
from tests.test_gpu_bots import _loaded
from tests.test_gpu_pool import _bits, _weights

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CFG = gio.configs()
SHORT = CFG['short']
SENTINEL = 0x55
Script = league.Script
ODD = Script(0.3, 0.9)


def _net(name):
    return qnet.QNetwork.from_module(_weights()[name], DEV)


# ---------------------------------------------------------------------------
# 1. the reference's decisions, default and non-default arguments, in one launch

@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_the_fixtures_on_the_device(dtype):
    tr = gio.Transitions('steps.npz')
    z = gio.load('script_args.npz')
    sets = [Script()] + [Script(d, t) for d, t in z['args'].tolist()]
    want = np.concatenate([gio.load('script_controls.npz')['control'][None], z['control']])   # [7, states, 2]
    checked = 0
    for name, idx in tr.groups():
        cfg = CFG[name]
        S, n = (1 if cfg.solo else 2), idx.size
        env = _loaded(tr, np.tile(idx, 7), cfg, dtype)
        seats = league.Seats(env, sets, [(s, b * n, (b + 1) * n, b) for b in range(7) for s in range(S)])
        assert seats.covered and seats.pool is None
        got = env.seat_controls(seats).cpu().numpy().reshape(7, n, S)
        assert np.array_equal(got, want[:, idx, :S]), name
        for b, sc in enumerate(sets[1:], 1):                 # script_args= of the whole-launch path
            whole = env.controls('script', script_args=sc.args).cpu().numpy()[:n]
            assert np.array_equal(whole, want[b, idx, :S]), (name, b)
        checked += 7 * n * S
    assert checked > 100000


# ---------------------------------------------------------------------------
# 2. bit identity with astro_controls on live games

A_, B_, C_ = Script(), ODD, Script(-0.05, 0.2)
SHIP0 = [(0, 63, A_), (63, 64, 'random'), (64, 65, 'nothing'), (65, 129, B_), (129, 129, C_), (129, 200, None),
         (200, 257, C_)]
SHIP1 = [(0, 64, B_), (65, 129, 'random'), (129, 257, A_)]     # env 64 has nobody


@pytest.mark.parametrize('dtype,p_pad,solo', [(torch.float32, 4, False), (torch.float64, 4, False),
                                              (torch.float32, 8, False), (torch.float64, 16, False),
                                              (torch.float32, 16, False), (torch.float32, 4, True),
                                              (torch.float64, 8, True)])
def test_seats_equal_astro_controls_bit_for_bit(dtype, p_pad, solo):
    cfg = SOLO_CONFIG if solo else DEFAULT_CONFIG
    n, seed, tick0 = 257, 77, 12
    env = BatchedEnv(cfg, n, device=DEV, b_cap=32, p_pad=p_pad, dtype=dtype, auto_reset=True, env_offset=40)
    env.reset()
    env.rollout(30, 'random', tick0=1 << 20)                     # games of several ages
    S = env.S
    cuts = [SHIP0] + ([SHIP1] if S == 2 else [])
    players, spans = [], []
    for s, cut in enumerate(cuts):
        for lo, hi, pl in cut:
            spans.append((s, lo, hi, None if pl is None else len(players)))
            players += [] if pl is None else [pl]
    seats = league.Seats(env, players, spans)
    assert seats.pool is None and not seats.covered and len(seats._seats) == len(spans)
    flat = torch.full((n * S + 64,), SENTINEL, dtype=torch.int8, device=DEV)
    out = flat[:n * S].view(n, S)
    assert env.seat_controls(seats, seed, tick0, out=out) is out
    want = torch.full((n, S), SENTINEL, dtype=torch.int8, device=DEV)
    refs = {}
    for s, cut in enumerate(cuts):
        for lo, hi, pl in cut:
            if pl is None:
                continue
            if pl not in refs:
                name = 'script' if isinstance(pl, Script) else pl
                refs[pl] = env.controls([name] * S, seed, tick0, script_args=pl.args if isinstance(pl, Script) else None)
            want[lo:hi, s] = refs[pl][lo:hi, s]
    assert torch.equal(out, want)
    assert bool((flat[n * S:] == SENTINEL).all())
    assert bool((out[129:200, 0] == SENTINEL).all()) and (S == 1 or int(out[64, 1]) == SENTINEL)
    # the three scripts disagree somewhere, so a seat's own arguments matter
    a, b, c = (refs[k] for k in (A_, B_, C_))
    assert int((a != b).sum()) > 0 and int((a != c).sum()) > 0
    env.check_errors()


# ---------------------------------------------------------------------------
# 3. composition with the networks' launch and with exploration

def _live(n, cfg=DEFAULT_CONFIG):
    env = BatchedEnv(cfg, n, device=DEV, b_cap=32, auto_reset=True)
    env.reset()
    env.rollout(150, 'random', seed=1)
    return env


def test_versus_script_is_the_per_ship_form_with_the_bot_merged_in():
    env, net = _live(300), _net('A')
    got = env.qcontrols(league.Seats.versus(env, net, ['script']), tick0=5)
    want = env.qcontrols((net, None), tick0=5)
    want[:, 1] = env.controls('script', tick0=5)[:, 1]
    assert torch.equal(got, want)


def test_a_mixed_table_equals_its_parts():
    n = 300
    env, a, b = _live(n), _net('A'), _net('B')
    snap = a.clone()
    seats = league.Seats.versus(env, a, [b, ODD, snap])
    assert seats.spans[1:] == ((1, 0, 100, 1), (1, 100, 200, 2), (1, 200, 300, 3)) and seats.covered
    q = torch.full((n, 2, 6), float('nan'), device=DEV)
    got = env.qcontrols(seats, tick0=7, q_out=q)
    qa, qb = env.qvalues(a), env.qvalues(b)
    ca, cb, cs = env.qcontrols(a), env.qcontrols(b), env.controls('script', script_args=ODD.args)
    want = torch.stack([ca[:, 0], torch.cat([cb[:100, 1], cs[100:200, 1], ca[200:, 1]])], 1)
    assert torch.equal(got, want)
    assert _bits(q[:, 0]) == _bits(qa[:, 0]) and _bits(q[:100, 1]) == _bits(qb[:100, 1])
    assert _bits(q[200:, 1]) == _bits(qa[200:, 1])
    assert bool(torch.isnan(q[100:200, 1]).all())                 # a scripted ship has no Q rows
    assert _bits(env.qvalues(seats, out=q.clone())) == _bits(q)
    # with exploration: the networks' entries as the pool's with the same exploration, the bot's untouched
    pool = league.Pool(env, [a, b, snap], [(0, 0, n, 0), (1, 0, 100, 1), (1, 200, 300, 2)])
    eg1 = actor.EpsilonGreedy(env, t_in=0.5, t_out=0.5, seed=3)
    eg2 = actor.EpsilonGreedy(env, t_in=0.5, t_out=0.5, seed=3)
    for t in range(4):
        g = env.qcontrols(seats, tick0=t, explore=eg1)
        w = env.qcontrols(pool, tick0=t, explore=eg2)
        assert torch.equal(g[100:200, 1], cs[100:200, 1])
        w[100:200, 1] = cs[100:200, 1]
        assert torch.equal(g, w)
    assert _bits(eg1.policy) == _bits(eg2.policy)
    assert int((g != want).sum()) > 0                              # exploration did change network entries


# ---------------------------------------------------------------------------
# 4. games

def _fresh(n, cfg=SHORT):
    env = BatchedEnv(cfg, n, device=DEV, b_cap=32, auto_reset=True)
    env.reset()
    return env


def test_play_q_of_default_scripts_is_play():
    n = 256
    want_w, want_l = _fresh(n).play(('script', 'script'), games=1)
    env = _fresh(n)
    got_w, got_l = env.play_q(league.Seats.versus(env, 'script', [Script()]))
    assert torch.equal(got_w, want_w) and torch.equal(got_l, want_l)
    assert int((got_w >= 0).sum()) > 0


def test_tournament_with_scripted_members_equals_its_pairs():
    n, net = 96, _net('A')
    members = [net, 'nothing', ODD]
    r = league.tournament(_fresh(n), members)
    wins = [[0] * 3 for _ in range(3)]
    none = [[0] * 3 for _ in range(3)]
    for j, (a, b) in enumerate(league.Pool.pairs(3)):
        env = _fresh(n)
        w = env.play_q(league.Seats.versus(env, members[a], [members[b]]))[0][j * n // 6:(j + 1) * n // 6, 0]
        wins[a][b] += int((w == 0).sum())
        wins[b][a] += int((w == 1).sum())
        for x, y in ((a, b), (b, a)):
            none[x][y] += int((w < 0).sum())
    assert r['wins'] == wins and r['none'] == none
    assert all(r['games'][a][b] == (0 if a == b else 32) for a in range(3) for b in range(3))
    assert sum(map(sum, wins)) > 0
    c = league.compare(_fresh(n), ODD, 'nothing')
    assert c['games'] == 2 * n and c['wins_a'] + c['wins_b'] + c['none'] == 2 * n


# ---------------------------------------------------------------------------
# 5. tune_script

def test_tune_script_is_the_walk_it_says():
    n, K, kw = 256, 2, dict(max_trials=300, threshold=0.9, max_mutations=2, scale=0.05)
    best, hist = league.tune_script(_fresh(n), candidates=K, seed=42, **kw)
    again = league.tune_script(_fresh(n), candidates=K, seed=42, **kw)
    assert (best, hist) == again and len(hist) == 2
    random = np.random.RandomState(42)
    env, cur = _fresh(n), Script().args
    for rnd in hist:
        cands = [league.mutate(cur, 0.05, random) for _ in range(K)]
        assert rnd['candidates'] == cands
        seats = league.Seats.versus(env, Script(**cur), [Script(**c) for c in cands])
        played = [[] for _ in range(K)]
        for _ in range(rnd['passes']):
            env.reset()
            w = env.play_q(seats)[0][:, 0].cpu().tolist()
            for j in range(K):
                played[j] += [None if x < 0 else x for x in w[j * n // K:(j + 1) * n // K]]
        for j in range(K):
            games = played[j][:kw['max_trials']]
            assert rnd['verdicts'][j] == league.find_better(games, kw['max_trials'], kw['threshold']), j
            used = games[:rnd['games'][j]]
            assert rnd['wins'][j] == [used.count(0), used.count(1), used.count(None)]
        better = [j for j in range(K) if rnd['verdicts'][j] == 1]
        cur = cands[better[0]] if better else cur
        assert rnd['best'] == cur
    assert best == cur


# ---------------------------------------------------------------------------
# 6. QTrainer

def _small(opponent):
    env = BatchedEnv(SHORT, 64, device=DEV, b_cap=32)
    env.reset()
    net = _net('A')
    buf = replay.ReplayBuffer(64, env.p_pad + env.b_cap, 2, 6, n_steps=2, device=DEV)
    eg = actor.EpsilonGreedy(env, t_in=0.2, t_out=0.1, seed=3)
    return env, net, buf, eg, train.QTrainer(env, net, buf, eg, n_samples=32, seed=5, opponent=opponent)


def test_qtrainer_ladder():
    """200 ticks against a ladder; opponent='script' is bit for bit opponent=['script']."""
    runs = [_small('script'), _small(['script'])]
    assert type(runs[1][4]._acting) is league.Seats and runs[0][4]._bot == 'script'
    start = _bits(runs[0][1].weights)
    for _ in range(200):
        for r in runs:
            r[4].tick()
    (env, net, buf, eg, tr), (env2, net2, buf2, eg2, tr2) = runs
    assert tr.nstep == tr2.nstep > 100
    assert _bits(net.weights) == _bits(net2.weights) != start
    assert _bits(buf.loss) == _bits(buf2.loss) and _bits(buf.action) == _bits(buf2.action)
    assert _bits(eg.policy) == _bits(eg2.policy) and _bits(env.hdr) == _bits(env2.hdr)
    env.check_errors()
    env2.check_errors()
    env, net, buf, eg, tr = _small(['nothing', ODD, 'script', _net('B')])
    assert tr._acting.spans[1:] == ((1, 0, 16, 1), (1, 16, 32, 2), (1, 32, 48, 3), (1, 48, 64, 4))
    for _ in range(200):
        tr.tick()
    assert tr.nstep > 100 and bool(torch.isfinite(net.weights).all()) and _bits(net.weights) != start
    env.check_errors()
