"""One Q-network per ship on the device (astro_qvalues_ships,
include/astro_qduel.h) and what is built on it: the per-ship form of
``BatchedEnv.qvalues`` / ``qcontrols``, network and snapshot opponents in
``rollout_q`` / ``play_q`` / ``QTrainer``, and ``league.compare``.

The main yardstick is astro_qvalues itself: ship s of the per-ship form must
equal ``qvalues(net[s])`` bit for bit.  Truth (test 4) is qnet.forward64 on the
env's own features, within 4 e_ref of the network on those very states
(tests/qnet_util.py's rule).
"""
import functools

import numpy as np
import pytest
import torch

from astro_amd import BatchedEnv, DEFAULT_CONFIG, SOLO_CONFIG, actor, league, qnet, replay, train
from tests import golden_io as gio
from tests import qnet_util as qu

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARD = 64


@functools.lru_cache(maxsize=None)
def _weights():
    """A: the fixture's networks; B: another one (every weight of A scaled by its own factor)."""
    fx, _, _ = qu.fixture()
    rng = np.random.default_rng(11)
    other = {k: (np.asarray(v, np.float32) * (1.0 + 0.3 * rng.standard_normal(v.shape))).astype(np.float32)
             for k, v in fx['duo']['weights'].items()}
    return dict(A=fx['duo']['weights'], B=other, A1=fx['solo']['weights'])


@pytest.fixture(scope='module')
def nets():
    return {k: qnet.QNetwork.from_module(w, DEV) for k, w in _weights().items()}


def _live(n, dtype=torch.float32, cfg=DEFAULT_CONFIG, auto_reset=True):
    """n games after 150 random ticks: bullets in flight, games of every age."""
    env = BatchedEnv(cfg, n, device=DEV, b_cap=32, dtype=dtype, auto_reset=auto_reset)
    env.reset()
    env.rollout(150, 'random', seed=1)
    return env


def _bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def _guarded(shape, dtype=torch.float32):
    """A buffer of ``shape`` prefilled with NaN (0x55 for int8) followed by GUARD elements of the same."""
    n = int(np.prod(shape))
    fill = float('nan') if dtype.is_floating_point else 0x55
    flat = torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)
    return flat, flat[:n].view(shape)


def _untouched(flat, n):
    tail = flat[n:]
    return bool(torch.isnan(tail).all()) if flat.dtype.is_floating_point else bool((tail == 0x55).all())


@functools.lru_cache(maxsize=None)
def _single(n, dtype):
    """What astro_qvalues gives for A and for B on the live state of n envs:
    (q_A, q_B, ctl_A, ctl_B, and with epsilon 0.3 at seed 9, tick0 4: eps_A, eps_B) -- computed once."""
    a, b = (qnet.QNetwork.from_module(_weights()[k], DEV) for k in 'AB')
    env = _live(n, dtype)
    return (env.qvalues(a), env.qvalues(b), env.qcontrols(a), env.qcontrols(b), env.qcontrols(a, 0.3, 9, 4),
            env.qcontrols(b, 0.3, 9, 4))


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('n', [1, 33, 70])
def test_bit_identity_per_ship(nets, n, dtype):
    """1. qvalues((A, B)) is qvalues(A) for ship 0 and qvalues(B) for ship 1, bit for bit; qcontrols
    the same, greedy and with the coin."""
    A, B = nets['A'], nets['B']
    qa, qb, ca, cb, ea, eb = _single(n, dtype)
    env = _live(n, dtype)
    assert int(env.nbullets.sum()) > 0 or n == 1
    q = env.qvalues((A, B))
    assert q.shape == (n, 2, 6) and q.dtype == torch.float32
    assert _bits(q[:, 0]) == _bits(qa[:, 0]) and _bits(q[:, 1]) == _bits(qb[:, 1])
    assert n == 1 or _bits(qa[:, 1]) != _bits(qb[:, 1])              # A and B are different networks
    q2 = torch.zeros_like(q)
    c = env.qcontrols([A, B], q_out=q2)
    assert c.dtype == torch.int8 and _bits(q2) == _bits(q)
    assert torch.equal(c[:, 0], ca[:, 0]) and torch.equal(c[:, 1], cb[:, 1])
    e = env.qcontrols((A, B), 0.3, 9, 4)
    assert torch.equal(e[:, 0], ea[:, 0]) and torch.equal(e[:, 1], eb[:, 1])
    assert n < 33 or not torch.equal(e, c)                           # the coin did something
    # the same network for both ships is astro_qvalues outright
    assert _bits(env.qvalues((A, A))) == _bits(qa) and _bits(env.qvalues((B, B))) == _bits(qb)
    env.check_errors()


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('n', [1, 33, 70])
def test_bit_identity_solo(nets, n, dtype):
    A1 = nets['A1']
    env = _live(n, dtype, cfg=SOLO_CONFIG)
    want = env.qvalues(A1)
    assert want.shape == (n, 1, 6)
    assert _bits(env.qvalues((A1,))) == _bits(want)
    assert torch.equal(env.qcontrols((A1,)), env.qcontrols(A1))
    assert torch.equal(env.qcontrols([A1], 0.3, 9, 4), env.qcontrols(A1, 0.3, 9, 4))
    with pytest.raises(ValueError):
        env.qvalues((nets['A'],))
    with pytest.raises(ValueError):
        env.qvalues((A1, None))
    env.check_errors()


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('n', [1, 33, 70])
def test_skipped_ships(nets, n, dtype):
    """2. (A, None) and (None, B): the skipped ship's rows of q, its column of control and the guards
    behind both keep their bits; the other ship is astro_qvalues' bit for bit."""
    A, B = nets['A'], nets['B']
    qa, qb, ca, cb, _, _ = _single(n, dtype)
    env = _live(n, dtype)
    for form, ship, q1, c1 in (((A, None), 0, qa, ca), ((None, B), 1, qb, cb)):
        flat, out = _guarded((n, 2, 6))
        assert env.qvalues(form, out=out) is out
        assert _bits(out[:, ship]) == _bits(q1[:, ship])
        assert bool(torch.isnan(out[:, 1 - ship]).all()) and _untouched(flat, n * 12)
        flat, out = _guarded((n, 2, 6))
        c = env.qcontrols(form, q_out=out)
        assert torch.equal(c[:, ship], c1[:, ship]) and _bits(out[:, ship]) == _bits(q1[:, ship])
        assert bool(torch.isnan(out[:, 1 - ship]).all()) and _untouched(flat, n * 12)
        # the entry point itself on buffers of the test's own
        qflat, q = _guarded((n, 2, 6))
        cflat, ctl = _guarded((n, 2), torch.int8)
        env._qvalues_ships(env._per_ship(form), q, ctl, None, 0.0)
        assert torch.equal(ctl[:, ship], c1[:, ship]) and bool((ctl[:, 1 - ship] == 0x55).all())
        assert _untouched(cflat, n * 2) and _untouched(qflat, n * 12) and bool(torch.isnan(q[:, 1 - ship]).all())
        assert _bits(q[:, ship]) == _bits(q1[:, ship])
        cflat, ctl = _guarded((n, 2), torch.int8)                  # control only
        env._qvalues_ships(env._per_ship(form), None, ctl, None, 0.0)
        assert torch.equal(ctl[:, ship], c1[:, ship]) and bool((ctl[:, 1 - ship] == 0x55).all())
        assert _untouched(cflat, n * 2)
    env.check_errors()


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
def test_later_chunks_of_a_wave(nets, dtype):
    """3. 300 envs are 10 chunks of 32 per ship, the last one of 12 envs.  One workgroup (max_blocks 1)
    walks them with its four waves, ship after ship; two workgroups, one per ship: a wave's second
    and third chunk.  Equal bit for bit to the default launch of the same state."""
    A, B = nets['A'], nets['B']
    n = 300
    env = _live(n, dtype)
    for form in ((A, B), (A, None), (None, B)):
        nets_ = env._per_ship(form)
        qflat, q0 = _guarded((n, 2, 6))
        cflat, c0 = _guarded((n, 2), torch.int8)
        env._qvalues_ships(nets_, q0, c0, None, 0.0)
        for ship in (0, 1):
            if form[ship] is not None:
                assert _bits(q0[:, ship]) == _bits(env.qvalues(form[ship])[:, ship])
        for max_blocks in (1, 2, 3):
            qf, q = _guarded((n, 2, 6))
            cf, c = _guarded((n, 2), torch.int8)
            env._qvalues_ships(nets_, q, c, None, 0.0, max_blocks=max_blocks)
            assert _bits(qf) == _bits(qflat) and _bits(cf) == _bits(cflat), (form, max_blocks)
    env.check_errors()


def test_truth(nets):
    """4. qvalues((A, B)) against qnet.forward64 on the env's features and their ego swap, on the 70-env
    live state: within tol = 4 e_ref of each network on these states; controls by the argmax rule."""
    w = _weights()
    env = _live(70, torch.float64)
    f = env.features().cpu().numpy()
    views = [f, qnet.swap_ego(f)]
    q = torch.zeros((70, 2, 6), device=DEV)
    ctl = env.qcontrols((nets['A'], nets['B']), q_out=q).cpu().numpy()
    q = q.cpu().numpy().astype(np.float64)
    assert np.array_equal(ctl, np.argmax(q, -1))
    tols = {}
    for ship, name in ((0, 'A'), (1, 'B')):
        q64 = qu.q64_of_views(w[name], views)[:, ship]
        e_ref = float(np.abs(qu.q32_of_views(w[name], views)[:, ship].astype(np.float64) - q64).max())
        tols[name] = tol = 4.0 * e_ref
        err = float(np.abs(q[:, ship] - q64).max())
        print('ship %d (%s): max|q - q64| %.3g, e_ref %.3g, tol %.3g' % (ship, name, err, e_ref, tol))
        assert e_ref > 0 and err <= tol, (name, err, tol)
        checked, skipped = qu.check_argmax_rule(q64, ctl[:, ship], tol)
        print('ship %d: %d controls checked, %d of them undecided within 2 tol' % (ship, checked, skipped))
        assert checked == 70
    # and the networks disagree on these states, so a swapped pair would not pass
    other = qu.q64_of_views(w['B'], views)[:, 0]
    assert np.abs(q[:, 0] - other).max() > 100 * max(tols.values())


def test_scripted_opponent_unchanged(nets):
    """5. rollout_q(A, opponent='script') -- now (A, None) and the column fill -- is the loop of
    qcontrols(A), column fill and step, bit for bit."""
    A = nets['A']
    a, b = _live(64), _live(64)
    assert _bits(a.hdr) == _bits(b.hdr) and _bits(a.ships) == _bits(b.ships)
    reward, done, control = a.rollout_q(A, 40, opponent='script', seed=3)
    for t in range(40):
        c = b.qcontrols(A, 0.0, 3, t)
        c[:, 1] = b.controls('script', 3, t)[:, 1]
        assert torch.equal(c, control[t]), t
        _, r, d = b.step(c)
        assert _bits(r) == _bits(reward[t]) and torch.equal(d, done[t]), t
    for f in ('ships', 'ships_b', 'planets', 'bullets', 'hdr'):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    # with the coin too: ship 0 explores, ship 1 is the bot whatever the coin said
    reward, done, control = a.rollout_q(A, 5, 0.3, 7, 100, opponent='random')
    for t in range(5):
        c = b.qcontrols(A, 0.3, 7, 100 + t)
        c[:, 1] = b.controls('random', 7, 100 + t)[:, 1]
        assert torch.equal(c, control[t]), t
        _, r, d = b.step(c)
        assert _bits(r) == _bits(reward[t]) and torch.equal(d, done[t]), t
    a.check_errors()


def _merged(env, A, B, t, explore=None):
    """What a user had to do for two networks: two single-network calls and a column merge."""
    c = env.qcontrols(A, tick0=t)
    c[:, 1] = env.qcontrols(B, tick0=t)[:, 1]
    if explore is not None:
        explore.apply(c, t)
    return c


SHORT = gio.configs()['short']


def test_network_opponent_play_q(nets):
    """6a. play_q(A, opponent=B) is the written-out loop of two single-network qcontrols and a merge."""
    A, B = nets['A'], nets['B']
    cfg = SHORT._replace(max_time=1.0)
    a, b = (BatchedEnv(cfg, 64, device=DEV, b_cap=32) for _ in range(2))
    a.reset()
    b.reset()
    winner, length = a.play_q(A, opponent=B, games=1)
    ep = actor.Episodes(b, 1)
    t = 0
    while int(ep.got.min()) < 1:
        assert t < b.schedule.timeout_tick + 1 + 64
        for _ in range(64):
            _, r, d = b.step(_merged(b, A, B, t))
            ep.push(r, d)
            t += 1
    assert torch.equal(ep.winner.to(torch.int64), winner) and torch.equal(ep.ticks.to(torch.int64), length)
    assert _bits(a.hdr) == _bits(b.hdr) and _bits(a.ships) == _bits(b.ships)
    # the per-ship form without `opponent` is the same game; rollout_q takes a network opponent too
    c = BatchedEnv(cfg, 64, device=DEV, b_cap=32)
    c.reset()
    w2, l2 = c.play_q((A, B), games=1)
    assert torch.equal(w2, winner) and torch.equal(l2, length)
    reward, done, control = c.rollout_q(A, 3, opponent=B, tick0=t)
    for k in range(3):
        ctl = _merged(b, A, B, t + k)
        assert torch.equal(ctl, control[k])
        _, r, d = b.step(ctl)
        assert _bits(r) == _bits(reward[k]) and torch.equal(d, done[k])
    with pytest.raises(ValueError):
        c.play_q((A, None))
    a.check_errors()


def _small(opponent=None, **kw):
    env = BatchedEnv(SHORT, 64, device=DEV, b_cap=32)
    env.reset()
    net = qnet.QNetwork.from_module(_weights()['A'], DEV)
    buf = replay.ReplayBuffer(64, env.p_pad + env.b_cap, 2, 6, n_steps=2, device=DEV)
    eg = actor.EpsilonGreedy(env, t_in=0.2, t_out=0.1, seed=3)
    tr = None if opponent is None else train.QTrainer(env, net, buf, eg, n_samples=32, seed=5, opponent=opponent, **kw)
    return env, net, buf, eg, tr


def test_network_opponent_qtrainer(nets):
    """6b. QTrainer(opponent=B) for 8 ticks is the loop written out with two single-network qcontrols
    and a merge: the same weights, losses, ring and exploration state, bit for bit."""
    B = nets['B']
    env, net, buf, eg, tr = _small(opponent=B)
    assert tr.rival is B
    start = _bits(net.weights)
    for _ in range(8):
        tr.tick()
    env.check_errors()
    env2, net2, buf2, eg2, _ = _small()
    steps = 0
    for t in range(8):
        env2.features(out=buf2.head())
        control = _merged(env2, net2, B, t, explore=eg2)
        _, reward, done = env2.step(control)
        buf2.push(control, reward, done)
        if buf2.eligible_lower_bound() < 32:
            continue
        ids = buf2.sample(32, seed=5, draw=t)
        f, a, r, d, nf, term = buf2.gather(ids)
        loss = net2.sgd_step(f, a, net2.td_targets(r, d, nf, term), lr=1e-2)
        buf2.update_loss(ids, loss)
        steps += 1
    assert steps == tr.nstep > 0
    assert _bits(net.weights) == _bits(net2.weights) != start
    assert _bits(buf.loss) == _bits(buf2.loss) and _bits(buf.action) == _bits(buf2.action)
    assert _bits(eg.policy) == _bits(eg2.policy) and _bits(env.hdr) == _bits(env2.hdr)
    assert _bits(B.weights) == _bits(qnet.QNetwork.from_module(_weights()['B'], DEV).weights)   # the rival is fixed
    s = tr.validate(_fresh_eval(), games=1, opponent=B)
    assert s['games'] == 16 and abs(sum(s['wins']) + s['none'] - 1) < 1e-12


def _fresh_eval():
    ev = BatchedEnv(SHORT._replace(max_time=1.0), 16, device=DEV, b_cap=32)
    ev.reset()
    return ev


def test_snapshot_opponent():
    """7. opponent='snapshot', opponent_sync=2: the rival is the network right after optimisation steps
    2 and 4 and an older one after step 3; training moved the weights."""
    env, net, buf, eg, tr = _small(opponent='snapshot', opponent_sync=2)
    assert tr.rival is not net and tr.rival.weights.data_ptr() != net.weights.data_ptr()
    start = _bits(net.weights)
    assert _bits(tr.rival.weights) == start
    seen = {}
    for _ in range(12):
        before = tr.nstep
        out = tr.tick()
        if tr.nstep != before:
            assert tr.nstep == before + 1
            seen[tr.nstep] = (_bits(net.weights), _bits(tr.rival.weights), float(out['loss']))
        if tr.nstep == 4:
            break
    env.check_errors()
    assert sorted(seen) == [1, 2, 3, 4]
    assert seen[1][1] == start != seen[1][0]                         # not yet refreshed
    assert seen[2][1] == seen[2][0] and seen[4][1] == seen[4][0]     # refreshed: equal to the network
    assert seen[3][1] == seen[2][0] != seen[3][0]                    # frozen at step 2's weights
    assert all(np.isfinite(v[2]) for v in seen.values())
    assert np.isfinite(np.frombuffer(seen[4][0], np.float32)).all() and seen[4][0] != start
    assert len({v[0] for v in seen.values()}) == 4                   # every step moved the weights
    # ship 1 really plays the rival: the acting form is (net, rival)
    assert tuple(tr._acting) == (net, tr.rival) and tr._bot is None


def test_compare(nets):
    """8. league.compare(env, A, A): every game is counted once; and the seats are swapped."""
    A, B = nets['A'], nets['B']
    env = BatchedEnv(SHORT._replace(max_time=1.0), 64, device=DEV, b_cap=32)
    env.reset()
    r = league.compare(env, A, A, games=1)
    assert set(r) == {'games', 'wins_a', 'wins_b', 'none', 'p_better'}
    assert r['games'] == 2 * 64 and r['wins_a'] + r['wins_b'] + r['none'] == 2 * 64
    assert min(r['wins_a'], r['wins_b'], r['none']) >= 0 and 0.0 <= r['p_better'] <= 1.0
    assert r['p_better'] == league.p_better(r['wins_a'], r['wins_b'])
    # A against B from a fresh env is the two play_q legs, a's wins counted in either seat
    env = BatchedEnv(SHORT._replace(max_time=1.0), 64, device=DEV, b_cap=32)
    env.reset()
    r = league.compare(env, A, B, games=1)
    ref = BatchedEnv(SHORT._replace(max_time=1.0), 64, device=DEV, b_cap=32)
    ref.reset()
    w1, _ = ref.play_q(A, opponent=B, games=1)
    w2, _ = ref.play_q(B, opponent=A, games=1)
    assert r['wins_a'] == int((w1 == 0).sum()) + int((w2 == 1).sum())
    assert r['wins_b'] == int((w1 == 1).sum()) + int((w2 == 0).sum())
    assert r['games'] == 128 and r['none'] == 128 - r['wins_a'] - r['wins_b']
    env.check_errors()
