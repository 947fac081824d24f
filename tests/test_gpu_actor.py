"""The actor library on the device (include/astro_actor.h, astro_amd/actor.py,
astro_amd/train.py) against its numpy models (actor.explore_host,
actor.episodes_host), ``env.play`` and the loop written out by hand."""
import functools

import numpy as np
import pytest
import torch

from astro_amd import BatchedEnv, SOLO_CONFIG, actor, qnet, replay, train
from tests import actor_util as au
from tests import golden_io as gio
from tests import qtrain_util as qt

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
MARK = 9                      # no control: shows which entries a call wrote
PLAY_MAX_TIME = 6.0           # script against nothing, 140 games: wins of both ships and timeouts (asserted)


def _cfg(S):
    return gio.configs()['short'] if S == 2 else SOLO_CONFIG


def _env(S, N, **kw):
    env = BatchedEnv(_cfg(S), N, device=DEV, b_cap=32, **kw)
    env.reset()
    return env


@functools.lru_cache(maxsize=None)
def _net(S=2):
    return qnet.QNetwork.from_module(qt.weights_of('duo' if S == 2 else 'solo'), DEV)


def _marked(env):
    return torch.full((env.n_env, env.S), MARK, dtype=torch.int8, device=DEV)


def _host_apply(eg, policy, tick, draw):
    control = np.full(policy.shape, MARK, np.int8)
    actor.explore_host(policy, tick, control, draw, eg.stay_out, eg.stay_in, eg.seed, eg.env.env_offset, eg.nrandom)
    return control


# ---------------------------------------------------------------------------
# astro_explore

@pytest.mark.parametrize('N,S', [(70, 2), (70, 1), (1, 2), (1, 1)])
def test_explore_equals_the_host_on_a_stepped_env(N, S):
    """300 calls on an env that is really stepped, a third of the envs reset
    every 40 ticks: policy and control bit for bit explore_host's."""
    env = _env(S, N, env_offset=3)
    eg = actor.EpsilonGreedy(env, t_in=0.05, t_out=0.05, seed=12)
    assert (eg.policy == -1).all() and eg.policy.dtype == torch.int8 and tuple(eg.policy.shape) == (N, S)
    policy = np.full((N, S), -1, np.int8)
    rng = np.random.RandomState(N + S)
    tally = au.Tally()
    held_at_t0 = 0
    for t in range(300):
        if t and t % 40 == 0:
            third = np.arange(N) % 3 == (t // 40) % 3
            env.reset(mask=(third if N > 1 else np.ones(1, bool)).astype(np.uint8))
        tick = env.tick.cpu().numpy()
        before = policy.copy()
        control = eg.apply(_marked(env), draw=1000 + t)
        want = _host_apply(eg, policy, tick, 1000 + t)
        got, got_policy = control.cpu().numpy(), eg.policy.cpu().numpy()
        assert np.array_equal(got_policy, policy), t
        assert np.array_equal(got, want), t
        assert ((got == MARK) == (got_policy < 0)).all()          # untouched exactly where no policy is held
        t0 = tick == 0
        assert np.array_equal(got_policy[t0], before[t0])
        held_at_t0 += int((before[t0] >= 0).sum())
        tally.add(before, got_policy, tick)
        played = np.where(got == MARK, rng.randint(0, 6, size=(N, S)), got).astype(np.int8)
        env.step(torch.from_numpy(played).to(DEV))
    env.check_errors()
    assert tally.t0_ticks > 0 and tally.t0_transitions == 0 and held_at_t0 > 0
    assert tally.entries > 5 * S and tally.exits > 5 * S and tally.hist[5] == 0
    if N > 1:
        assert (tally.hist[:5] > 0).all()


def _ticking(N=70, S=2, **kw):
    """An env whose every tick counter is 1."""
    env = _env(S, N, **kw)
    env.step(torch.full((N, S), 2, dtype=torch.int8, device=DEV))
    assert (env.tick == 1).all()
    return env


def test_explore_edges():
    env = _ticking()
    never = actor.EpsilonGreedy(env, t_in=float('inf'), t_out=0.1)
    for t in range(50):
        c = never.apply(_marked(env), t)
    assert (never.policy == -1).all() and (c == MARK).all()
    for nrandom in (1, 6):
        # t_in and t_out tiny: enters on the first call, leaves on the second, enters again on the third
        eg = actor.EpsilonGreedy(env, t_in=1e-9, t_out=1e-9, seed=4, nrandom=nrandom)
        assert (eg.stay_out, eg.stay_in) == (0, 0)
        policy = np.full((70, 2), -1, np.int8)
        tick = np.ones(70, np.int64)
        for t in range(3):
            c = eg.apply(_marked(env), t)
            want = _host_apply(eg, policy, tick, t)
            assert np.array_equal(c.cpu().numpy(), want) and np.array_equal(eg.policy.cpu().numpy(), policy)
            if t == 1:
                assert (eg.policy == -1).all() and (c == MARK).all()
            else:
                assert (eg.policy >= 0).all() and torch.equal(c, eg.policy)
                assert set(np.unique(policy)) == set(range(nrandom))
        eg.reset()
        assert (eg.policy == -1).all()
    with pytest.raises(ValueError):
        actor.EpsilonGreedy(env, nrandom=7)
    with pytest.raises(ValueError):
        never.apply(torch.zeros((70, 2), dtype=torch.int32, device=DEV), 0)


def test_explore_threshold_is_inclusive():
    """A word equal to the threshold moves the state (k >= stay), a word one below it does not."""
    env, (N, S), seed, draw, j = _ticking(), (70, 2), 21, 5, (17, 1)
    k = (replay.random_words(np.arange(N * S, dtype=np.uint64), seed, draw) >> np.uint64(11)).reshape(N, S)
    kj = int(k[j])
    for held in (False, True):
        for stay, moves in ((kj, True), (kj + 1, False)):
            eg = actor.EpsilonGreedy(env, seed=seed)
            eg.policy.fill_(3 if held else -1)
            eg.c.stay_out, eg.c.stay_in = (actor.ONE, stay) if held else (stay, actor.ONE)
            eg.apply(_marked(env), draw)
            now_held = (eg.policy >= 0).cpu().numpy()
            assert bool(now_held[j]) == (held != moves), (held, stay)
            assert int((now_held != held).sum()) == int((k >= np.uint64(stay)).sum())


def test_explore_half_batches_equal_the_whole():
    whole = actor.EpsilonGreedy(_ticking(70), t_in=0.05, t_out=0.05, seed=8)
    a = actor.EpsilonGreedy(_ticking(35), t_in=0.05, t_out=0.05, seed=8)
    b = actor.EpsilonGreedy(_ticking(35, env_offset=35), t_in=0.05, t_out=0.05, seed=8)
    for t in range(40):
        cw, ca, cb = (eg.apply(_marked(eg.env), t) for eg in (whole, a, b))
        assert torch.equal(cw, torch.cat([ca, cb])) and torch.equal(whole.policy, torch.cat([a.policy, b.policy]))
    assert (whole.policy >= 0).any() and (whole.policy < 0).any() and not torch.equal(a.policy, b.policy)


def test_explore_is_a_function_of_state_and_draw():
    env = _ticking()
    eg = actor.EpsilonGreedy(env, t_in=0.05, t_out=0.05, seed=2)
    for t in range(10):
        eg.apply(_marked(env), t)
    start = eg.policy.clone()
    c1 = eg.apply(_marked(env), 77).clone()
    p1 = eg.policy.clone()
    eg.policy.copy_(start)
    c2 = eg.apply(_marked(env), 77)
    assert torch.equal(c1, c2) and torch.equal(p1, eg.policy) and not torch.equal(p1, start)
    eg.policy.copy_(start)
    eg.apply(_marked(env), 78)
    assert not torch.equal(p1, eg.policy)


def test_qcontrols_with_explore_is_greedy_then_apply():
    env, net = _ticking(), _net()
    eg1 = actor.EpsilonGreedy(env, t_in=0.05, t_out=0.05, seed=6)
    eg2 = actor.EpsilonGreedy(env, t_in=0.05, t_out=0.05, seed=6)
    greedy = env.qcontrols(net)
    for t in range(12):
        c1 = env.qcontrols(net, tick0=t, explore=eg1)
        c2 = eg2.apply(env.qcontrols(net), t)
        assert torch.equal(c1, c2) and torch.equal(eg1.policy, eg2.policy)
        held = eg1.policy >= 0
        assert torch.equal(c1[held], eg1.policy[held]) and torch.equal(c1[~held], greedy[~held])
    assert held.any() and (~held).any()
    with pytest.raises(ValueError, match='epsilon'):
        env.qcontrols(net, epsilon=0.1, explore=eg1)
    with pytest.raises(ValueError, match='another env'):
        _ticking(8).qcontrols(net, explore=eg1)
    # rollout_q passes it on: the same controls as the loop above would play
    twin = _ticking()
    eg3, eg4 = actor.EpsilonGreedy(env, seed=1, t_in=0.05), actor.EpsilonGreedy(twin, seed=1, t_in=0.05)
    _, _, ctl = env.rollout_q(net, 6, tick0=3, explore=eg3)
    for t in range(6):
        c = twin.qcontrols(net, tick0=3 + t, explore=eg4)
        assert torch.equal(c, ctl[t])
        twin.step(c)


# ---------------------------------------------------------------------------
# astro_episodes

EP_KEYS = ('length', 'got', 'winner', 'ticks', 'wins', 'finished', 'tick_sum')


def _ep_host(ep):
    return {k: getattr(ep, k).cpu().numpy() for k in EP_KEYS}


@pytest.mark.parametrize('S', [2, 1])
def test_episodes_equal_the_host_on_the_designed_schedule(S):
    N = 70
    reward, done = au.schedule(N)
    reward = np.ascontiguousarray(reward[:, :, :S])
    ep = actor.Episodes(_env(S, N), au.GAMES)
    h = actor.new_episodes_host(N, S, au.GAMES)
    for t in range(au.T_DESIGNED):
        ep.push(torch.from_numpy(reward[t]).to(DEV), torch.from_numpy(done[t]).to(DEV))
        actor.episodes_host(h, reward[t], done[t])
        got = _ep_host(ep)
        for k in EP_KEYS:
            assert got[k].dtype == h[k].dtype and np.array_equal(got[k], h[k]), (t, k)
    if S == 2:
        au.check_expect(_ep_host(ep))
    assert (h['got'] > au.GAMES).any() and (h['got'] == 0).any()
    s = ep.summary()
    played = h['winner'] > -2
    assert s['games'] == int(played.sum()) and abs(sum(s['wins']) + s['none'] - 1) < 1e-12
    assert s['median_ticks'] == float(np.median(h['ticks'][played]))
    ep.reset()
    assert (ep.winner == -2).all() and (ep.got == 0).all() and (ep.tick_sum == 0).all()


def test_episode_loop_equals_play():
    """env.play against the per-tick loop of controls, step and Episodes.push on a twin env."""
    cfg = gio.configs()['short']._replace(max_time=PLAY_MAX_TIME)
    N, G, bots = 70, 2, ('script', 'nothing')
    a = BatchedEnv(cfg, N, device=DEV, b_cap=32)
    b = BatchedEnv(cfg, N, device=DEV, b_cap=32)
    a.reset()
    b.reset()
    winner, length = a.play(bots, games=G)
    ep = actor.Episodes(b, G)
    t = 0
    timeouts = torch.zeros((), dtype=torch.int64, device=DEV)
    while t < 64 or int(ep.got.min()) < G:
        assert t < G * (b.schedule.timeout_tick + 1) + 64
        for _ in range(64):
            _, r, d = b.step(b.controls(bots, tick0=t))
            ep.push(r, d)
            timeouts += ((d == 2) & (ep.got <= G)).sum()
            t += 1
    b.check_errors()
    assert set(winner.unique().tolist()) == {-1, 0, 1}, 'the config no longer gives every outcome'
    assert int(timeouts) > 0 and (length < length.max()).any()
    assert torch.equal(ep.winner.to(torch.int64), winner) and torch.equal(ep.ticks.to(torch.int64), length)


def test_play_q_equals_the_rollouts_raw_arrays():
    cfg = gio.configs()['short']._replace(max_time=1.0)
    N, G, net = 33, 2, _net()
    a = BatchedEnv(cfg, N, device=DEV, b_cap=32)
    b = BatchedEnv(cfg, N, device=DEV, b_cap=32)
    a.reset()
    b.reset()
    T = 128
    assert G * (a.schedule.timeout_tick + 1) <= T
    winner, length = a.play_q(net, opponent='script', games=G)
    assert winner.dtype == length.dtype == torch.int64 and tuple(winner.shape) == tuple(length.shape) == (N, G)
    assert winner.device == a.device
    reward, done, _ = b.rollout_q(net, T, opponent='script')
    reward, done = reward.cpu().numpy(), done.cpu().numpy()
    for e in range(N):
        ends = np.nonzero(done[:, e])[0][:G]
        assert ends.size == G
        for g, k in enumerate(ends):
            r = reward[k, e]
            assert int(winner[e, g]) == (int(np.argmax(r)) if r.max() >= 1 else -1), (e, g)
            assert int(length[e, g]) == k + 1 - (0 if g == 0 else ends[g - 1] + 1), (e, g)
    with pytest.raises(RuntimeError, match='did not finish'):
        a.play_q(net, games=50, max_ticks=64)
    with pytest.raises(ValueError, match='opponent'):
        a.play_q(net, opponent='qbot')


# ---------------------------------------------------------------------------
# the loop

def _pieces(seed_explore=3):
    cfg = gio.configs()['short']
    N = 64
    env = BatchedEnv(cfg, N, device=DEV, b_cap=32)
    env.reset()
    net = qnet.QNetwork.from_module(qt.weights_of('duo'), DEV)
    buf = replay.ReplayBuffer(N, env.p_pad + env.b_cap, 2, 12, n_steps=4, device=DEV)
    eg = actor.EpsilonGreedy(env, t_in=0.2, t_out=0.1, seed=seed_explore)
    return env, net, buf, eg


def _trainer_run():
    env, net, buf, eg = _pieces()
    tr = train.QTrainer(env, net, buf, eg, n_samples=32, seed=5)
    outs = [tr.tick() for _ in range(20)]
    env.check_errors()
    return net.weights.cpu().numpy(), buf.loss.cpu().numpy(), eg.policy.cpu().numpy(), outs, tr


def test_qtrainer_is_the_loop_written_out_and_reproducible():
    w1, l1, p1, outs, tr = _trainer_run()
    w2, l2, p2, _, _ = _trainer_run()
    assert w1.tobytes() == w2.tobytes() and l1.tobytes() == l2.tobytes() and np.array_equal(p1, p2)
    # the README's loop from the same pieces
    env, net, buf, eg = _pieces()
    start = net.weights.cpu().numpy()
    trained = 0
    for t in range(20):
        env.features(out=buf.head())
        control = env.qcontrols(net, tick0=t, explore=eg)
        _, reward, done = env.step(control)
        buf.push(control, reward, done)
        if buf.eligible_lower_bound() >= 32:
            ids = buf.sample(32, seed=5, draw=t)
            f, a, r, d, nf, term = buf.gather(ids)
            loss = net.sgd_step(f, a, net.td_targets(r, d, nf, term), lr=1e-2)
            buf.update_loss(ids, loss)
            trained += 1
            o = outs[t]
            assert torch.is_tensor(o['loss']) and o['loss'].device.type == 'cuda' and int(o['n']) == 32
            assert float(o['loss']) == float(loss.sum())
        else:
            assert outs[t] is None
    assert trained == tr.nstep == 16 and buf.t == 20
    assert net.weights.cpu().numpy().tobytes() == w1.tobytes() and buf.loss.cpu().numpy().tobytes() == l1.tobytes()
    assert np.array_equal(eg.policy.cpu().numpy(), p1)
    assert w1.tobytes() != start.tobytes() and np.isfinite(w1).all() and np.isfinite(l1).any()
    # validate: play_q greedy and the summary
    ev = BatchedEnv(gio.configs()['short']._replace(max_time=1.0), 16, device=DEV, b_cap=32)
    ev.reset()
    s = tr.validate(ev, games=2, opponent='nothing')
    assert s['games'] == 32 and len(s['wins']) == 2 and abs(sum(s['wins']) + s['none'] - 1) < 1e-12
    assert 1 <= s['median_ticks'] <= ev.schedule.timeout_tick + 1
    with pytest.raises(ValueError, match='replay buffer'):
        train.QTrainer(ev, net, buf, None)
