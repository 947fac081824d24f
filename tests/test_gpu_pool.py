"""A pool of Q-networks over blocks of envs on the device (astro_qvalues_pool,
include/astro_qpool.h) and what is built on it: the pool form of
``BatchedEnv.qvalues`` / ``qcontrols`` / ``rollout_q`` / ``play_q``,
``league.tournament`` and ``QTrainer(opponent='pool')``.

The main yardstick is astro_qvalues itself: ship s of env i of a span must equal
``qvalues(that span's network)[i, s]`` bit for bit.  Truth (test 7) is
qnet.forward64 on the env's own features, within 4 e_ref of the network on those
very states (tests/qnet_util.py's rule).
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
COIN = (0.3, 9, 4)   # epsilon, seed, tick0


@functools.lru_cache(maxsize=None)
def _weights():
    """A: the fixture's networks; B, C: others (every weight of A scaled by its own factor); N0..N15:
    sixteen more of that kind; A1, B1: the solo ones."""
    fx, _, _ = qu.fixture()

    def other(base, seed):
        rng = np.random.default_rng(seed)
        return {k: (np.asarray(v, np.float32) * (1.0 + 0.3 * rng.standard_normal(v.shape))).astype(np.float32)
                for k, v in base.items()}
    duo, solo = fx['duo']['weights'], fx['solo']['weights']
    w = dict(A=duo, B=other(duo, 11), C=other(duo, 12), A1=solo, B1=other(solo, 13))
    w.update({'N%d' % k: other(duo, 100 + k) for k in range(16)})
    return w


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
def _single(n, dtype, names, cfg=DEFAULT_CONFIG):
    """What astro_qvalues gives for each named network on the live state of n envs: {name: (q, greedy
    controls, controls with the coin)} -- computed once and left unchanged."""
    env = _live(n, dtype, cfg)
    out = {}
    for name in names:
        net = qnet.QNetwork.from_module(_weights()[name], DEV)
        out[name] = (env.qvalues(net), env.qcontrols(net), env.qcontrols(net, *COIN))
    return out


def _expected(n, S, spans, names, ref):
    """(q, greedy, coin, covered mask [n, S]) of a pool from the per-network results: uncovered entries NaN / 0x55."""
    q = torch.full((n, S, 6), float('nan'), device=DEV)
    c = torch.full((n, S), 0x55, dtype=torch.int8, device=DEV)
    e = c.clone()
    mask = torch.zeros((n, S), dtype=torch.bool, device=DEV)
    for ship, lo, hi, k in spans:
        if k is None:
            continue
        rq, rc, re_ = ref[names[k]]
        q[lo:hi, ship], c[lo:hi, ship], e[lo:hi, ship] = rq[lo:hi, ship], rc[lo:hi, ship], re_[lo:hi, ship]
        mask[lo:hi, ship] = True
    return q, c, e, mask


def _check_pool(env, pool, names, ref, max_blocks=0):
    """Every way of calling the kernel on ``pool`` against the per-network reference, guards included."""
    n, S = env.n_env, env.S
    q1, c1, e1, mask = _expected(n, S, pool.spans, names, ref)
    coin = env.policy('random', COIN[1], COIN[2])
    for explore, eps, want in ((None, 0.0, c1), (coin, COIN[0], e1)):
        qflat, q = _guarded((n, S, 6))
        cflat, ctl = _guarded((n, S), torch.int8)
        env._qvalues_pool(pool, q, ctl, explore, eps, max_blocks=max_blocks)
        assert _bits(q) == _bits(q1) and _untouched(qflat, n * S * 6)          # NaN bits where nothing is covered
        assert torch.equal(ctl, want) and _untouched(cflat, n * S)
        assert bool(torch.isnan(q[~mask]).all()) and bool((ctl[~mask] == 0x55).all())
    cflat, ctl = _guarded((n, S), torch.int8)                                    # control only
    env._qvalues_pool(pool, None, ctl, None, 0.0, max_blocks=max_blocks)
    assert torch.equal(ctl, c1) and _untouched(cflat, n * S)
    qflat, q = _guarded((n, S, 6))                                               # q only
    env._qvalues_pool(pool, q, None, None, 0.0, max_blocks=max_blocks)
    assert _bits(q) == _bits(q1) and _untouched(qflat, n * S * 6)
    return q1, c1, e1, mask


def _spans_of(n):
    """Test 1's spans: unaligned edges, an empty span, a skipped one.  n = 70 is the issue's case."""
    if n == 70:
        return [(0, 0, 70, 0), (1, 0, 1, 1), (1, 1, 34, 0), (1, 34, 34, 2), (1, 34, 66, None), (1, 66, 70, 2)]
    if n == 33:
        return [(0, 0, 33, 0), (1, 0, 1, 1), (1, 1, 17, 0), (1, 17, 17, 2), (1, 17, 30, None), (1, 30, 33, 2)]
    return [(0, 0, 1, 2), (1, 0, 0, 0), (1, 0, 1, 1), (1, 1, 1, None)]


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('n', [1, 33, 70])
def test_bit_identity_per_span(nets, n, dtype):
    """1. Every covered (ship, env) is astro_qvalues' with that span's network, bit for bit: q, the greedy
    control and the control with the coin; uncovered entries and the guards keep their bits; control-only
    and q-only calls alike.  The public calls give the same."""
    names = ('A', 'B', 'C')
    ref = _single(n, dtype, names)
    env = _live(n, dtype)
    assert int(env.nbullets.sum()) > 0 or n == 1
    pool = league.Pool(env, [nets[k] for k in names], _spans_of(n))
    q1, c1, e1, mask = _check_pool(env, pool, names, ref)
    assert n == 1 or not bool(mask.all())
    if n > 1:
        assert _bits(ref['A'][0][:, 1]) != _bits(ref['B'][0][:, 1]) != _bits(ref['C'][0][:, 1])   # different networks
        assert not torch.equal(e1[mask], c1[mask])                                                # the coin did something
    flat, out = _guarded((n, 2, 6))
    assert env.qvalues(pool, out=out) is out and _bits(out) == _bits(q1) and _untouched(flat, n * 12)
    q2 = torch.full((n, 2, 6), float('nan'), device=DEV)
    c = env.qcontrols(pool, q_out=q2)
    assert c.dtype == torch.int8 and _bits(q2) == _bits(q1) and torch.equal(c[mask], c1[mask])
    assert torch.equal(env.qcontrols(pool, *COIN)[mask], e1[mask])
    assert env.qvalues(pool).shape == (n, 2, 6)
    env.check_errors()


EDGES = (31, 32, 33, 64, 65, 75)   # 300 envs: spans that end before, on and after a chunk's edge


def _edge_spans(ship):
    spans, at = [(1 - ship, 0, 300, 1)], 0
    for j, size in enumerate(EDGES):
        spans.append((ship, at, at + size, j % 3))
        at += size
    assert at == 300
    return spans


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
def test_chunk_edges_inside_a_span(nets, dtype):
    """2. 300 envs, one ship's spans of 31, 32, 33, 64, 65 and 75 envs cycling through three networks, the
    other ship one span: equal to the per-network qvalues slices."""
    names = ('A', 'B', 'C')
    ref = _single(300, dtype, names)
    env = _live(300, dtype)
    for ship in (1, 0):
        pool = league.Pool(env, [nets[k] for k in names], _edge_spans(ship))
        assert pool.covered
        _, _, _, mask = _check_pool(env, pool, names, ref)
        assert bool(mask.all())
    env.check_errors()


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
def test_later_chunks_and_the_one_workgroup_path(nets, dtype):
    """3. The same 300 envs with max_blocks 1 (one workgroup serves all seven spans one after the other and
    restages when the network changes), 2, 3 and 5 (shared workgroups; a wave's second and third chunk):
    the default launch's bytes, guards included."""
    names = ('A', 'B', 'C')
    env = _live(300, dtype)
    pool = league.Pool(env, [nets[k] for k in names], _edge_spans(1))
    part = league.Pool(env, [nets[k] for k in names], _spans_of(70))      # with a skipped and an empty span
    coin = env.policy('random', COIN[1], COIN[2])
    for pl in (pool, part):
        qflat, q0 = _guarded((300, 2, 6))
        cflat, c0 = _guarded((300, 2), torch.int8)
        env._qvalues_pool(pl, q0, c0, coin, COIN[0])
        assert bool(torch.isnan(q0).any()) == (pl is part)
        for max_blocks in (1, 2, 3, 5, 7, 8):
            qf, q = _guarded((300, 2, 6))
            cf, c = _guarded((300, 2), torch.int8)
            env._qvalues_pool(pl, q, c, coin, COIN[0], max_blocks=max_blocks)
            assert _bits(qf) == _bits(qflat) and _bits(cf) == _bits(cflat), max_blocks
    # and the default launch is right (test 2), also when capped
    _check_pool(env, pool, names, _single(300, dtype, names), max_blocks=2)
    env.check_errors()


def test_one_network_in_several_spans_and_sixteen_networks(nets):
    """4. The same network in several spans of both ships; 16 networks, one span each on ship 1, over 300
    envs: each slice against its own network."""
    names = ('A', 'B')
    env = _live(300)
    pool = league.Pool(env, [nets['A'], nets['B']], [(0, 0, 100, 0), (0, 100, 130, 1), (0, 130, 300, 0), (1, 0, 7, 0),
                                                     (1, 7, 200, 1), (1, 200, 300, 0)])
    _check_pool(env, pool, names, _single(300, torch.float32, names))
    names = ('A',) + tuple('N%d' % k for k in range(16))
    ref = _single(300, torch.float32, names)
    assert len({_bits(ref[k][0][:, 1]) for k in names}) == 17
    spans = [(0, 0, 300, 0)] + [(1, k * 300 // 16, (k + 1) * 300 // 16, 1 + k) for k in range(16)]
    pool = league.Pool(env, [nets[k] for k in names], spans)
    assert pool.spans == league.Pool.versus(env, nets['A'], [nets[k] for k in names[1:]]).spans
    for max_blocks in (0, 4, 17, 40):
        _check_pool(env, pool, names, ref, max_blocks=max_blocks)
    env.check_errors()


@pytest.mark.parametrize('n', [33, 300])
def test_degenerate_forms(nets, n):
    """5. One span per ship is the per-ship form: (A, B), and with ship 0 only (A, None)."""
    A, B = nets['A'], nets['B']
    env = _live(n)
    both = league.Pool(env, [A, B], [(0, 0, n, 0), (1, 0, n, 1)])
    assert _bits(env.qvalues(both)) == _bits(env.qvalues((A, B)))
    assert torch.equal(env.qcontrols(both, *COIN), env.qcontrols((A, B), *COIN))
    flat, out = _guarded((n, 2, 6))
    flat2, out2 = _guarded((n, 2, 6))
    env.qvalues(league.Pool(env, [A, B], [(0, 0, n, 0)]), out=out)
    env.qvalues((A, None), out=out2)
    assert _bits(flat) == _bits(flat2) and bool(torch.isnan(out[:, 1]).all())
    env.check_errors()


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('n', [1, 70])
def test_solo(nets, n, dtype):
    """6. A one-ship env: two solo networks over two spans."""
    names = ('A1', 'B1')
    ref = _single(n, dtype, names, SOLO_CONFIG)
    env = _live(n, dtype, cfg=SOLO_CONFIG)
    cut = n * 33 // 70
    pool = league.Pool(env, [nets[k] for k in names], [(0, 0, cut, 0), (0, cut, n, 1)])
    assert pool.covered
    q1, _, _, mask = _check_pool(env, pool, names, ref)
    assert q1.shape == (n, 1, 6) and bool(mask.all())
    with pytest.raises(ValueError):
        league.Pool(env, [nets['A']], [(0, 0, n, 0)])
    env.check_errors()


def test_truth(nets):
    """7. The 70-env case against qnet.forward64 on the env's features and their ego swap: within tol = 4
    e_ref of each network on these states; controls by the argmax rule."""
    w = _weights()
    names = ('A', 'B', 'C')
    env = _live(70, torch.float64)
    f = env.features().cpu().numpy()
    views = [f, qnet.swap_ego(f)]
    pool = league.Pool(env, [nets[k] for k in names], _spans_of(70))
    q = torch.zeros((70, 2, 6), device=DEV)
    ctl = env.qcontrols(pool, q_out=q).cpu().numpy()
    q = q.cpu().numpy().astype(np.float64)
    checked = 0
    for ship, lo, hi, k in pool.spans:
        if k is None or lo == hi:
            continue
        name = names[k]
        # e_ref: the float32 network's own distance from float64 on this ship of all 70 states, as
        # tests/test_gpu_league.py takes it
        all64 = qu.q64_of_views(w[name], views)[:, ship]
        e_ref = float(np.abs(qu.q32_of_views(w[name], views)[:, ship].astype(np.float64) - all64).max())
        q64 = all64[lo:hi]
        tol = 4.0 * e_ref
        err = float(np.abs(q[lo:hi, ship] - q64).max())
        print('ship %d [%d, %d) %s: max|q - q64| %.3g, e_ref %.3g, tol %.3g' % (ship, lo, hi, name, err, e_ref, tol))
        assert e_ref > 0 and err <= tol, (name, lo, hi, err, tol)
        assert np.array_equal(ctl[lo:hi, ship], np.argmax(q[lo:hi, ship], -1))
        n_checked, _ = qu.check_argmax_rule(q64, ctl[lo:hi, ship], tol)
        checked += n_checked
        # the other networks disagree on these states, so a span with the wrong network would not pass
        for wrong in names:
            if wrong != name:
                assert np.abs(q[lo:hi, ship] - qu.q64_of_views(w[wrong], views)[lo:hi, ship]).max() > 100 * tol
    assert checked == 70 + 1 + 33 + 4
    assert np.all(q[34:66, 1] == 0.0)                                  # the skipped span kept what it held
    env.check_errors()


SHORT = gio.configs()['short']


def _fresh(n, cfg=None):
    env = BatchedEnv(SHORT._replace(max_time=1.0) if cfg is None else cfg, n, device=DEV, b_cap=32)
    env.reset()
    return env


def test_play_q_with_a_pool(nets):
    """8. play_q on Pool.versus(env, A, [B, C]): envs [0, 32) play the games of play_q(A, opponent=B) on an
    identically reset env and envs [32, 64) those of play_q(A, opponent=C); rollout_q likewise."""
    A, B, C = nets['A'], nets['B'], nets['C']
    env, ref_b, ref_c = _fresh(64), _fresh(64), _fresh(64)
    pool = league.Pool.versus(env, A, [B, C])
    assert pool.spans == ((0, 0, 64, 0), (1, 0, 32, 1), (1, 32, 64, 2))
    winner, length = env.play_q(pool, games=1)
    wb, lb = ref_b.play_q(A, opponent=B, games=1)
    wc, lc = ref_c.play_q(A, opponent=C, games=1)
    assert torch.equal(winner[:32], wb[:32]) and torch.equal(length[:32], lb[:32])
    assert torch.equal(winner[32:], wc[32:]) and torch.equal(length[32:], lc[32:])
    assert not (torch.equal(wb, wc) and torch.equal(lb, lc))         # B and C play differently
    # a game lasts at most 50 ticks, so each play_q was one round of 64 ticks: the three envs are in step
    def same(f, dim):
        a, b, c = (getattr(e, f) for e in (env, ref_b, ref_c))
        return _bits(a.narrow(dim, 0, 32)) == _bits(b.narrow(dim, 0, 32)) \
            and _bits(a.narrow(dim, 32, 32)) == _bits(c.narrow(dim, 32, 32))
    assert same('hdr', 0) and same('ships', 1) and same('bullets', 0)
    reward, done, control = env.rollout_q(pool, 3, tick0=64)
    rb, db, cb = ref_b.rollout_q(A, 3, tick0=64, opponent=B)
    rc, dc, cc = ref_c.rollout_q(A, 3, tick0=64, opponent=C)
    for got, b, c in ((control, cb, cc), (reward, rb, rc), (done, db, dc)):
        assert _bits(got[:, :32]) == _bits(b[:, :32]) and _bits(got[:, 32:]) == _bits(c[:, 32:])
    assert same('hdr', 0) and same('ships', 1)
    part = league.Pool(env, [A, B], [(0, 0, 64, 0), (1, 0, 63, 1)])
    with pytest.raises(ValueError):
        env.play_q(part)
    with pytest.raises(ValueError):
        env.rollout_q(part, 1)
    for e in (env, ref_b, ref_c):
        e.check_errors()


def test_tournament(nets):
    """9. Three networks on 96 envs are six blocks of 16: the counts are those of six play_q((a, b)) runs on
    fresh identically reset 96-env envs, each restricted to its block."""
    trio = [nets['A'], nets['B'], nets['C']]
    r = league.tournament(_fresh(96), trio, games=1)
    assert set(r) == {'games', 'wins', 'none', 'p_better'}
    wins = [[0] * 3 for _ in range(3)]
    none = [[0] * 3 for _ in range(3)]
    pairs = league.Pool.pairs(3)
    assert pairs == [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)]
    for j, (a, b) in enumerate(pairs):
        ref = _fresh(96)
        w, _ = ref.play_q((trio[a], trio[b]), games=1)
        w = w[16 * j:16 * (j + 1)]
        wins[a][b] += int((w == 0).sum())
        wins[b][a] += int((w == 1).sum())
        none[a][b] += int((w == -1).sum())
        none[b][a] += int((w == -1).sum())
        ref.check_errors()
    assert r['wins'] == wins and r['none'] == none
    for a in range(3):
        for b in range(3):
            assert r['games'][a][b] == (0 if a == b else 32) == r['games'][b][a]
            assert r['wins'][a][b] + r['wins'][b][a] + r['none'][a][b] == r['games'][a][b]
            assert r['p_better'][a][b] == league.p_better(r['wins'][a][b], r['wins'][b][a])
        assert r['wins'][a][a] == 0 and r['none'][a][a] == 0 and r['p_better'][a][a] == 0.5
    assert sum(map(sum, wins)) > 0


def _small(opponent, **kw):
    env = BatchedEnv(SHORT, 64, device=DEV, b_cap=32)
    env.reset()
    net = qnet.QNetwork.from_module(_weights()['A'], DEV)
    buf = replay.ReplayBuffer(64, env.p_pad + env.b_cap, 2, 6, n_steps=2, device=DEV)
    eg = actor.EpsilonGreedy(env, t_in=0.2, t_out=0.1, seed=3)
    return env, net, buf, eg, train.QTrainer(env, net, buf, eg, n_samples=32, seed=5, opponent=opponent, **kw)


def test_qtrainer_pool_of_one_is_snapshot():
    """10a. pool_size=1, opponent_sync=2 for 12 ticks is opponent='snapshot', opponent_sync=2 bit for bit:
    weights, ring losses and actions, exploration state, env header."""
    env, net, buf, eg, tr = _small('pool', pool_size=1, opponent_sync=2)
    env2, net2, buf2, eg2, tr2 = _small('snapshot', opponent_sync=2)
    start = _bits(net.weights)
    assert type(tr._acting) is league.Pool and tr._acting.spans == ((0, 0, 64, 0), (1, 0, 64, 1))
    for _ in range(12):
        tr.tick()
        tr2.tick()
    assert tr.nstep == tr2.nstep > 2
    assert _bits(net.weights) == _bits(net2.weights) != start
    assert _bits(tr.rivals[0].weights) == _bits(tr2.rival.weights)
    assert _bits(buf.loss) == _bits(buf2.loss) and _bits(buf.action) == _bits(buf2.action)
    assert _bits(eg.policy) == _bits(eg2.policy) and _bits(env.hdr) == _bits(env2.hdr)
    env.check_errors()
    env2.check_errors()


def test_qtrainer_pool_round_robin():
    """10b. pool_size=2, opponent_sync=1: after optimisation steps 1..4 the slots hold the weights of steps
    (1, start), (1, 2), (3, 2), (3, 4); ship 1's spans are [0, 32) and [32, 64); every step moves the
    weights and they stay finite."""
    env, net, buf, eg, tr = _small('pool', pool_size=2, opponent_sync=1)
    assert len(tr.rivals) == 2 and tr.rival is None and tr._bot is None
    assert tr._acting.nets == (net, tr.rivals[0], tr.rivals[1])
    assert tr._acting.spans == ((0, 0, 64, 0), (1, 0, 32, 1), (1, 32, 64, 2))
    assert len({net.weights.data_ptr(), tr.rivals[0].weights.data_ptr(), tr.rivals[1].weights.data_ptr()}) == 3
    start = _bits(net.weights)
    assert _bits(tr.rivals[0].weights) == _bits(tr.rivals[1].weights) == start
    seen = {0: start}
    slots = {}
    for _ in range(12):
        before = tr.nstep
        out = tr.tick()
        if tr.nstep != before:
            assert tr.nstep == before + 1
            seen[tr.nstep] = _bits(net.weights)
            slots[tr.nstep] = (_bits(tr.rivals[0].weights), _bits(tr.rivals[1].weights))
            assert np.isfinite(float(out['loss']))
        if tr.nstep == 4:
            break
    env.check_errors()
    assert sorted(slots) == [1, 2, 3, 4]
    assert slots[1] == (seen[1], seen[0]) and slots[2] == (seen[1], seen[2])
    assert slots[3] == (seen[3], seen[2]) and slots[4] == (seen[3], seen[4])
    assert len(set(seen.values())) == 5                                # every step moved the weights
    assert np.isfinite(np.frombuffer(seen[4], np.float32)).all()
    s = tr.validate(_fresh(16), games=1, opponent=tr.rivals[1])       # validate is what it was
    assert s['games'] == 16 and abs(sum(s['wins']) + s['none'] - 1) < 1e-12
