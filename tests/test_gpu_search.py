"""The search's value reduction on the device (astro_search_values,
include/astro_search.h) and what is built on it: ``search.reduce``,
``fork.Lookahead`` with a leaf network and a reply ply, ``Lookahead.play``'s
recording, and ``train.Distiller``.

The kernel has two yardsticks and equals both bit for bit: ``reduce_host``
(numpy, one branch at a time) and ``reduce_torch`` (the torch ops ``Lookahead``
ran before the kernel).  The arrays are synthetic: the done patterns, the leaf
rows and the replies are built so that every rule of the header decides some
element.  Nothing here claims that anything learns."""
import ctypes

import numpy as np
import pytest
import torch

from astro_amd import BatchedEnv, DEFAULT_CONFIG, Recorder, _lib, fork, optim, qnet, search, train
from tests import qtrain_util as qt

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
A = 6
GUARD = 64
SHORT = DEFAULT_CONFIG._replace(max_time=3.0)            # 150 ticks at most
NEVER, TICK0, LAST, TWICE, TIMEOUT_P0, TIMEOUT_M0, ANY = range(7)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32}[a.dtype.itemsize])


def synthetic(N, K, R, S, ship, leaf, seed=0):
    """Numpy inputs of one call.  Every reward is noise, so a value read at a wrong tick, branch or ship is
    a wrong number; the done bytes follow one of seven patterns per branch."""
    rng = np.random.RandomState(seed + 1000 * N + 100 * K + 10 * R + S)
    M = N * A * R
    c = dict(reward0=rng.uniform(-2, 2, (M, S)).astype(np.float32), done0=np.zeros(M, np.uint8), reward=None, done=None)
    if K > 1:
        c['reward'] = rng.uniform(-2, 2, (K - 1, M, S)).astype(np.float32)
        c['done'] = np.zeros((K - 1, M), np.uint8)
    pattern = (np.arange(M) * 3 + np.arange(M) // 7) % 7

    def put(m, t, byte, r=None):
        (c['done0'] if t == 0 else c['done'][t - 1])[m] = byte
        if r is not None:
            (c['reward0'] if t == 0 else c['reward'][t - 1])[m, ship] = r
    for m, p in enumerate(pattern):
        if p == TICK0:
            put(m, 0, 1)
        elif p == LAST:
            put(m, K - 1, 1)
        elif p == TWICE:                       # opposite signs: the first must win
            t = rng.randint(0, max(K - 1, 1))
            put(m, t, 1, -1.5)
            if K > 1:
                put(m, rng.randint(t + 1, K), 1, 1.5)
        elif p == TIMEOUT_P0:
            put(m, rng.randint(0, K), 2, 0.0)
        elif p == TIMEOUT_M0:
            put(m, rng.randint(0, K), 2, -0.0)
        elif p == ANY:
            put(m, rng.randint(0, K), rng.choice([1, 2, 255]))
    if R > 1:
        # every third control's branches all end at tick 0, the worst reply at a chosen o
        for g in range(0, N * A, 3):
            for o in range(R):
                m = g * R + o
                c['done0'][m] = 1
                c['reward0'][m, ship] = rng.uniform(1, 2) - (3.0 if o == (g // 3) % R else 0.0)
    c['leaf'] = None
    if leaf:
        q = np.full((M, S, A), np.nan, np.float32)     # the other ship's rows must not be read
        q[:, ship] = rng.uniform(-1, 1, (M, A))
        q[np.arange(M), ship, np.arange(M) % A] += 2.5   # the maximum at each of the six positions
        c['leaf'] = q
    c['gamma'] = search.gammas(0.9, K)
    c['own'] = rng.randint(-1, A + 1, N).astype(np.int8)
    return c, pattern


def dev(c):
    return {k: None if v is None else torch.from_numpy(v).to(DEV) for k, v in c.items()}


def guarded(n, dtype, fill):
    big = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return big, big[GUARD:GUARD + n]


def launch(d, N, K, R, S, ship, value, own, control, first):
    """The library call itself, on the caller's output views."""
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()   # noqa: E731
    s = search.AstroSearch(reward0=ptr(d['reward0']), done0=ptr(d['done0']), reward=ptr(d['reward']), done=ptr(d['done']),
                           gamma=ptr(d['gamma']), leaf=ptr(d['leaf']), n_env=N, replies=R, nships=S, ship=ship, horizon=K)
    rc = search.load().astro_search_values(ctypes.byref(s), ptr(value), ptr(own), ptr(control), ptr(first),
                                           _lib.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize('R', [1, 6])
@pytest.mark.parametrize('K', [1, 2, 7])
@pytest.mark.parametrize('N', [1, 11, 77])       # 11: 66 branches, across a wave at a non-multiple of 6
def test_kernel_equals_both_mirrors_bit_for_bit(N, K, R):
    seen, worst = set(), set()
    for S, ship in ((1, 0), (2, 0), (2, 1)):
        for leaf in (False, True):
            c, pattern = synthetic(N, K, R, S, ship, leaf)
            seen |= set(pattern.tolist())
            d = dev(c)
            kw = dict(gamma=c['gamma'], ship=ship, replies=R, leaf=c['leaf'], own=c['own'])
            want_v, want_c, want_f = search.reduce_host(c['reward0'], c['done0'], c['reward'], c['done'], **kw)
            M = N * A * R
            bv, value = guarded(N * A, torch.float32, -7.25)
            bc, control = guarded(N, torch.int8, 99)
            bf, first = guarded(M, torch.int32, -77)
            before = {k: v.clone() for k, v in d.items() if v is not None}
            assert launch(d, N, K, R, S, ship, value, d['own'], control, first) == 0
            where = (N, K, R, S, ship, leaf)
            assert np.array_equal(bits(value.cpu().numpy().reshape(N, A)), bits(want_v)), where
            assert np.array_equal(control.cpu().numpy(), want_c), where
            assert np.array_equal(first.cpu().numpy(), want_f), where
            for big, n, fill in ((bv, N * A, -7.25), (bc, N, 99), (bf, M, -77)):      # the guard bands keep their bytes
                assert (big[:GUARD] == fill).all() and (big[GUARD + n:] == fill).all(), where
            for k, v in before.items():                                                # and no input is written
                assert torch.equal(v.view(torch.uint8), d[k].view(torch.uint8)), (where, k)
            # without the optional outputs nothing but the values is written
            bv2, value2 = guarded(N * A, torch.float32, -7.25)
            assert launch(d, N, K, R, S, ship, value2, None, None, None) == 0
            assert torch.equal(bv2.view(torch.int32), bv.view(torch.int32)), where
            # the checked call, and the torch formula
            tk = dict(gamma=d['gamma'], ship=ship, replies=R, leaf=d['leaf'])
            got_v, got_c, got_f = search.reduce(d['reward0'], d['done0'], d['reward'], d['done'], own=d['own'],
                                                first=True, **tk)
            assert torch.equal(got_v.view(torch.int32), value.view(N, A).view(torch.int32))
            assert torch.equal(got_c, control) and torch.equal(got_f, first)
            only = search.reduce(d['reward0'], d['done0'], d['reward'], d['done'], **tk)
            assert torch.is_tensor(only) and torch.equal(only.view(torch.int32), got_v.view(torch.int32))
            tv, tc = search.reduce_torch(d['reward0'], d['done0'], d['reward'], d['done'], own=d['own'], **tk)
            assert torch.equal(tv.contiguous().view(torch.int32), got_v.view(torch.int32)), where
            assert torch.equal(tc, got_c), where
            # what the construction promises
            if R > 1:
                b, _, _ = search.reduce_host(c['reward0'], c['done0'], c['reward'], c['done'], gamma=c['gamma'], ship=ship,
                                             replies=1, leaf=c['leaf'])
                worst |= set(b.reshape(N * A, R).argmin(1).tolist())
            if leaf and (want_f < 0).any():
                m = np.nonzero(want_f < 0)[0]
                assert not np.isnan(want_v).any() and set((m % A).tolist()) == set(c['leaf'][m, ship].argmax(1).tolist())
            twice = np.nonzero(pattern == TWICE)[0] if R == 1 else np.zeros(0, np.int64)
            for m in twice:
                assert want_v.reshape(-1)[m] < 0, 'the first of two done ticks'
            zero = np.nonzero(pattern == TIMEOUT_M0)[0] if R == 1 else np.zeros(0, np.int64)
            for m in zero:
                assert want_v.reshape(-1)[m] == 0 and np.signbit(want_v.reshape(-1)[m])
    if N * A * R >= 7:
        assert seen == set(range(7))
    if R > 1 and N > 1:
        assert worst == set(range(R))


def test_the_pick():
    """K = 1, every branch ends at tick 0: the values are the rewards, written out here."""
    rows = [([0, 5, 1, 5, 2, 3], 1, 1),      # own already maximal stays
            ([0, 5, 1, 5, 2, 3], 3, 3),      # own tied with an earlier maximal control stays
            ([0, 5, 1, 5, 2, 6], 1, 5),      # a strictly greater one later wins
            ([0, 5, 1, 5, 2, 3], 0, 1),      # two equal maxima: the first
            ([0, 5, 1, 5, 2, 3], 6, 1),      # own out of range: the first maximal
            ([0, 5, 1, 5, 2, 3], -1, 1),
            ([4, 4, 4, 4, 4, 4], 5, 5),      # all equal: own
            ([-3, -2, -1, -1, -2, -3], 0, 2),
            ([0.0, -0.0, 0, 0, 0, 0], 1, 1),  # zeros of both signs are equal
            ([1, 0, 0, 0, 0, 0], 127, 0), ([0, 0, 0, 0, 0, 1], -128, 5)] * 7      # 77 envs: every lane position
    v = torch.tensor([r for r, _, _ in rows], dtype=torch.float32, device=DEV)
    own = torch.tensor([o for _, o, _ in rows], dtype=torch.int8, device=DEV)
    want = torch.tensor([w for _, _, w in rows], dtype=torch.int8, device=DEV)
    N = len(rows)
    done0 = torch.ones(N * A, dtype=torch.uint8, device=DEV)
    gamma = torch.ones(2, dtype=torch.float32, device=DEV)
    got_v, got_c = search.reduce(v.view(N * A, 1), done0, gamma=gamma, own=own)
    assert torch.equal(got_v.view(torch.int32), v.view(torch.int32)) and torch.equal(got_c, want)
    assert np.array_equal(search.pick_host(v.cpu().numpy(), own.cpu().numpy()), want.cpu().numpy())
    assert torch.equal(search.reduce_torch(v.view(N * A, 1), done0, gamma=gamma, own=own)[1], want)


def test_no_envs_and_argument_errors():
    bv, value = guarded(8, torch.float32, -7.25)
    d = dict(reward0=None, done0=None, reward=None, done=None, gamma=None, leaf=None)
    assert launch(d, 0, 3, 1, 2, 0, value, None, None, None) == 0
    assert (bv == -7.25).all()
    e = lambda *shape, dt=torch.float32: torch.empty(shape, dtype=dt, device=DEV)   # noqa: E731
    g = torch.ones(4, dtype=torch.float32, device=DEV)
    v, c, f = search.reduce(e(0, 2), e(0, dt=torch.uint8), e(2, 0, 2), e(2, 0, dt=torch.uint8), gamma=g,
                            own=e(0, dt=torch.int8), first=True)
    assert tuple(v.shape) == (0, 6) and tuple(c.shape) == (0,) and tuple(f.shape) == (0,)
    r0, d0 = e(12, 2), e(12, dt=torch.uint8)
    for kw, word in ((dict(gamma=g), 'needed'), (dict(gamma=g[:2], ship=2), 'ship'),
                     (dict(gamma=g[:2].double()), 'gamma'), (dict(gamma=g[:2].cpu()), 'gamma'),
                     (dict(gamma=g[:2], leaf=e(12, 2, 6)[:, :, :]), None), (dict(gamma=g[:2], out=e(2, 5)), 'out'),
                     (dict(gamma=g[:2], own=e(2, dt=torch.int64)), 'own'), (dict(gamma=g[::2]), 'gamma')):
        if word is None:
            search.reduce(r0, d0, **kw)
            continue
        with pytest.raises(ValueError, match=word):
            search.reduce(r0, d0, **kw)
    with pytest.raises(ValueError, match='done0'):
        search.reduce(r0, d0.to(torch.int8), gamma=g[:2])
    out = e(2, 6)
    assert search.reduce(r0, d0, gamma=g[:2], out=out) is out


# ---------------------------------------------------------------------------
# Lookahead

def make(cfg=DEFAULT_CONFIG, n=77, age=150, **kw):
    env = BatchedEnv(cfg, n, device=DEV, auto_reset=True, b_cap=32, **kw)
    env.reset()
    if age:
        env.rollout(age, 'random', tick0=1 << 20)
    return env


def net_of(factor=1.0):
    return qnet.QNetwork.from_module(qt.weights_of('duo', factor=factor), DEV)


def i32(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope='module')
def busy():
    """77 aged envs, chosen from a larger batch and moved here by an indexed fork: in 40 of them ship 0
    loses within 20 ticks of script play (so some branch ends, and a search has something to avoid), in
    37 nothing ends within 24."""
    big = make(n=8192)
    snap = big.snapshot()
    reward, done = big.rollout(24, 'script')
    ended = done != 0
    lost = (ended[:20] & (reward[:20, :, 0] < 0)).any(0)
    lost &= ~(ended[:20] & (reward[:20, :, 0] >= 0)).any(0)
    ids = torch.cat([torch.nonzero(lost)[:40, 0], torch.nonzero(~ended.any(0))[:37, 0]]).cpu().numpy()
    assert ids.size == 77
    big.restore(snap)
    env = make(n=77, age=0, env_offset=9000)
    env.fork_from(big, ids, np.arange(77))
    return env


def test_lookahead_default_is_the_torch_formula_on_its_scratch_outputs(busy):
    la = fork.Lookahead(busy, ship=0, horizon=24, discount=0.9)
    v = la.values()
    r0, d0, r, d, q = la._outputs
    assert q is None and tuple(la._gamma.shape) == (25,)
    want = search.reduce_torch(r0, d0, r, d, gamma=la._gamma, ship=0)
    assert torch.equal(i32(v), i32(want))
    ended = (torch.cat([d0[None], d]) != 0).any(0)
    assert ended.any() and not ended.all() and (v != 0).any()
    c = la.controls()
    assert torch.equal(la.controls(values=v), c)
    own = busy.controls('script')[:, 0].contiguous()
    assert torch.equal(c, search.reduce_torch(r0, d0, r, d, gamma=la._gamma, ship=0, own=own)[1])
    # (one other first control seldom changes how these games end, so the search may well play the base's
    # controls here: the rule that departs from them is test_the_pick's)


@pytest.mark.parametrize('ship', [0, 1])
def test_lookahead_leaf_values_what_does_not_end(busy, ship):
    K = 6
    net = net_of()
    plain = fork.Lookahead(busy, ship=ship, horizon=K, discount=0.9)
    la = fork.Lookahead(busy, ship=ship, horizon=K, discount=0.9, leaf=net)
    v0, v = plain.values().clone(), la.values()
    r0, d0, r, d, q = la._outputs
    assert q is la.leaf_q and tuple(q.shape) == (77 * 6, 2, 6)
    nets = [None, None]
    nets[ship] = net
    fresh = la.scratch.qvalues(nets)       # the scratch env is still where the rollout left it
    assert torch.equal(i32(q[:, ship]), i32(fresh[:, ship])) and (q[:, 1 - ship] == 0).all()
    ended = (torch.cat([d0[None], d]) != 0).any(0).view(77, 6)
    assert ended.any() and not ended.all()
    want = torch.where(ended, v0, la._gamma[K] * fresh[:, ship].max(1).values.view(77, 6))
    assert torch.equal(i32(v), i32(want))
    assert torch.equal(i32(v), i32(search.reduce_torch(r0, d0, r, d, gamma=la._gamma, ship=ship, leaf=q)))
    # leaf is a plain attribute: another network, other values; None, the default's
    la.leaf = net_of(0.5)
    assert not torch.equal(la.values(), v)
    la.leaf = None
    assert torch.equal(i32(la.values()), i32(v0))


def test_lookahead_reply_ply():
    env = make(n=4)
    la = fork.Lookahead(env, ship=0, horizon=5, discount=0.9, reply=True, leaf=net_of())
    assert la.scratch.n_env == 4 * 36 and la.replies == 6
    assert np.array_equal(la.plan.src_ids, np.repeat(np.arange(4), 36))
    v = la.values()
    c = la._first_control.cpu().numpy().reshape(4, 6, 6, 2)
    assert (c[..., 0] == np.arange(6)[None, :, None]).all() and (c[..., 1] == np.arange(6)[None, None, :]).all()
    r0, d0, r, d, q = (None if t is None else t.cpu().numpy() for t in la._outputs)
    want, want_c, _ = search.reduce_host(r0, d0, r, d, gamma=la._gamma.cpu().numpy(), ship=0, replies=6, leaf=q,
                                         own=env.controls('script')[:, 0].cpu().numpy())
    assert np.array_equal(bits(v.cpu().numpy()), bits(want))
    assert np.array_equal(la.controls().cpu().numpy(), want_c)
    # the other ship's search mirrors the columns
    lb = fork.Lookahead(env, ship=1, horizon=2, reply=True)
    lb.values()
    c = lb._first_control.cpu().numpy().reshape(4, 6, 6, 2)
    assert (c[..., 1] == np.arange(6)[None, :, None]).all() and (c[..., 0] == np.arange(6)[None, None, :]).all()


def test_play_records_the_search_values():
    n, horizon = 8, 4
    env, twin = make(SHORT, n=n, age=0), make(SHORT, n=n, age=0)
    rec = Recorder(env, [0, 3, 7], ticks=64, q=6)
    winner, length = fork.Lookahead(env, horizon=horizon).play('script', games=1, record=rec)
    la = fork.Lookahead(twin, horizon=horizon)
    values = []
    for t in range(int(length.max())):
        v = la.values()
        values.append(v.cpu().numpy())
        c = twin.controls('script', tick0=t)
        c[:, 0] = la.controls(values=v)
        twin.step(c)
    for i in (0, 3, 7):
        game = rec.games[i][0]
        assert len(game.ticks) == int(length[i, 0])
        for t, tick in enumerate(game.ticks):
            data = tick.bot_data
            assert data[1] is None
            assert np.array_equal(bits(np.asarray(data[0]['q'], np.float32)), bits(values[t][i])), (i, t)
    with pytest.raises(ValueError, match='q=6'):
        fork.Lookahead(env, horizon=horizon).play('script', record=Recorder(env, [0], ticks=64))
    with pytest.raises(ValueError, match='of this env'):
        fork.Lookahead(env, horizon=horizon).play('script', record=Recorder(twin, [0], ticks=64, q=6))


# ---------------------------------------------------------------------------
# Distiller

def distiller(**kw):
    env = make(SHORT, n=64, age=40)
    net = net_of()
    teacher = fork.Lookahead(env, horizon=4)
    return env, net, teacher, train.Distiller(env, net, teacher, **kw)


def test_distiller_tick_is_one_gradient_step_on_the_repeated_batch():
    env, net, teacher, ds = distiller(lr=0.05)
    f, v = env.features(), teacher.values()
    w0 = net.weights.clone()
    loss, grad = net.clone().grad(f.repeat_interleave(6, 0), torch.arange(6, device=DEV).repeat(64), v.reshape(-1))
    got = ds.tick()
    assert got.dim() == 0 and torch.equal(got, loss.mean()) and ds.last is got and ds.nstep == 1
    assert torch.equal(net.weights, w0.add(grad, alpha=-0.05)) and not torch.equal(net.weights, w0)
    assert int(env.tick.max()) > 0 and teacher.leaf is None


def test_distiller_subset_optimizer_and_determinism():
    def run():
        env, net, teacher, ds = distiller(optimizer=optim.Adam(lr=1e-3), envs_per_step=10, seed=3)
        order = ds._order.cpu().numpy()
        assert sorted(order.tolist()) == list(range(64))
        f, v = env.features(), teacher.values()
        ids = torch.from_numpy(order[:10]).to(DEV)
        loss, _ = net.clone().grad(f[ids].repeat_interleave(6, 0), torch.arange(6, device=DEV).repeat(10),
                                   v[ids].reshape(-1))
        assert torch.equal(ds.tick(), loss.mean())
        ds.run(9)
        assert ds.nstep == 10
        return net.weights.cpu().numpy(), order
    (a, oa), (b, ob) = run(), run()
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(oa, ob)


def test_distiller_leaf_sync_copies_at_the_stated_steps():
    env, net, teacher, ds = distiller(leaf_sync=3, lr=0.05)
    assert teacher.leaf is not None and teacher.leaf is not net
    assert torch.equal(teacher.leaf.weights, net.weights)
    leaf = teacher.leaf
    for step in range(1, 8):
        before = leaf.weights.clone()
        ds.tick()
        assert teacher.leaf is leaf
        if step % 3 == 0:
            assert torch.equal(leaf.weights, net.weights) and not torch.equal(leaf.weights, before), step
        else:
            assert torch.equal(leaf.weights, before) and not torch.equal(leaf.weights, net.weights), step
    summary = ds.validate(make(SHORT, n=16, age=0), games=1, opponent='script')
    assert summary is not None
