"""The device replay buffer (include/astro_replay.h, astro_amd/replay.py)
against its numpy model (replay.push_host, replay.sample_host).

Every output buffer holds NaN (or, for ids, a sentinel) before the call and is
followed by 64 guard elements; the sampling workspace is filled with 0xFF
bytes before every call."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from astro_amd import BatchedEnv, _lib, qnet, replay
from tests import golden_io as gio
from tests import qtrain_util as qt

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARD = 64
SENTINEL = -7
META = ('action', 'reward', 'discount', 'next', 'loss', 'wstart')


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _meta(buf):
    return {k: getattr(buf, k).cpu().numpy() for k in META}


def _assert_meta(buf, h, what):
    got = _meta(buf)
    for k in META:
        assert _same(got[k], h[k]), (what, k, np.argwhere(_bits(got[k]) != _bits(h[k]))[:4])


def _load(buf, h, t):
    """Put a host state into the device buffer."""
    for k in META:
        getattr(buf, k).copy_(torch.from_numpy(h[k]))
    buf.t = int(t)


def _dirty_workspace(buf):
    need = int(_lib.load_replay().astro_replay_sample_workspace_bytes(ctypes.byref(buf.c)))
    buf._workspace = torch.full(((need + 3) // 4,), -1, dtype=torch.int32, device=DEV).view(torch.float32)
    return buf._workspace


def _sample(buf, n, seed, draw):
    """buf.sample into a guarded sentinel buffer with a dirty workspace: the ids as numpy."""
    _dirty_workspace(buf)
    out = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    ids = buf.sample(n, seed, draw, out=out[:n])
    count = buf.last_count()
    torch.cuda.synchronize()
    assert ids.shape[0] in (n, count) and count <= n
    assert (out[count:] == SENTINEL).all(), 'an element past the count changed'
    return out[:count].cpu().numpy()


def _host_ids(h, t, n, seed, draw):
    """sample_host, and the guard against a last-place difference between two
    float64 logs: E moved by 4 ulp either way (3 for the device library's
    documented bound, 1 for numpy's) must give the same set.  That is a
    property of the inputs alone; the seeds below were picked so that it holds."""
    want = replay.sample_host(h['loss'], h['next'], t, n, seed, draw)
    for ulps in (-4, 4):
        assert np.array_equal(want, replay.sample_host(h['loss'], h['next'], t, n, seed, draw, ulps)), (seed, draw, ulps)
    return want


# ---------------------------------------------------------------------------
# push

N_DESIGNED, TICKS_DESIGNED, STEPS_DESIGNED = 77, 10, 7


@functools.lru_cache(maxsize=None)
def _schedule(S):
    """60 ticks of N = 77 envs (one wave and a ragged tail), n_steps 7: env 0 is
    never done, env 1 is done on a window's first tick, env 2 exactly when
    L == n_steps, env 3 on three consecutive ticks, env 4 with both codes, the
    others at random with codes 1 and 2."""
    rng = np.random.RandomState(3 + S)
    T, N = 60, N_DESIGNED
    done = np.where(rng.rand(T, N) < 0.08, rng.randint(1, 3, size=(T, N)), 0).astype(np.uint8)
    done[:, :5] = 0
    done[7, 1] = 1          # windows of env 1: ticks 0..6 (closed by L == 7), then tick 7 alone
    done[6, 2] = 2          # L == n_steps and done at once
    done[10:13, 3] = 1
    done[20, 4], done[33, 4] = 1, 2
    reward = rng.uniform(0.1, 1.0, size=(T, N, S)).astype(np.float32) * rng.choice([-1, 1], size=(T, N, S))
    control = rng.randint(0, 6, size=(T, N, S)).astype(np.int8)
    assert set(np.unique(done)) == {0, 1, 2} and (reward != 0).all()
    return control, reward.astype(np.float32), done


@pytest.fixture(scope='module')
def designed():
    """The designed schedule pushed through the device, S = 2: (buffer, host state)."""
    control, reward, done = _schedule(2)
    buf = replay.ReplayBuffer(N_DESIGNED, 3, 2, TICKS_DESIGNED, n_steps=STEPS_DESIGNED, discount=0.995, device=DEV)
    h = replay.new_host(N_DESIGNED, 2, TICKS_DESIGNED)
    for t in range(control.shape[0]):
        buf.push(torch.from_numpy(control[t]).to(DEV), torch.from_numpy(reward[t]).to(DEV),
                 torch.from_numpy(done[t]).to(DEV))
        replay.push_host(h, t, control[t], reward[t], done[t], STEPS_DESIGNED, 0.995)
    _assert_meta(buf, h, 'designed')
    return buf, h


@pytest.mark.parametrize('S', [2, 1])
def test_push_designed_schedule(S):
    control, reward, done = _schedule(S)
    buf = replay.ReplayBuffer(N_DESIGNED, 3, S, TICKS_DESIGNED, n_steps=STEPS_DESIGNED, discount=0.995, device=DEV)
    buf.features.fill_(float('nan'))
    h = replay.new_host(N_DESIGNED, S, TICKS_DESIGNED)
    _assert_meta(buf, h, 'initial')
    seen = dict(first=False, full=False)
    for t in range(control.shape[0]):
        w = h['wstart'].copy()
        seen['first'] |= bool(((w == t) & (done[t] != 0)).any())
        seen['full'] |= bool(((t - w + 1 == STEPS_DESIGNED) & (done[t] != 0)).any())
        assert buf.t == t and buf.head().data_ptr() == buf.features[t % TICKS_DESIGNED].data_ptr()
        buf.push(torch.from_numpy(control[t]).to(DEV), torch.from_numpy(reward[t]).to(DEV),
                 torch.from_numpy(done[t]).to(DEV))
        replay.push_host(h, t, control[t], reward[t], done[t], STEPS_DESIGNED, 0.995)
        _assert_meta(buf, h, 'tick %d' % t)      # rows never written keep the initial state, too
    assert seen['first'] and seen['full'] and buf.t == 60 == 6 * TICKS_DESIGNED
    assert h['wstart'][0] == 56 and (h['next'][:, 0] != -1).all()           # the env that is never done
    assert (h['next'] == -1).any() and (h['next'] == -2).any()
    assert torch.isnan(buf.features).all(), 'push wrote a feature'


def test_push_live_env():
    """200 envs of the fixture's config, random controls, 320 ticks (a game
    lasts 150 ticks at most): the observation goes straight into the ring."""
    cfg = gio.configs()['short']
    N, T = 200, 320
    env = BatchedEnv(cfg, N, device=DEV, b_cap=32)
    env.reset()
    rows = env.p_pad + env.b_cap
    buf = replay.ReplayBuffer(N, rows, 2, 10, n_steps=7, discount=0.995, device=DEV)
    h = replay.new_host(N, 2, 10)
    g = torch.Generator().manual_seed(5)
    ends = np.zeros(N, np.int64)
    for t in range(T):
        env.features(out=buf.head())
        apart = env.features()
        control = torch.randint(0, 6, (N, 2), generator=g).to(torch.int8).to(DEV)
        _, reward, done = env.step(control)
        buf.push(control, reward, done)
        assert torch.equal(buf.features[t % 10].view(torch.int32), apart.view(torch.int32)), t
        d = done.cpu().numpy()
        replay.push_host(h, t, control.cpu().numpy(), reward.cpu().numpy(), d, 7, 0.995)
        ends += d != 0
        if t % 16 == 15 or t == T - 1:
            _assert_meta(buf, h, 'tick %d' % t)
    env.check_errors()
    assert ends.min() >= 2
    assert (h['next'] == -1).any() and (h['reward'] != 0).any()


# ---------------------------------------------------------------------------
# eligibility

def test_eligibility_follows_the_head():
    N, S, ticks, n_steps = 5, 2, 6, 3
    buf = replay.ReplayBuffer(N, 2, S, ticks, n_steps=n_steps, device=DEV)
    h = replay.new_host(N, S, ticks)
    rng = np.random.RandomState(1)
    m = ticks * N * S
    closed_then_sampled = 0
    before = None
    assert _sample(buf, m + 5, 1, 0).size == 0                        # nothing written
    for t in range(20):
        done = (rng.rand(N) < 0.25).astype(np.uint8)
        control = rng.randint(0, 6, size=(N, S)).astype(np.int8)
        reward = rng.uniform(-1, 1, size=(N, S)).astype(np.float32)
        buf.push(control, reward, done)
        replay.push_host(h, t, control, reward, done, n_steps)
        ok = replay.eligible_host(h['next'], t + 1, S)
        head = (t + 1) % ticks
        assert not ok[head].any() and not ok[h['next'] == -2].any() and not ok[h['next'] == head].any()
        if t + 1 < ticks:
            assert not ok[t + 1:].any()
        ids = _sample(buf, m + 5, seed=1, draw=t)
        assert np.array_equal(ids, np.nonzero(ok.ravel())[0]), t      # the count and the whole eligible set
        if before is not None:
            closed_then_sampled += int((before & ok).sum())
        # entries closed by this push without a done wait for their next state: the head row
        before = np.repeat(((h['next'] == head) & (np.arange(ticks) != head)[:, None])[:, :, None], S, 2)
        assert not (before & ok).any()
    assert closed_then_sampled > 0


# ---------------------------------------------------------------------------
# selection

def _synthetic(N, ticks, S, t, rng):
    """A host state with arbitrary next rows (-2, -1 or any row)."""
    h = replay.new_host(N, S, ticks)
    h['next'][:] = rng.randint(-2, ticks, size=(ticks, N))
    return h


def _losses(pattern, shape, rng):
    pos = rng.exponential(1.0, size=shape).astype(np.float32) + np.float32(1e-3)
    if pattern == 'unscored':
        return np.full(shape, np.inf, np.float32)
    if pattern == 'scored':
        return pos
    kind = rng.randint(0, 10, size=shape)
    return np.where(kind < 2, np.float32(np.inf), np.where(kind < 4, np.float32(0), pos)).astype(np.float32)


@pytest.fixture(scope='module')
def wide():
    """N = 3,001, ticks 12, S = 2: 72,024 ids over 71 tiles, 29 pushes so far."""
    rng = np.random.RandomState(21)
    h = _synthetic(3001, 12, 2, 29, rng)
    buf = replay.ReplayBuffer(3001, 1, 2, 12, n_steps=7, device=DEV)
    return buf, h, 29


# (seed, draw) per case: picked on the CPU so that _host_ids' guard holds
@pytest.mark.parametrize('pattern,seed', [('unscored', 11), ('mixed', 12), ('scored', 13)])
@pytest.mark.parametrize('which', ['designed', 'wide'])
def test_selection_equals_the_host(designed, wide, which, pattern, seed):
    buf, h0, t = (designed[0], designed[1], 60) if which == 'designed' else wide
    h = dict(h0, loss=_losses(pattern, h0['loss'].shape, np.random.RandomState(seed)))
    _load(buf, h, t)
    eligible = int(replay.eligible_host(h['next'], t, 2).sum())
    assert eligible > 64
    ok = replay.eligible_host(h['next'], t, 2).ravel()
    cls, _ = replay.keys_host(h['loss'].ravel()[ok], np.nonzero(ok)[0], seed, 0)
    inside = int((cls == 0).sum() + (cls == 1).sum() // 2)      # the threshold among the scored ones, if there are any
    for draw, n in enumerate([1, 64, 1000, eligible - 1, eligible, eligible + 5, inside]):
        want = _host_ids(h, t, n, seed, draw)
        got = _sample(buf, n, seed, draw)
        assert want.shape[0] == min(n, eligible) and (np.diff(want) > 0).all()
        assert _same(got, want), (which, pattern, n, got[:8], want[:8])
    _load(buf, h0, t)


def test_ties_at_the_threshold(designed):
    buf, h0, t = designed[0], designed[1], 60
    ok = np.nonzero(replay.eligible_host(h0['next'], t, 2).ravel())[0]
    rng = np.random.RandomState(8)
    some = np.sort(rng.choice(ok, size=40, replace=False))
    loss = np.zeros(h0['loss'].size, np.float32)
    loss[some] = rng.uniform(0.5, 2.0, size=40).astype(np.float32)
    h = dict(h0, loss=loss.reshape(h0['loss'].shape))
    _load(buf, h, t)
    rest = np.setdiff1d(ok, some)
    want = np.sort(np.concatenate([some, rest[:60]])).astype(np.int32)
    assert _same(replay.sample_host(h['loss'], h['next'], t, 100, 5, 6), want)
    assert _same(_sample(buf, 100, 5, 6), want)
    # more unscored entries than n: a subset of them, the host's
    loss = np.full(h0['loss'].size, np.inf, np.float32)
    loss[some] = 1.0
    h = dict(h0, loss=loss.reshape(h0['loss'].shape))
    _load(buf, h, t)
    want = _host_ids(h, t, 100, 5, 7)
    assert not np.isin(want, some).any() and ok.size - 40 > 100
    assert _same(_sample(buf, 100, 5, 7), want)
    _load(buf, h0, t)


def test_selection_at_size():
    """N = 65,589, ticks 9, n_steps 4, rows 4, S = 2: 1,180,602 ids, 1,153 tiles,
    every pass of the select with many workgroups; n = 65,536, once."""
    rng = np.random.RandomState(31)
    N, ticks, t = 65589, 9, 40
    h = _synthetic(N, ticks, 2, t, rng)
    kind = rng.randint(0, 100, size=h['loss'].shape)      # 3 % unscored, 10 % zero
    h['loss'] = np.where(kind < 3, np.float32(np.inf), np.where(kind < 13, np.float32(0),
                                                                _losses('scored', kind.shape, rng))).astype(np.float32)
    buf = replay.ReplayBuffer(N, 4, 2, ticks, n_steps=4, device=DEV)
    _load(buf, h, t)
    want = _host_ids(h, t, 65536, 41, 2)
    assert want.shape[0] == 65536
    cls, _ = replay.keys_host(h['loss'].ravel()[want], want, 41, 2)
    assert (cls == 0).sum() > 1000 and (cls == 1).sum() > 1000      # the threshold lies among the scored ones
    assert _same(_sample(buf, 65536, 41, 2), want)


def test_selection_is_deterministic(wide):
    buf, h0, t = wide
    h = dict(h0, loss=_losses('mixed', h0['loss'].shape, np.random.RandomState(2)))
    _load(buf, h, t)
    n = 5000
    a = _sample(buf, n, 3, 4)
    b = _sample(buf, n, 3, 4)
    assert a.shape[0] == n and _same(a, b)
    # a larger workspace, filled with 3e38, at another offset
    need = buf._workspace.numel()
    big = torch.full((need + 4096,), 3e38, dtype=torch.float32, device=DEV)
    out = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    c = buf._sample(n, 3, 4, out[:n], big[36:])
    torch.cuda.synchronize()
    assert _same(c.cpu().numpy(), a) and (out[n:] == SENTINEL).all()
    d = _sample(buf, n, 3, 5)
    assert d.shape[0] == n and not np.array_equal(a, d)
    _load(buf, h0, t)


# ---------------------------------------------------------------------------
# gather, update

def _gather_case(S, rows, rng):
    """A ring of 40 envs and 9 rows with synthetic states: live rows hold
    random values, padding rows column 0 = -1 and NaN elsewhere."""
    N, ticks = 40, 9
    nf = 5 + 5 * S
    buf = replay.ReplayBuffer(N, rows, S, ticks, n_steps=7, device=DEV)
    f = rng.uniform(-1.2, 1.2, size=(ticks, N, rows, nf)).astype(np.float32)
    live = rng.rand(ticks, N, rows) < 0.4
    live[:, :, rng.randint(0, rows)] = True                     # at least one live row, not always the first
    f[..., 0] = np.where(live, rng.randint(0, 2, size=live.shape), -1)
    f[~live, 1:] = np.nan
    h = replay.new_host(N, S, ticks)
    h['next'][:] = rng.randint(-1, ticks, size=(ticks, N))
    h['action'][:] = rng.randint(0, 6, size=h['action'].shape)
    h['reward'][:] = rng.uniform(-1, 1, size=h['reward'].shape)
    h['discount'][:] = rng.uniform(0.5, 1, size=h['discount'].shape)
    _load(buf, h, 20)
    buf.features.copy_(torch.from_numpy(f))
    return buf, h, f, live


def _guarded_f32(shape):
    n = int(np.prod(shape))
    flat = torch.full((n + GUARD,), float('nan'), dtype=torch.float32, device=DEV)
    flat[n:] = 12345.0
    return flat, flat[:n].view(shape)


@pytest.mark.parametrize('S', [2, 1])
@pytest.mark.parametrize('rows', [5, 36])
def test_gather(S, rows):
    rng = np.random.RandomState(rows + S)
    buf, h, f, live = _gather_case(S, rows, rng)
    N, nf = buf.n_env, buf.nf
    net = qnet.QNetwork.from_module(qt.weights_of('duo' if S == 2 else 'solo'), DEV)
    for n in (1, 33, 1000):
        ids = rng.randint(0, buf.ticks * N * S, size=n).astype(np.int32)
        if n > 1:
            assert set(ids % S) == set(range(S))
        fa, fo = _guarded_f32((n, rows, nf))
        na, no = _guarded_f32((n, rows, nf))
        ra, ro = _guarded_f32((n,))
        da, do = _guarded_f32((n,))
        a8 = torch.full((n + GUARD,), 99, dtype=torch.int8, device=DEV)
        t8 = torch.full((n + GUARD,), 99, dtype=torch.uint8, device=DEV)
        out = buf.gather(torch.from_numpy(ids).to(DEV), out=(fo, a8[:n], ro, do, no, t8[:n]))
        torch.cuda.synchronize()
        assert out[0].data_ptr() == fo.data_ptr() and out[4].data_ptr() == no.data_ptr()
        for g in (fa, na, ra, da):
            assert (g[-GUARD:] == 12345.0).all(), 'a guard element changed'
        assert (a8[n:] == 99).all() and (t8[n:] == 99).all()
        re, ship = ids // S, ids % S
        row, env = re // N, re % N
        nxt = h['next'][row, env]
        view = lambda x, s: qnet.swap_ego(x) if s == 1 else x  # noqa: E731
        got_f, got_n = fo.cpu().numpy(), no.cpu().numpy()
        assert _same(a8[:n].cpu().numpy(), h['action'].reshape(-1)[ids])
        assert _same(ro.cpu().numpy(), h['reward'].reshape(-1)[ids])
        assert _same(do.cpu().numpy(), h['discount'][row, env])
        assert _same(t8[:n].cpu().numpy(), (nxt == -1).astype(np.uint8))
        assert (nxt == -1).any() or n == 1
        for i in range(n):
            want, lv = view(f[row[i], env[i]], ship[i]), live[row[i], env[i]]
            assert _same(got_f[i, :, 0], want[:, 0]) and _same(got_f[i][lv], want[lv]), (n, i)
            if nxt[i] == -1:
                assert (got_n[i, :, 0] == -1).all()
            else:
                want, lv = view(f[nxt[i], env[i]], ship[i]), live[nxt[i], env[i]]
                assert _same(got_n[i, :, 0], want[:, 0]) and _same(got_n[i][lv], want[lv]), (n, i)
        # the ring's padding is NaN outside column 0: none of it reaches the network
        assert np.isnan(f[~live][:, 1:]).all()
        assert torch.isfinite(net.forward(fo)).all()
        keep = torch.from_numpy(nxt != -1).to(DEV)
        if bool(keep.any()):
            assert torch.isfinite(net.forward(no[keep].contiguous())).all()
        # and through td_targets: a terminal sample's target is its reward
        target = net.td_targets(ro, do, no, t8[:n])
        assert torch.isfinite(target).all() and torch.equal(target[~keep], ro[~keep])
    # fresh outputs
    f2 = buf.gather(torch.from_numpy(ids).to(DEV))
    assert torch.equal(f2[1], a8[:n]) and torch.equal(f2[5], t8[:n])


def test_update_loss(designed):
    buf, h0, t = designed[0], designed[1], 60
    _load(buf, h0, t)
    assert np.isinf(h0['loss']).all()
    ok = np.nonzero(replay.eligible_host(h0['next'], t, 2).ravel())[0]
    rng = np.random.RandomState(4)
    ids = np.sort(rng.choice(ok, size=300, replace=False)).astype(np.int32)
    vals = rng.exponential(1.0, size=300).astype(np.float32) + np.float32(0.01)
    buf.update_loss(torch.from_numpy(ids).to(DEV), torch.from_numpy(vals).to(DEV))
    want = h0['loss'].copy()
    want.reshape(-1)[ids] = vals
    assert _same(buf.loss.cpu().numpy(), want)
    # a second update keeps the old values elsewhere
    vals2 = vals[:50] * np.float32(2)
    buf.update_loss(torch.from_numpy(ids[:50]).to(DEV), torch.from_numpy(vals2).to(DEV))
    want.reshape(-1)[ids[:50]] = vals2
    assert _same(buf.loss.cpu().numpy(), want)
    # those ids have left class 0: with n = the unscored count the sample is exactly the unscored ones
    h = dict(h0, loss=want)
    got = _sample(buf, ok.size - 300, 9, 1)
    assert _same(got, np.setdiff1d(ok, ids).astype(np.int32))
    assert _same(_sample(buf, ok.size - 200, 9, 2), _host_ids(h, t, ok.size - 200, 9, 2))
    _load(buf, h0, t)


# ---------------------------------------------------------------------------
# the loop

def _training_run(check):
    cfg = gio.configs()['short']
    N, T, n_steps, ticks, batch = 512, 60, 7, 16, 256
    env = BatchedEnv(cfg, N, device=DEV, b_cap=32)
    env.reset()
    net = qnet.QNetwork.from_module(qt.weights_of('duo'), DEV)
    start = net.weights.clone()
    buf = replay.ReplayBuffer(N, env.p_pad + env.b_cap, 2, ticks, n_steps=n_steps, device=DEV)
    trained = 0
    for t in range(T):
        env.features(out=buf.head())
        control = env.qcontrols(net, epsilon=0.3, seed=17, tick0=t)
        _, reward, done = env.step(control)
        buf.push(control, reward, done)
        if buf.eligible_lower_bound() < batch:
            continue
        loss_before = buf.loss.cpu().numpy()
        ids = buf.sample(batch, seed=23, draw=t)
        assert ids.shape[0] == batch
        f, a, r, d, nf, term = buf.gather(ids)
        loss = net.sgd_step(f, a, net.td_targets(r, d, nf, term))
        buf.update_loss(ids, loss)
        trained += 1
        if check:
            want = replay.sample_host(loss_before, buf.next.cpu().numpy(), buf.t, batch, 23, t)
            assert _same(ids.cpu().numpy(), want), t
            assert torch.isfinite(loss).all() and torch.isfinite(net.weights).all()
            assert torch.equal(buf.loss.view(-1)[ids.long()], loss)
    env.check_errors()
    assert trained >= 40 and not torch.equal(net.weights, start)
    assert torch.isfinite(net.weights).all() and not torch.isinf(buf.loss).all()
    return net.weights.cpu().numpy()


def test_training_loop_is_reproducible():
    a = _training_run(True)
    b = _training_run(False)
    assert _same(a, b)
