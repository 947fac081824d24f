"""Forks on the device (astro_fork, include/astro_fork.h) and what is built on
them: ``BatchedEnv.fork_from`` / ``snapshot`` / ``restore``, the ``fork.Fork``
plan and the ``fork.Lookahead`` bot.

The yardstick is the step library itself: a forked env must hold its source's
bytes and then step like it, bit for bit, through auto-resets; what a fork does
not name must keep its bytes.  ``Lookahead.values`` is compared with the same
quantity obtained through ``to_host`` / ``load_host`` into plain envs, without
the fork library."""
import ctypes

import numpy as np
import pytest
import torch

from astro_amd import BatchedEnv, DEFAULT_CONFIG, SOLO_CONFIG, _lib, fork

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
N = 77                                                   # a ragged last wave, a ragged last group of four pairs
SHORT = DEFAULT_CONFIG._replace(max_time=3.0)            # 150 ticks at most: resets within every test's horizon
SOLO_SHORT = SOLO_CONFIG._replace(max_time=3.0)
ARRAYS = ('ships', 'ships_b', 'planets', 'bullets', 'hdr', 'stream', 'stream_ring')
SENTINEL = -12345.5
KEY_VALID, UNDRAWN = -(1 << 31), 1 << 30                 # hdr word 2 as int32


def make(cfg=SHORT, n=N, age=40, policy='random', **kw):
    """An env whose games have mixed ages: bullets are live and some games have ended."""
    kw.setdefault('b_cap', 32)
    env = BatchedEnv(cfg, n, device=DEV, auto_reset=True, **kw)
    env.reset()
    if age:
        env.rollout(age, policy, tick0=1 << 20)
    return env


def bits(a):
    """An array's bits as unsigned integers (floats are never compared as floats)."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def raw(env):
    """Every state array as it stands, env-major: {name: bits [n_env, ...]}."""
    torch.cuda.synchronize()
    out = {k: bits(getattr(env, k).cpu().numpy()) for k in ARRAYS}
    for k in ('ships', 'planets'):
        out[k] = out[k].transpose(1, 0, 2)
    out['ships_b'] = out['ships_b'].transpose(1, 0)
    return out


def nbullets(r):
    return (r['hdr'][:, 1] >> 16) & 0xffff


def live(r):
    """The live bullet rows as a mask [n_env, b_cap]."""
    return np.arange(r['bullets'].shape[1])[None, :] < nbullets(r)[:, None]


GAME = ('ships', 'ships_b', 'planets')


def assert_game(got, i, want, j, what):
    """Env i of `got` holds the current game of env j of `want`."""
    for k in GAME:
        assert np.array_equal(got[k][i], want[k][j]), (what, k)
    assert np.array_equal(got['hdr'][i, :2], want['hdr'][j, :2]), (what, 'hdr words 0-1')
    assert np.array_equal(got['stream'][i, 3], want['stream'][j, 3]), (what, 'game seed')
    nb = nbullets(want)[j]
    assert np.array_equal(got['bullets'][i, :nb], want['bullets'][j, :nb]), (what, 'live bullets')


def assert_future(got, i, want, j, what):
    assert np.array_equal(got['hdr'][i, 2:], want['hdr'][j, 2:]), (what, 'hdr words 2-3')
    assert np.array_equal(got['stream'][i, :3], want['stream'][j, :3]), (what, 'stream cursor')
    assert np.array_equal(got['stream_ring'][i], want['stream_ring'][j]), (what, 'ring')


def assert_same_batch(a, b, what):
    """Every env of two raw states: every array, bullets on live rows."""
    for k in ARRAYS:
        if k != 'bullets':
            assert np.array_equal(a[k], b[k]), (what, k)
    assert np.array_equal(live(a), live(b)) and np.array_equal(a['bullets'][live(a)], b['bullets'][live(b)]), what


def raw_fork(src, dst, src_ids, dst_ids, what, m=None):
    """astro_fork itself, past the Python layer's checks."""
    s = torch.tensor(src_ids, dtype=torch.int32, device=DEV)
    d = torch.tensor(dst_ids, dtype=torch.int32, device=DEV)
    rc = _lib.load_fork().astro_fork(ctypes.byref(src.params), ctypes.byref(src.state), ctypes.byref(dst.state),
                                     s.data_ptr(), d.data_ptr(), len(src_ids) if m is None else m, what,
                                     _lib.stream_ptr(dst.device))
    torch.cuda.synchronize()
    return rc


# ---------------------------------------------------------------------------
# 1. identity, everything: the bytes, then 200 ticks through auto-resets

@pytest.mark.parametrize('kernel', ['lane', 'quad', 'pair'])
@pytest.mark.parametrize('dtype,p_pad,cfg', [(torch.float32, 4, SHORT), (torch.float64, 4, SHORT),
                                             (torch.float32, 8, SHORT), (torch.float64, 8, SHORT),
                                             (torch.float32, 4, SOLO_SHORT)])
def test_identity_fork_then_equal_steps(kernel, dtype, p_pad, cfg):
    a = make(cfg, dtype=dtype, p_pad=p_pad)
    b = make(cfg, dtype=dtype, p_pad=p_pad, age=13, policy='script', kernel=kernel, env_offset=1000)
    assert b.step_kernel == kernel
    ra = raw(a)
    assert nbullets(ra).max() > 0 or cfg.solo
    assert not np.array_equal(ra['hdr'], raw(b)['hdr'])
    b.fork_from(a)
    assert_same_batch(raw(b), ra, 'after the fork')
    with pytest.raises(RuntimeError):
        b.info()
    ra_r, ra_d = a.rollout(200, 'script')
    rb_r, rb_d = b.rollout(200, 'script')
    done = ra_d.cpu().numpy()
    assert (done != 0).sum() >= N                     # every game ends within 150 ticks: the run contains resets
    assert np.array_equal(done, rb_d.cpu().numpy())
    assert np.array_equal(bits(ra_r.cpu().numpy()), bits(rb_r.cpu().numpy()))
    assert_same_batch(raw(b), raw(a), 'after 200 ticks')
    assert torch.equal(a.game_seed, b.game_seed) and not np.array_equal(raw(a)['stream'][:, 3], ra['stream'][:, 3])
    assert a.device_errors() == 0 and b.device_errors() == 0


# ---------------------------------------------------------------------------
# 2. indexed, inside one batch

def scramble_ring(env, seed):
    """Every word of every env's ring is its own (a young stream has written few of the 624: the rest are the
    zeros of its allocation, alike in every env).  For tests that do not step afterwards."""
    g = torch.Generator().manual_seed(seed)
    words = torch.randint(-2 ** 31, 2 ** 31 - 1, tuple(env.stream_ring.shape), generator=g, dtype=torch.int64)
    env.stream_ring.copy_(words.to(torch.int32))


def fill_dead_rows(env):
    """Every bullet row at or past its env's count holds the sentinel."""
    dead = torch.arange(env.b_cap, device=DEV)[None, :] >= env.nbullets[:, None]
    env.bullets[dead] = SENTINEL
    return dead.cpu().numpy()


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_indexed_fork_on_the_same_arrays(dtype):
    env = make(dtype=dtype, age=60)
    src, dst = [3, 3, 3, 70], [10, 11, 12, 0]
    fill_dead_rows(env)
    scramble_ring(env, 1)
    before = raw(env)
    nb = nbullets(before)
    assert nb[3] > 0 or nb[70] > 0
    env.fork_from(env, src, dst)
    after = raw(env)
    for s, d in zip(src, dst):
        assert_game(after, d, before, s, (s, d))
        assert_future(after, d, before, s, (s, d))
        # rows at or past the source's count: what the destination held (the sentinel where it was dead there)
        assert np.array_equal(after['bullets'][d, nb[s]:], before['bullets'][d, nb[s]:]), (s, d)
    others = np.setdiff1d(np.arange(N), dst)
    for k in ARRAYS:
        assert np.array_equal(after[k][others], before[k][others]), k
    sentinel = bits(np.array([SENTINEL], before_dtype(dtype)))[0]
    assert (before['bullets'][~live(before)] == sentinel).all()
    keeps = [d for s, d in zip(src, dst) if nb[d] <= nb[s]]      # dead before and after: still the sentinel
    assert all((after['bullets'][d, nb[s]:] == sentinel).all() for s, d in zip(src, dst) if d in keeps)


def before_dtype(dtype):
    return np.float64 if dtype == torch.float64 else np.float32


# ---------------------------------------------------------------------------
# 3. skipped pairs, m = 0

def test_out_of_range_ids_skip_their_pair_only():
    src, dst = make(), make(age=20, policy='script', env_offset=300, n=50)
    scramble_ring(src, 2)
    before = raw(dst)
    what = _lib.FORK_GAME | _lib.FORK_STREAM
    assert raw_fork(src, dst, [-1, 5, N, 6, 60, 76], [1, 50, 2, 7, -1, 49], what) == 0
    after, rs = raw(dst), raw(src)
    for s, d in ((6, 7), (76, 49)):
        assert_game(after, d, rs, s, (s, d))
        assert_future(after, d, rs, s, (s, d))
    others = np.setdiff1d(np.arange(50), [7, 49])
    for k in ARRAYS:
        assert np.array_equal(after[k][others], before[k][others]), k
    # m = 0 touches nothing, whatever the ids are
    assert raw_fork(src, dst, [1, 2], [3, 4], what, m=0) == 0
    again = raw(dst)
    for k in ARRAYS:
        assert np.array_equal(again[k], after[k]), k
    assert src.device_errors() == 0 and dst.device_errors() == 0


# ---------------------------------------------------------------------------
# 4. bullet counts

@pytest.mark.parametrize('dtype,b_cap,counts', [(torch.float32, 32, (0, 1, 32)), (torch.float64, 32, (0, 1, 32)),
                                                (torch.float32, 300, (0, 1, 257, 300)),
                                                (torch.float64, 300, (257, 300, 1, 0))])
def test_bullet_counts(dtype, b_cap, counts):
    a = make(age=0, dtype=dtype, b_cap=b_cap)
    b = make(age=0, dtype=dtype, b_cap=b_cap, env_offset=200)
    h = a.to_host()
    rng = np.random.RandomState(b_cap)
    nb = np.array([counts[i % len(counts)] for i in range(N)])
    flags = (nb == b_cap).astype(np.int64)                       # a full row: the overflow flag is set
    bullets = rng.uniform(-1, 1, size=(N, b_cap, 4)).astype(before_dtype(dtype))
    a.load_host(h['ships'], h['ships_b'], h['planets'], bullets, h['tick'] + 5, h['nplanets'], nb, flags)
    b.bullets.fill_(SENTINEL)
    b.fork_from(a)
    ra, rb = raw(a), raw(b)
    assert np.array_equal(nbullets(rb), nb) and np.array_equal((rb['hdr'][:, 1] >> 8) & 0xff, flags)
    assert np.array_equal(rb['hdr'], ra['hdr'])
    mask = live(ra)
    assert mask.sum() == nb.sum() and np.array_equal(rb['bullets'][mask], bits(bullets)[mask])
    sentinel = bits(np.array([SENTINEL], before_dtype(dtype)))[0]
    assert (rb['bullets'][~mask] == sentinel).all()              # no row past the count was written


# ---------------------------------------------------------------------------
# 5. GAME alone, STREAM alone

def seed_sequence(env, control):
    """Per env, the seeds of the games its auto-resets start while `control` [T, N, S] is stepped."""
    seqs = [[] for _ in range(env.n_env)]
    for t in range(control.shape[0]):
        _, _, done = env.step(control[t])
        d, s = done.cpu().numpy(), env.game_seed.cpu().numpy()
        for i in np.nonzero(d)[0]:
            seqs[i].append(int(s[i]))
    return seqs


@pytest.mark.parametrize('aged', [False, True])
def test_game_alone_keeps_the_destinations_future(aged):
    src = make(age=40)
    dst, twin = (make(age=25 if aged else 0, policy='script', env_offset=500) for _ in range(2))
    before, rs = raw(dst), raw(src)
    assert_same_batch(before, raw(twin), 'the twin')
    word2 = before['hdr'][:, 2].view(np.int32)
    if aged:
        assert (word2 & KEY_VALID != 0).all() and (word2 & UNDRAWN == 0).all()
    else:
        assert (word2 == UNDRAWN).all()
    dst.fork_from(src, game=True, stream=False)
    after = raw(dst)
    for i in range(N):
        assert_game(after, i, rs, i, i)
        assert_future(after, i, before, i, i)
    assert not np.array_equal(after['hdr'][:, 2:], rs['hdr'][:, 2:])
    # from its first reset on, the forked env plays the games its twin plays
    control = torch.from_numpy(np.random.RandomState(3).randint(0, 6, size=(320, N, 2)).astype(np.int8)).to(DEV)
    got, want = seed_sequence(dst, control), seed_sequence(twin, control)
    for i in range(N):
        n = min(len(got[i]), len(want[i]))
        assert n >= 2 and got[i][:n] == want[i][:n], i
    assert dst.device_errors() == 0 and twin.device_errors() == 0


def test_stream_alone_keeps_the_destinations_game():
    src = make(age=40)
    dst = make(age=25, policy='script', env_offset=500)
    fill_dead_rows(dst)
    scramble_ring(src, 3)
    before, rs = raw(dst), raw(src)
    dst.fork_from(src, game=False, stream=True)
    after = raw(dst)
    for i in range(N):
        assert_future(after, i, rs, i, i)
    for k in GAME + ('bullets',):
        assert np.array_equal(after[k], before[k]), k
    assert np.array_equal(after['hdr'][:, :2], before['hdr'][:, :2])
    assert np.array_equal(after['stream'][:, 3], before['stream'][:, 3])
    assert not np.array_equal(after['stream'][:, 3], rs['stream'][:, 3])


# ---------------------------------------------------------------------------
# 6. the pair-with-helpers instance

def test_filtered_streams_on_the_helper_instance():
    kw = dict(cfg=DEFAULT_CONFIG, n=512, p_pad=4, kernel='pair', planets_only=3)
    a, b = make(age=30, **kw), make(age=7, policy='script', env_offset=4096, **kw)
    assert b.launch_waves() == (16, 16)
    b.fork_from(a)
    assert_same_batch(raw(b), raw(a), 'after the fork')
    control = torch.from_numpy(np.random.RandomState(4).randint(0, 6, size=(60, 512, 2)).astype(np.int8)).to(DEV)
    for t in range(60):
        _, ra, da = a.step(control[t], stats=False)
        _, rb, db = b.step(control[t], stats=False)
        assert torch.equal(da, db) and torch.equal(ra, rb), t
    assert_same_batch(raw(b), raw(a), 'after 60 ticks')
    assert (raw(a)['hdr'][:, 1] & 0xff == 3).all()
    assert a.device_errors() == 0 and b.device_errors() == 0


# ---------------------------------------------------------------------------
# 7. snapshot / restore

@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_snapshot_and_restore(dtype):
    env = make(age=120, dtype=dtype)                 # close to the timeout: the 50 ticks contain resets
    start = raw(env)
    snap = env.snapshot()
    assert type(snap) is fork.Snapshot and not isinstance(snap, BatchedEnv)
    control = torch.from_numpy(np.random.RandomState(5).randint(0, 6, size=(50, N, 2)).astype(np.int8)).to(DEV)
    r1, d1 = env.rollout(50, control)
    end1 = raw(env)
    assert (d1 != 0).any() and not np.array_equal(end1['hdr'], start['hdr'])
    env.restore(snap)
    assert_same_batch(raw(env), start, 'restored')
    with pytest.raises(RuntimeError):
        env.info()
    r2, d2 = env.rollout(50, control)
    assert torch.equal(d1, d2) and np.array_equal(bits(r1.cpu().numpy()), bits(r2.cpu().numpy()))
    assert_same_batch(raw(env), end1, 'after the same 50 ticks')
    with pytest.raises(ValueError):
        make(age=0, n=5).restore(snap)


# ---------------------------------------------------------------------------
# 8. Lookahead

def doomed_envs(n, horizon):
    """An env of `n` games each of which ends within `horizon` ticks of script play with a non-zero reward
    (chosen from a larger batch, moved here by an indexed fork)."""
    big = make(DEFAULT_CONFIG, n=8192, age=150)
    snap = big.snapshot()
    reward, done = big.rollout(horizon - 2, 'script')
    ends = ((done != 0)[:, :, None] & (reward != 0)).any(2).any(0)
    ids = torch.nonzero(ends)[:, 0].cpu().numpy()
    assert ids.size >= n
    big.restore(snap)
    env = make(DEFAULT_CONFIG, n=n, age=0, env_offset=9000)
    env.fork_from(big, ids[:n], np.arange(n))
    return env


@pytest.mark.parametrize('ship', [0, 1])
def test_lookahead_values_equal_the_host_route(ship):
    horizon, discount = 12, 0.9
    env = doomed_envs(8, horizon)
    la = fork.Lookahead(env, ship=ship, horizon=horizon, discount=discount)
    before = raw(env)
    got = la.values()
    assert got.dtype == torch.float32 and tuple(got.shape) == (8, 6)
    assert_same_batch(raw(env), before, 'values() leaves the env alone')
    h = env.to_host()
    want = np.zeros((8, 6), np.float32)
    gamma = (discount ** np.arange(horizon)).astype(np.float32)
    for a in range(6):
        plain = make(DEFAULT_CONFIG, n=8, age=0, env_offset=100 * a)
        plain.load_host(**h)
        c = plain.controls('script')
        c[:, ship] = a
        _, r0, d0 = plain.step(c)
        r, d = plain.rollout(horizon - 1, 'script')
        reward = np.concatenate([r0.cpu().numpy()[None], r.cpu().numpy()])[:, :, ship]
        done = np.concatenate([d0.cpu().numpy()[None], d.cpu().numpy()]) != 0
        for i in range(8):
            t = np.nonzero(done[:, i])[0]
            if t.size:
                want[i, a] = gamma[t[0]] * reward[t[0], i]
    got = got.cpu().numpy()
    assert np.array_equal(bits(got), bits(want)), (got, want)
    assert (want != 0).sum() >= 8 and set(np.unique(np.abs(want))) <= set(gamma) | {0.0}
    # the decision: the base's own control unless another is strictly better, then the first maximal one
    own = env.controls('script')[:, ship].cpu().numpy()
    best = np.where(want.max(1) > want[np.arange(8), own], want.argmax(1), own)
    c = la.controls()
    assert c.dtype == torch.int8 and np.array_equal(c.cpu().numpy(), best)


def test_lookahead_with_nothing_in_sight_plays_its_base():
    env = make(DEFAULT_CONFIG, n=8, age=0)
    for horizon in (1, 3):
        la = fork.Lookahead(env, ship=0, horizon=horizon)
        assert (la.values() == 0).all()
        assert torch.equal(la.controls(), env.controls('script')[:, 0])
    solo = make(SOLO_SHORT, n=8, age=0)
    la = fork.Lookahead(solo, horizon=1)
    assert (la.values() == 0).all() and torch.equal(la.controls(), solo.controls('script')[:, 0])


def test_lookahead_play_equals_stepping_its_controls_by_hand():
    n, horizon = 16, 4
    env, twin = make(n=n, age=0), make(n=n, age=0)
    winner, length = fork.Lookahead(env, horizon=horizon).play('script', games=1)
    assert tuple(winner.shape) == tuple(length.shape) == (n, 1) and winner.dtype == length.dtype == torch.int64
    winner, length = winner.cpu().numpy()[:, 0], length.cpu().numpy()[:, 0]
    assert set(winner) <= {-1, 0, 1} and (length > 0).all() and (length <= 150).all()
    la = fork.Lookahead(twin, horizon=horizon)
    want_w, want_l = np.full(n, -2), np.zeros(n, np.int64)
    for t in range(150):
        c = twin.controls('script', tick0=t)
        c[:, 0] = la.controls()
        _, r, d = twin.step(c)
        r, d = r.cpu().numpy(), d.cpu().numpy()
        for i in np.nonzero((d != 0) & (want_w == -2))[0]:
            want_w[i] = r[i].argmax() if r[i].max() >= 1 else -1
            want_l[i] = t + 1
    assert np.array_equal(winner, want_w) and np.array_equal(length, want_l)
