"""The bullet-capacity axis: large b_cap, full rows, exact counters.  Needs an MI355X.

The step library reduces its per-wave counters two to a 32-bit wave sum while a wave's bullets stay
below 2^16 (lane kernel: b_cap <= 1023; quad and pair: b_cap * envs per wave < 65,536, that is
b_cap <= 4095 and <= 2047) and one by one above; the quad and pair kernels number a wave's live
bullets and walk them in LDS windows of 1,024; the header keeps an env's bullet count in 16 bits;
and the resident rollout keeps 32 bullet slots per env in LDS.  None of these limits is reached
by play -- bullets leave the arena -- so every state here is hand-loaded (tests/bullet_util.py, whose
scenarios tests/test_bullet_caps_host.py proves on the oracle alone) and every kernel is compared
with the oracle's trajectory from it, at every tick.

Bars as in tests/test_gpu_parity.py, no tolerance anywhere: float64 state bit-exact, float32 state
equal to the float32 rounding of the oracle's value computed from the same float32 input, integers
and every counter of stat_dict() exact (counter definitions: include/astro_step.h).
"""
import numpy as np
import pytest
import torch

from oracle import batched
from tests import bullet_util as bu
from tests.test_gpu_parity import KERNELS, _assert_same, _host_batch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
DTYPES = [pytest.param(torch.float64, id='f64'), pytest.param(torch.float32, id='f32')]
STORE = {torch.float32: 'f32', torch.float64: 'f64'}
STATE = ('ships', 'ships_b', 'planets', 'bullets', 'hdr')


def _env(name, n, b_cap, kernel, dtype=torch.float32, auto_reset=False):
    from astro_amd import BatchedEnv
    return BatchedEnv(bu.CFG[name], n, device=DEV, b_cap=b_cap, p_pad=bu.P_PAD, dtype=dtype,
                      auto_reset=auto_reset, kernel=kernel)


def _loaded(sc, kernel, dtype=torch.float32, b_cap=None):
    env = _env(sc.name, sc.n, b_cap or sc.b_cap, kernel, dtype)
    B = sc.start
    env.load_host(B.ships, B.ships_b, B.planets, B.bullets, B.tick, B.nplanets, B.nbullets)
    return env


def _ctl(sc):
    return torch.from_numpy(sc.ctl).to(DEV)


def _check_tick(tag, env, t, rew, done, rounding, alive=None):
    """One tick's reward and done, and the state, overflow flags included, of the envs that go on."""
    done = done.cpu().numpy()
    seen = np.ones(done.shape, bool) if alive is None else alive   # (alive: the envs no earlier tick ended)
    assert np.array_equal(done[seen], t.done[seen]), tag
    assert np.array_equal(rew.cpu().numpy()[seen], t.reward[seen]), tag
    run = seen & (t.done == 0)
    got = _host_batch(env)
    _assert_same(tag, got, t.out, run, rounding)
    assert np.array_equal(got.nplanets, t.out.nplanets), tag
    assert np.array_equal(got.overflow[run], t.out.overflow[run]), tag
    assert np.array_equal(env.info()['overflow'].cpu().numpy()[run], t.out.overflow[run]), tag
    return got


def _follow(tag, env, sc, stats=True):
    """Step the scenario's ticks: every tick equal to the oracle's, the counters too."""
    ctl = _ctl(sc)
    rounding = env.dtype == torch.float32
    for k, t in enumerate(sc.ticks):
        _, rew, done = env.step(ctl[k], auto_reset=False, stats=stats)
        _check_tick('%s t=%d' % (tag, k), env, t, rew, done, rounding)
        if stats:
            got, want = env.stat_dict(), bu.totals(sc.ticks[:k + 1])
            print(tag, k, got)
            assert got == want, (tag, k)
    return env


def _same_arrays(a, b, fields=STATE):
    for f in fields:
        assert torch.equal(getattr(a, f), getattr(b, f)), f


# --------------------------------------------------------- a. packing thresholds

@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('b_cap', bu.THRESHOLDS)
def test_packing_thresholds(b_cap, dtype, kernel):
    """64 full envs (bu.thresholds): each wave's bullet counts sum to the most the packed counters
    hold (b_cap 1023 lane, 4095 quad, 2047 pair) or to 65,536, which only the unpacked reduction
    holds; a firing tick drops S shots per full env.  State and all counters equal the oracle's at
    every tick, the overflow flags are set, and the counter-free instance computes the same state
    and leaves the stats rows zero."""
    sc = bu.thresholds(b_cap, STORE[dtype])
    env = _follow('thresholds %d %s' % (b_cap, kernel), _loaded(sc, kernel, dtype), sc)
    assert env.stat_dict()['overflows'] == 2 * bu.N_FULL
    assert env.info()['overflow'].cpu().numpy()[:bu.N_FULL].all()
    plain = _follow('plain', _loaded(sc, kernel, dtype), sc, stats=False)
    assert not any(plain.stat_dict().values())
    _same_arrays(env, plain)


@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('b_cap', [1024, 4096])
def test_packing_thresholds_from_tick0(b_cap, kernel):
    """The same from fresh games (tick 0: bullets moved and shots made in float32), a shot at
    every tick."""
    sc = bu.thresholds(b_cap, 'f32', True)
    env = _follow('thresholds tick0 %d %s' % (b_cap, kernel), _loaded(sc, kernel), sc)
    assert env.stat_dict()['overflows'] == 2 * bu.N_FULL * len(sc.ticks)


@pytest.mark.parametrize('b_cap', bu.THRESHOLDS)
def test_kernels_agree_on_counters(b_cap):
    """lane, quad and pair on the same full waves: the same counters, headers and live bullets."""
    sc = bu.thresholds(b_cap, 'f32')
    ctl = _ctl(sc)
    envs = [_loaded(sc, k) for k in KERNELS]
    for e in envs:
        for k in range(len(sc.ticks)):
            e.step(ctl[k], auto_reset=False)
    lane = envs[0]
    for e in envs[1:]:
        assert e.stat_dict() == lane.stat_dict()
        _same_arrays(e, lane, ('ships', 'ships_b', 'planets', 'hdr'))
        _assert_same('kernels', _host_batch(e), _host_batch(lane), np.ones(sc.n, bool), False)
    assert lane.stat_dict() == bu.totals(sc.ticks)


# ------------------------------------------------------------ b. window geometry

def _geometry(pattern, tick0, kernel, dtype):
    sc = bu.geometry(pattern, store=STORE[dtype], tick0=tick0)
    other = bu.geometry(pattern, b_cap=bu.GEOM_BCAP + 60, store=STORE[dtype], tick0=tick0)
    a, b = _loaded(sc, kernel, dtype), _loaded(other, kernel, dtype)
    ctl = _ctl(sc)
    same = np.ones(sc.n, bool)
    rounding = dtype == torch.float32
    for k, (ta, tb) in enumerate(zip(sc.ticks, other.ticks)):
        tag = 'geometry %s %s t=%d' % (pattern, kernel, k)
        _, rew, done = a.step(ctl[k], auto_reset=False)
        ga = _check_tick(tag, a, ta, rew, done, rounding)
        _, rew, done = b.step(ctl[k], auto_reset=False)
        gb = _check_tick(tag + ' stride', b, tb, rew, done, rounding)
        # another row stride, the same live bullets (until an env drops a shot at 4,100 slots)
        same &= ta.counts['overflows'] == 0
        gb.bullets = gb.bullets[:, :bu.GEOM_BCAP]
        _assert_same(tag + ' strides', ga, gb, same, False)
        assert a.stat_dict() == bu.totals(sc.ticks[:k + 1]), tag
        assert b.stat_dict() == bu.totals(other.ticks[:k + 1]), tag


@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('tick0', [False, True], ids=['late', 'tick0'])
@pytest.mark.parametrize('pattern', bu.PATTERNS)
def test_window_geometry(pattern, tick0, kernel):
    """b_cap 4,100 with envs that start and end exactly on a window boundary, cover whole windows,
    are empty between large ones and first and last in the wave, or leave lanes of their group idle
    (bu.GEOM_NB), under each kill pattern: the compaction keeps slot order (the live bullets equal
    the oracle's, slot by slot) at this row stride and at b_cap 4,160."""
    _geometry(pattern, tick0, kernel, torch.float32)


@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('pattern', ['window_edges', 'random30'])
def test_window_geometry_float64(pattern, kernel):
    _geometry(pattern, False, kernel, torch.float64)


# ------------------------------------------------------------- c. the 16-bit ends

@pytest.mark.parametrize('kernel', KERNELS)
def test_sixteen_bit_ends(kernel):
    """b_cap 65,535 and counts (65535, 0, 65534, 1, 32768): the header's 16-bit bullet count and
    the index word's 16-bit slot at their ends, across a firing tick that drops 2 and 1 shots."""
    sc = bu.ends()
    env = _follow('ends %s' % kernel, _loaded(sc, kernel), sc)
    assert env.nbullets.cpu().tolist() == [65535, 2, 65535, 3, 32770]
    assert env.to_host()['nbullets'].tolist() == [65535, 2, 65535, 3, 32770]
    assert env.stat_dict()['overflows'] == 3
    assert env.info()['overflow'].cpu().tolist() == [True, False, True, False, False]


# ---------------------------------------------------------- d. a loaded game ends

@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_loaded_game_ends(dtype, kernel):
    """Envs of more than 2,048 bullets take a ship hit from a bullet in the first, a middle or the
    last index window (bu.HIT_AT), no auto-reset: reward, done, info()['hit'] and the counters equal
    the oracle's, and a finished env keeps what the oracle keeps -- header, ships and planets; its
    bullet rows are compacted in place before the hit is known and are not defined (astro_step.h).
    The other envs go on equal to the oracle."""
    sc = bu.hits(STORE[dtype])
    env = _loaded(sc, kernel, dtype)
    ctl = _ctl(sc)
    rounding = dtype == torch.float32
    alive = np.ones(sc.n, bool)
    for k, t in enumerate(sc.ticks):
        _, rew, done = env.step(ctl[k], auto_reset=False)
        got = _check_tick('hits %s t=%d' % (kernel, k), env, t, rew, done, rounding, alive)
        if k == 0:
            fin = t.done != 0
            assert fin.sum() == len(bu.HIT_AT)
            want_hit = ((t.reward < 0) & fin[:, None]).astype(np.uint8) @ np.array([1, 2], np.uint8)
            assert np.array_equal(env.info()['hit'].cpu().numpy(), want_hit) and set(want_hit.tolist()) == {0, 1, 2, 3}
            assert env.stat_dict() == bu.totals(sc.ticks[:1])
            for f in ('tick', 'nplanets', 'nbullets', 'ships', 'ships_b', 'planets'):
                assert np.array_equal(getattr(got, f)[fin], getattr(sc.start, f)[fin]), f
        alive &= t.done == 0
    assert alive.sum() == sc.n - len(bu.HIT_AT)


def _part(env, sl, cols):
    """_host_batch of the envs ``sl`` with their first ``cols`` bullet slots only."""
    f64 = lambda t: t.cpu().numpy().astype(np.float64)   # noqa: E731
    return batched.Batch(env.tick[sl].cpu().numpy().astype(np.int32), env.nplanets[sl].cpu().numpy().astype(np.int32),
                         env.nbullets[sl].cpu().numpy().astype(np.int32), f64(env.ships[:, sl].permute(1, 0, 2)),
                         f64(env.ships_b[:, sl].permute(1, 0)), f64(env.planets[:, sl].permute(1, 0, 2)),
                         f64(env.bullets[sl, :cols]), (env.flags[sl].cpu().numpy() & 1).astype(bool))


def _load_front(env, B):
    """Overwrite the first envs with B (as load_host does for a whole batch; seed streams kept)."""
    from astro_amd.env import TICK_MASK
    k = B.tick.shape[0]
    put = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=env.dtype)   # noqa: E731
    env.ships[:, :k] = put(B.ships.transpose(1, 0, 2))
    env.ships_b[:, :k] = put(B.ships_b.transpose(1, 0))
    env.planets[:, :k] = put(B.planets.transpose(1, 0, 2))
    env.bullets[:k] = put(B.bullets)
    hdr = env.hdr[:k].cpu().numpy().view(np.uint32).astype(np.int64)
    hdr[:, 0] = (hdr[:, 0] & ~TICK_MASK & 0xFFFFFFFF) | B.tick
    hdr[:, 1] = B.nplanets.astype(np.int64) | (B.nbullets.astype(np.int64) << 16)
    env.hdr[:k] = torch.as_tensor(hdr.astype(np.uint32).view(np.int32)).to(DEV)


FILL_COLS = 16    # bullet slots of the freshly reset envs the oracle steps (they hold a few shots at most)
RESTART = [pytest.param(k, False, id=k + '-helpers') for k in KERNELS]
RESTART += [pytest.param('quad', True, id='quad-large'), pytest.param('pair', True, id='pair-large')]


@pytest.mark.parametrize('kernel,large', RESTART)
def test_loaded_game_restarts(kernel, large):
    """The same designed envs in front of a freshly reset batch, auto-reset on: the env a loaded
    bullet ends becomes batched.create of its stream's next seed with no bullets, and the next ticks
    equal the oracle -- in a launch with helper waves (at most 2,048 step waves) and in one too
    large for them, which creates the games in its step waves."""
    name, store, ticks = 'default', 'f32', 2 if large else 3
    n = {'quad': 32800, 'pair': 65600}[kernel] if large else 77
    P = bu.params(name)
    k = len(bu.HIT_NB)
    bs = bu.base(name, k, store, False, 3)
    front, _ = bu.load_hits(bs)
    env = _env(name, n, bu.HIT_BCAP, kernel, auto_reset=True)
    if kernel != 'lane':
        assert (env.launch_waves()[1] > 0) != large
    env.reset()
    _load_front(env, front)
    seeds = batched.game_seeds(env.stream_seeds, 8)
    games = np.ones(n, np.int64)
    parts = [(slice(0, k), bu.HIT_BCAP), (slice(k, n), FILL_COLS)]
    ctl = np.random.RandomState(8).randint(0, 6, size=(ticks, n, 2)).astype(np.int8)
    ctl[:, :k] = bs.ctl[:ticks]
    want = dict.fromkeys(bu.COUNTERS + ('resets',), 0)
    for t in range(ticks):
        ins = [_part(env, sl, cols) for sl, cols in parts]
        _, rew, done = env.step(torch.from_numpy(ctl[t]).to(DEV))
        rew, done = rew.cpu().numpy(), done.cpu().numpy()
        for (sl, cols), B in zip(parts, ins):
            g = games[sl]
            tk = bu.run(B, ctl[t:t + 1, sl], P, store, seeds=seeds[sl], games=g)[0]
            games[sl] = g
            tag = 'restart %s t=%d envs %d..' % (kernel, t, sl.start)
            assert np.array_equal(done[sl], tk.done) and np.array_equal(rew[sl], tk.reward), tag
            got = _part(env, sl, cols)
            _assert_same(tag, got, tk.out, np.ones(tk.done.size, bool), True)
            assert np.array_equal(got.overflow, tk.out.overflow), tag
            for c in want:
                want[c] += int(tk.counts[c].sum())
            if t == 0 and sl.start == 0:
                fin = np.nonzero(tk.done)[0]
                assert fin.tolist() == sorted(bu.HIT_AT)
                assert (got.nbullets[fin] == 0).all() and (got.tick[fin] == 0).all()
        assert (env.game_seed.cpu().numpy().view(np.uint32) == seeds[np.arange(n), games - 1]).all(), t
    st = env.stat_dict()
    # (serial_resets is no oracle count: the quad and pair kernels create a game that ends at its
    # first step -- its next seed not drawn yet -- on their serial path)
    serial = st.pop('serial_resets')
    assert st == want and st['resets'] >= len(bu.HIT_AT) and serial <= st['resets']


# ------------------------------------------------------------ e. multi-tick paths

MULTI = [pytest.param('quad', 4096, id='quad-4096'), pytest.param('pair', 2048, id='pair-2048'),
         pytest.param('lane', 1024, id='lane-1024')]


def _stepped(sc, kernel, ctl):
    env = _loaded(sc, kernel)
    out = [[x.clone() for x in env.step(ctl[k], auto_reset=False)[1:]] for k in range(ctl.shape[0])]
    return env, out


@pytest.mark.parametrize('kernel,b_cap', MULTI)
def test_step_many_at_the_unpacked_threshold(kernel, b_cap):
    """step_many(k) from full waves that sum to 65,536 == k step calls bit for bit, the summed
    counters too (and both equal the oracle's)."""
    sc = bu.thresholds(b_cap, 'f32')
    ctl = _ctl(sc)
    b, steps = _stepped(sc, kernel, ctl)
    a = _loaded(sc, kernel)
    rew, done = a.step_many(ctl, auto_reset=False)
    for k, (r, d) in enumerate(steps):
        assert torch.equal(rew[k], r) and torch.equal(done[k], d), k
    _same_arrays(a, b)
    assert a.stat_dict() == b.stat_dict() == bu.totals(sc.ticks)


@pytest.mark.parametrize('policy', ['control', 'random'])
@pytest.mark.parametrize('kernel,b_cap', MULTI)
def test_rollout_at_the_unpacked_threshold(kernel, b_cap, policy):
    """rollout(K) -- the quad and pair kernels' K-tick instance, whose counters are flushed every
    tick by the same packing rule -- from the same state, on a control array (the scenario's: also
    the oracle's totals) and on the device's random policy (bench.controls on the host)."""
    import bench
    sc = bu.thresholds(b_cap, 'f32')
    K = len(sc.ticks)
    ctl = _ctl(sc) if policy == 'control' else torch.from_numpy(bench.controls(0, sc.n, 2, 9 + K)[9:]).to(DEV)
    b, steps = _stepped(sc, kernel, ctl)
    a = _loaded(sc, kernel)
    rew, done = a.rollout(K, ctl if policy == 'control' else 'random', seed=0, tick0=9, auto_reset=False)
    for k, (r, d) in enumerate(steps):
        assert torch.equal(rew[k], r) and torch.equal(done[k], d), k
    _same_arrays(a, b)
    assert a.stat_dict() == b.stat_dict()
    assert a.stat_dict()['bullets_in'] >= K * bu.N_FULL * b_cap
    if policy == 'control':
        assert a.stat_dict() == bu.totals(sc.ticks)


# ----------------------------------------------------------- f. resident boundary

@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('b_cap', [32, 33])
def test_resident_boundary(b_cap, kernel):
    """float32, every env full: at b_cap 32 the resident rollout (32 bullet slots per env in LDS,
    index windows of 256: a quad wave's 512 bullets are 2 windows, a pair wave's 1,024 are 4) across
    a firing tick == stepping on every array and counter; at 33 the library must run the
    global-memory instance (rows of 33 do not fit the LDS rows).  Both equal the oracle."""
    sc = bu.resident(b_cap)
    K = len(sc.ticks)
    ctl = _ctl(sc)
    b, steps = _stepped(sc, kernel, ctl)
    a = _loaded(sc, kernel)
    rew, done = a.rollout(K, ctl, auto_reset=False)
    for k, (r, d) in enumerate(steps):
        assert torch.equal(rew[k], r) and torch.equal(done[k], d), k
        assert np.array_equal(rew[k].cpu().numpy(), sc.ticks[k].reward) and not done[k].any()
    _same_arrays(a, b)
    assert a.stat_dict() == b.stat_dict() == bu.totals(sc.ticks)
    for e in (a, b):
        got = _host_batch(e)
        _assert_same('resident %d %s' % (b_cap, kernel), got, sc.ticks[-1].out, np.ones(sc.n, bool), True)
        assert got.overflow.all()
    assert a.stat_dict()['overflows'] == 2 * sc.n
