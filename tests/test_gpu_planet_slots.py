"""Every planet-slot count: p_pad 1..16, the 16-slot kernel instances, and
p_pad below the instance's register capacity.  Needs an MI355X.

The step library builds its kernels for 4, 8 or 16 planet registers
(dispatch in csrc/astro_kernels.hip) while the state's ``planets`` array has
p_pad slots: with p_pad 1-3, 5-7 or 9-15 every load and store of a planet
slot has to stay inside the shorter array, and with 9-16 slots the 16-register
instances run (lane kernel only).  Every env of this module keeps its planets
inside a larger allocation, 64 guard elements before and 64 after, filled
with a NaN of a fixed bit pattern:

  * a store outside the array changes a guard element: ``assert_guard_intact``
    after the launches;
  * a load outside it that is used reads NaN, and the bit-exact comparisons
    against the CPU oracle (oracle.batched, oracle.features: pinned to the
    reference up to 16 planets by tests/test_wide_host.py) and against
    tests/golden/wide.npz fail.

Bars as in tests/test_gpu_parity.py: float64 state bit-exact, float32 state
equal to the float32 rounding of the reference value computed from the same
float32 input state; integer fields exact.
"""
import functools

import numpy as np
import pytest
import torch

from astro_amd.config import DEFAULT_CONFIG
from oracle import batched, features
from tests import golden_io as gio
from tests import qnet_util as qu
from tests.test_gpu_bots import _dtype_rule_holds
from tests.test_gpu_parity import _assert_same, _auto_reset_vs_oracle, _host_batch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
F32, F64 = np.float32, np.float64
DTYPES = [pytest.param(torch.float64, id='f64'), pytest.param(torch.float32, id='f32')]
N, TICKS, B_CAP = 200, 40, 16
# The stepped runs' games: max_time of LIFE ticks, so that every env re-creates within TICKS (a
# one-planet game hardly ends otherwise); a shot every 5 ticks and ships of 0.08, so that games of two and
# more planets also end by collisions, at different ages, and bullets are in flight (never more than B_CAP)
LIFE = 25
LIVELY = dict(reload_time=0.1, ship_radius=0.08)

# ---------------------------------------------------------------------------
# the guard

GUARD = 64
GUARD_BITS = {torch.float32: (torch.int32, 0x7FC5A5A5), torch.float64: (torch.int64, 0x7FF85A5A5A5A5A5A)}


def guarded(t):
    """A copy of tensor ``t`` inside a larger allocation: GUARD elements of a
    fixed-pattern NaN before it and GUARD after it.  Returns (copy, whole
    allocation); the copy starts 32-byte aligned."""
    it, bits = GUARD_BITS[t.dtype]
    big = torch.empty(GUARD + t.numel() + GUARD, dtype=t.dtype, device=t.device)
    big.view(it).fill_(bits)
    view = big[GUARD:GUARD + t.numel()].view(t.shape)
    assert view.data_ptr() % 32 == 0 and torch.isnan(big).all()
    view.copy_(t)
    return view, big


def guard_untouched(view, big, where=''):
    """No guard element of ``guarded``'s allocation changed, read through an integer view."""
    it, bits = GUARD_BITS[big.dtype]
    g = big.view(it)
    assert view.data_ptr() == big.data_ptr() + GUARD * big.element_size()
    for side, part in (('before', g[:GUARD]), ('after', g[GUARD + view.numel():])):
        assert part.numel() == GUARD
        bad = torch.nonzero(part != bits).flatten().tolist()
        assert not bad, 'guard elements %s %s the array were overwritten (%s)' % (bad[:8], side, where)


def guard_planets(env):
    """Swap the env's planets for a guarded copy and point env.state.planets at it."""
    view, big = guarded(env.planets)
    env.planets = view
    env.state.planets = view.data_ptr()
    env.planet_guard = big
    return env


def assert_guard_intact(env, where=''):
    assert env.state.planets == env.planets.data_ptr(), 'the launches did not use the guarded planets'
    guard_untouched(env.planets, env.planet_guard, where)


# ---------------------------------------------------------------------------
# the slot-count matrix

def _config(max_planets, solo=False, life=None):
    cfg = DEFAULT_CONFIG._replace(max_planets=max_planets, solo=solo)
    return cfg if life is None else cfg._replace(max_time=cfg.dt * life, **LIVELY)


def _matrix():
    """(max_planets, p_pad, kernel, solo): every p_pad 1..16 full, slack slots
    below each register capacity, lane everywhere and quad and pair up to 8
    slots; one-ship games at 16, 12 and 7 slots (lane) and 3 (all kernels)."""
    slots = [(p, p, False) for p in range(1, 17)] + [(3, 4, False), (3, 5, False), (6, 7, False), (11, 16, False)]
    slots += [(16, 16, True), (9, 12, True), (6, 7, True), (3, 3, True)]
    out = []
    for mp, p_pad, solo in slots:
        for kernel in ('lane', 'quad', 'pair'):
            if kernel == 'lane' or (p_pad <= 8 and not (solo and p_pad > 3)):
                out.append(pytest.param(mp, p_pad, kernel, solo,
                                        id='mp%d-pad%d-%s%s' % (mp, p_pad, kernel, '-solo' if solo else '')))
    return out


MATRIX = _matrix()


def _env(cfg, n, p_pad, dtype, kernel='auto', auto_reset=True, b_cap=B_CAP):
    from astro_amd import BatchedEnv
    env = BatchedEnv(cfg, n, device=DEV, b_cap=b_cap, p_pad=p_pad, dtype=dtype, auto_reset=auto_reset, kernel=kernel)
    assert env.p_pad == p_pad and env.planets.shape == (p_pad, n, 4)
    return guard_planets(env)


def _rnd(dtype):
    return (lambda a: a.astype(F32).astype(F64)) if dtype == torch.float32 else (lambda a: a)


@functools.lru_cache(maxsize=None)
def _created(max_planets, solo):
    """(seeds [N, 2], create() of every one of them at 16 slots in float64, N * 2 games): the stream's
    first game and an explicit seed per env, shared by the cases of a config and never written to."""
    cfg = _config(max_planets, solo)
    seeds = batched.game_seeds(batched.stream_seeds(cfg.seed, N), 2)
    want = batched.create(seeds.reshape(-1), batched.make_params(cfg), p_pad=16, b_cap=1, store='f64')
    for f in want.__dataclass_fields__:
        getattr(want, f).setflags(write=False)
    seeds.setflags(write=False)
    return seeds, want


def _check_created(env, want, k, seeds, where):
    """tests/test_gpu_reset_create.py::_check_fresh's rule on every env: env i holds game k[i] of ``want``."""
    h = env.to_host()
    rnd = _rnd(env.dtype)
    assert np.array_equal(env.game_seed.cpu().numpy().view(np.uint32), seeds), where
    assert np.array_equal(h['nplanets'], want.nplanets[k]), where
    assert not h['tick'].any() and not h['nbullets'].any() and not h['flags'].any(), where
    assert np.array_equal(h['ships'].astype(F64), rnd(want.ships[k])), where
    assert np.array_equal(h['ships_b'].astype(F64), rnd(want.ships_b[k])), where
    live = np.arange(env.p_pad)[None, :] < want.nplanets[k][:, None]
    assert np.array_equal(h['planets'].astype(F64)[live], rnd(want.planets[k][:, :env.p_pad])[live]), where


# ------------------------------------------------------------------ (a) create

@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('max_planets,p_pad,kernel,solo', MATRIX)
def test_create(max_planets, p_pad, kernel, solo, dtype):
    """reset() from the stream and reset(seeds=...) == the oracle's create() on
    every field, with every planet count 1..max_planets among the games."""
    seeds, want = _created(max_planets, solo)
    env = _env(_config(max_planets, solo), N, p_pad, dtype, kernel)
    assert np.array_equal(env.stream_seeds, batched.stream_seeds(env.config.seed, N))
    i = np.arange(N)
    env.reset()
    _check_created(env, want, 2 * i, seeds[:, 0], 'reset()')
    env.reset(seeds=seeds[:, 1].copy())
    _check_created(env, want, 2 * i + 1, seeds[:, 1], 'reset(seeds)')
    for k in (0, 1):
        assert set(want.nplanets[k::2].tolist()) == set(range(1, max_planets + 1))
    assert_guard_intact(env, 'reset')


WIDE = [('mp11', 11), ('mp11', 16), ('mp16', 16), ('mp16_solo', 16)]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name,p_pad', WIDE)
def test_create_matches_wide_fixture(name, p_pad, dtype):
    """create() of the fixture's seeds (every planet count 1..max, rejected
    randint words at 11) == the reference's own arrays."""
    z = gio.load('wide.npz')
    cfg = gio.wide_configs()[name]
    seeds = z[name + '__seed']
    env = _env(cfg, seeds.size, p_pad, dtype)
    env.reset(seeds=seeds)
    h = env.to_host()
    S = env.S
    npl = z[name + '__nplanets']
    assert set(npl.tolist()) == set(range(1, cfg.max_planets + 1))
    assert (h['nplanets'] == npl).all() and (h['tick'] == 0).all() and (h['nbullets'] == 0).all()
    assert np.array_equal(h['ships'][..., 0:2].astype(F32), z[name + '__ships_x'][:, :S])
    assert not h['ships'][..., 2:4].any()
    assert np.array_equal(h['ships_b'].astype(F32), z[name + '__ships_b'][:, :S])
    pv = np.arange(p_pad)[None, :] < npl[:, None]
    assert np.array_equal(h['planets'][..., 0:2][pv].astype(F32), z[name + '__planets_x'][:, :p_pad][pv])
    want_dx = z[name + '__planets_dx'][:, :p_pad][pv]
    if dtype == torch.float32:
        want_dx = want_dx.astype(F32)
    assert np.array_equal(h['planets'][..., 2:4][pv], want_dx)
    assert (env.game_seed.cpu().numpy().view(np.uint32) == seeds).all()
    assert_guard_intact(env, 'reset(seeds)')


# ------------------------------------------- (b) step with auto-reset vs oracle

def _stepped_vs_oracle(max_planets, p_pad, kernel, solo, dtype, stats):
    cfg = _config(max_planets, solo, LIFE)
    rec = {}
    _auto_reset_vs_oracle(cfg, 'mp%d/pad%d' % (max_planets, p_pad), N, TICKS, B_CAP, kernel, stats, p_pad=p_pad,
                          dtype=dtype, prepare=guard_planets, record=rec)
    env, games = rec['env'], rec['games']
    assert env.p_pad == p_pad and env.step_kernel == kernel
    assert_guard_intact(env, 'reset and %d steps' % TICKS)
    assert rec['counts_seen'] == set(range(1, max_planets + 1))
    assert (games > 1).all(), 'an env never re-created'
    seeds = batched.game_seeds(env.stream_seeds, 64)
    assert np.array_equal(env.game_seed.cpu().numpy().view(np.uint32), seeds[np.arange(N), games - 1])
    if stats:
        st = rec['stats']
        assert st['resets'] == int((games - 1).sum()) > 0
        assert st['planets'] == rec['planets_read'] and st['collisions'] == rec['collisions']
        assert st['collisions'] > 0 or max_planets < 3   # (ships of a one- or two-planet game start far apart)


@pytest.mark.parametrize('stats', [False, True], ids=['plain', 'stats'])
@pytest.mark.parametrize('max_planets,p_pad,kernel,solo', MATRIX)
def test_step_auto_reset_vs_oracle(max_planets, p_pad, kernel, solo, stats):
    """tests/test_gpu_parity.py's auto-reset loop at every slot count, float32
    state: each tick equals the oracle stepped from the kernel's own input
    state, each finished game's successor the oracle's create()."""
    _stepped_vs_oracle(max_planets, p_pad, kernel, solo, torch.float32, stats)


F64_STEP = [p for p in MATRIX if p.values[1] in (3, 7, 11, 16)]


@pytest.mark.parametrize('max_planets,p_pad,kernel,solo', F64_STEP)
def test_step_auto_reset_vs_oracle_float64(max_planets, p_pad, kernel, solo):
    _stepped_vs_oracle(max_planets, p_pad, kernel, solo, torch.float64, True)


# ------------------------------------- (c) teacher-forced transitions of wide.npz

@functools.lru_cache(maxsize=None)
def _wide():
    return gio.Transitions('wide.npz')


def _wide_group(name, p_pad):
    """(row indices, b_cap, input Batch at p_pad slots) of a config's transitions."""
    tr = _wide()
    idx = dict(tr.groups())[name]
    assert int(tr.z['nplanets'][idx].max()) == gio.wide_configs()[name].max_planets <= p_pad
    b_cap = tr.max_bullets(idx) + 2
    S = 1 if gio.wide_configs()[name].solo else 2
    return idx, b_cap, tr.batch_in(idx, S, p_pad=p_pad, b_cap=b_cap)


def _loaded(name, p_pad, dtype, kernel='auto'):
    idx, b_cap, B = _wide_group(name, p_pad)
    env = _env(gio.wide_configs()[name], idx.size, p_pad, dtype, kernel, auto_reset=False, b_cap=b_cap)
    env.load_host(B.ships, B.ships_b, B.planets, B.bullets, B.tick, B.nplanets, B.nbullets)
    return env, idx, b_cap


@pytest.mark.parametrize('stats', [False, True], ids=['plain', 'stats'])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name,p_pad', WIDE)
def test_step_teacher_forced_vs_wide_fixture(name, p_pad, dtype, stats):
    """One step from every input state of wide.npz (9-16 planets among them,
    tick 0, bullets, planet collisions) == the reference's own output."""
    tr = _wide()
    env, idx, b_cap = _loaded(name, p_pad, dtype)
    assert env.step_kernel == 'lane'
    S = env.S
    ctl = tr.z['control'][idx, :S].astype(np.int8)
    _, rew, done = env.step(torch.from_numpy(ctl).cuda(), auto_reset=False, stats=stats)
    E, erew, edone = tr.expected(idx, S, p_pad=p_pad, b_cap=b_cap)
    done = done.cpu().numpy()
    assert (done == edone).all() and (done == 1).any() and (done == 0).any()
    assert np.array_equal(rew.cpu().numpy(), erew.astype(F32))
    _assert_same('wide.npz/%s' % name, _host_batch(env), E, done == 0, rounding=dtype == torch.float32)
    assert_guard_intact(env, 'step')


@pytest.mark.parametrize('stats', [False, True], ids=['plain', 'stats'])
@pytest.mark.parametrize('kernel', ['lane', 'quad', 'pair'])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', ['mp3', 'mp6_solo', 'solo_easy'])
def test_step_teacher_forced_at_default_slots(name, dtype, kernel, stats):
    """steps.npz's configs of 3, 6 and 1 planets with the p_pad a BatchedEnv
    gives them by default (max_planets; tests/test_gpu_parity.py runs them with
    8 slots), no auto-reset: the one-tick instances without helper waves."""
    tr = gio.Transitions('steps.npz')
    cfg = gio.configs()[name]
    idx = dict(tr.groups())[name]
    S = 1 if cfg.solo else 2
    b_cap = tr.max_bullets(idx) + 2
    B = tr.batch_in(idx, S, p_pad=cfg.max_planets, b_cap=b_cap)
    env = _env(cfg, idx.size, cfg.max_planets, dtype, kernel, auto_reset=False, b_cap=b_cap)
    assert env.launch_waves()[1] == 0
    env.load_host(B.ships, B.ships_b, B.planets, B.bullets, B.tick, B.nplanets, B.nbullets)
    ctl = tr.z['control'][idx, :S].astype(np.int8)
    _, rew, done = env.step(torch.from_numpy(ctl).cuda(), auto_reset=False, stats=stats)
    E, erew, edone = tr.expected(idx, S, p_pad=cfg.max_planets, b_cap=b_cap)
    done = done.cpu().numpy()
    assert (done == edone).all()
    assert np.array_equal(rew.cpu().numpy(), erew.astype(F32))
    _assert_same('steps.npz/%s' % name, _host_batch(env), E, done == 0, rounding=dtype == torch.float32)
    assert_guard_intact(env, 'step')


# ------------------------------------------ (d) multi-tick paths equal stepping

STATE = ('ships', 'ships_b', 'planets', 'bullets', 'hdr', 'stream', 'stream_ring')
MULTI = [pytest.param(p, k, id='pad%d-%s' % (p, k)) for p in (3, 6) for k in ('quad', 'pair')]
MULTI.append(pytest.param(16, 'lane', id='pad16-lane'))


@pytest.mark.parametrize('policy', ['random', 'nothing', 'script'])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('p_pad,kernel', MULTI)
def test_multi_tick_paths_equal_stepping(p_pad, kernel, dtype, policy):
    """rollout(K, policy) -- the resident rollout for float32 state on quad and
    pair, their multi-tick instance for float64, one launch per tick on lane --
    and step_many == K times controls(policy) then step, bit for bit on every
    state array, reward, done and the statistics, auto-reset included."""
    cfg = _config(p_pad, life=LIFE)
    K, t0 = TICKS, 7
    a, b, c = (_env(cfg, N, p_pad, dtype, kernel) for _ in range(3))
    for e in (a, b, c):
        assert e.step_kernel == kernel
        e.reset()
    rew, done = a.rollout(K, policy, seed=3, tick0=t0)
    ctl = torch.empty((K, N, b.S), dtype=torch.int8, device=DEV)
    for k in range(K):
        ctl[k] = b.controls(policy, seed=3, tick0=t0 + k)
        _, r, d = b.step(ctl[k])
        assert torch.equal(rew[k], r) and torch.equal(done[k], d), k
    rew_c, done_c = c.step_many(ctl)
    assert torch.equal(rew_c, rew) and torch.equal(done_c, done)
    for other, what in ((a, 'rollout'), (c, 'step_many')):
        for f in STATE:
            assert torch.equal(getattr(other, f), getattr(b, f)), (what, f)
        assert other.stat_dict() == b.stat_dict(), what
    assert int(done.ne(0).sum()) >= N and int(b.nbullets.sum()) > 0
    assert not torch.isnan(b.planets).any()
    npl = b.nplanets.cpu().numpy()
    assert npl.min() >= 1 and npl.max() == p_pad
    for e, what in ((a, 'rollout'), (b, 'controls and step'), (c, 'step_many')):
        assert_guard_intact(e, what)


# ------------------------------------------------------ (e) ScriptBot decisions

def _script_cases():
    """(Transitions, rows, config, p_pad, reference decisions [rows, S])."""
    wide = _wide()
    for name, p_pad in WIDE:
        idx = dict(wide.groups())[name]
        yield name, wide, idx, gio.wide_configs()[name], p_pad, wide.z['script_control'][idx]
    steps = gio.Transitions('steps.npz')   # 3 slots: the 4-register instances read aliased slots
    idx = dict(steps.groups())['mp3']
    yield 'mp3', steps, idx, gio.configs()['mp3'], 3, gio.load('script_controls.npz')['control'][idx]


def _script_env(tr, idx, cfg, p_pad, dtype, kernel='auto'):
    S = 1 if cfg.solo else 2
    b_cap = tr.max_bullets(idx) + 2
    B = tr.batch_in(idx, S, p_pad=p_pad, b_cap=b_cap)
    env = _env(cfg, idx.size, p_pad, dtype, kernel, auto_reset=False, b_cap=b_cap)
    env.load_host(B.ships, B.ships_b, B.planets, B.bullets, B.tick, B.nplanets, B.nbullets)
    return env


@pytest.mark.parametrize('dtype', DTYPES)
def test_scriptbot_decisions_match_reference(dtype):
    """astro_controls' ScriptBot on the fixture's states at 11 and 16 slots (1
    and 2 ships) and on the 3-planet-config states at 3 slots == the
    reference ScriptBot's decision for every ship."""
    checked = 0
    for name, tr, idx, cfg, p_pad, want in _script_cases():
        assert all(_dtype_rule_holds(tr, i) for i in idx), name
        env = _script_env(tr, idx, cfg, p_pad, dtype)
        got = env.controls('script').cpu().numpy()
        bad = np.nonzero((got != want[:, :env.S]).any(1))[0]
        assert bad.size == 0, (name, p_pad, idx[bad[:5]], got[bad[:5]], want[bad[:5], :env.S])
        assert_guard_intact(env, name)
        checked += idx.size * env.S
    assert checked > 1000


@pytest.mark.parametrize('kernel', ['lane', 'pair'])
def test_scripted_rollout_tick_equals_step_with_reference_decisions(kernel):
    """One tick of the scripted rollout from every such state == astro_step
    with the reference's decisions (the pair instance at 3 slots; above 8
    slots every kernel choice runs the lane kernel)."""
    for name, tr, idx, cfg, p_pad, want in _script_cases():
        a = _script_env(tr, idx, cfg, p_pad, torch.float64, kernel)
        b = _script_env(tr, idx, cfg, p_pad, torch.float64, kernel)
        assert a.step_kernel == (kernel if p_pad <= 8 else 'lane')
        ra, da = a.rollout(1, 'script', auto_reset=False)
        _, rb, db = b.step(torch.from_numpy(want[:, :a.S].astype(np.int8)).cuda(), auto_reset=False)
        assert torch.equal(da[0], db) and torch.equal(ra[0], rb), name
        run = db == 0
        assert int(run.sum()) > 0
        for f in ('ships', 'ships_b'):
            assert torch.equal(getattr(a, f)[:, run], getattr(b, f)[:, run]), (name, f)
        assert torch.equal(a.hdr[run], b.hdr[run]), name
        assert_guard_intact(a, name)
        assert_guard_intact(b, name)


# -------------------------------------------------------------- (f) features

def _live_controls(n, nships, seed):
    return np.random.RandomState(seed).randint(0, 6, size=(TICKS, n, nships)).astype(np.int8)


def _fresh_mask(n):
    return np.arange(n) % 7 == 3


def _live(max_planets, p_pad, dtype, n=N, solo=False, seed=5):
    """A guarded auto-reset env after TICKS random ticks of LIFE-tick games,
    every seventh env then reset: bullets in flight, games of several ages,
    some at tick 0.  Checked against the oracle's own run of the same games."""
    env = _env(_config(max_planets, solo, LIFE), n, p_pad, dtype)
    env.reset()
    env.step_many(torch.from_numpy(_live_controls(n, env.S, seed)).cuda())
    env.reset(mask=torch.from_numpy(_fresh_mask(n).astype(np.uint8)).cuda())
    want = live_oracle(max_planets, p_pad, n, solo, seed, 'f32' if dtype == torch.float32 else 'f64')
    got = _host_batch(env)
    assert np.array_equal(got.nplanets, want.nplanets)
    _assert_same('live state', got, want, np.ones(n, bool), rounding=False)
    return env


@functools.lru_cache(maxsize=None)
def live_oracle(max_planets, p_pad, n, solo, seed, store):
    """The oracle's own run of ``_live`` (nothing from the device enters it)."""
    cfg = _config(max_planets, solo, LIFE)
    P = batched.make_params(cfg)
    seeds = batched.game_seeds(batched.stream_seeds(cfg.seed, n), TICKS + 2)
    B = batched.create(seeds[:, 0], P, p_pad=p_pad, b_cap=B_CAP, store=store)
    games = np.ones(n, np.int64)
    ctl = _live_controls(n, P.nships, seed)
    for t in range(TICKS + 1):
        if t < TICKS:
            B, _, done = batched.step(B, ctl[t], P, store=store)
            fin = np.nonzero(done)[0]
        else:
            fin = np.nonzero(_fresh_mask(n))[0]
        if fin.size:
            B.put(fin, batched.create(seeds[fin, games[fin]], P, p_pad=p_pad, b_cap=B_CAP, store=store))
            games[fin] += 1
    for f in B.__dataclass_fields__:
        getattr(B, f).setflags(write=False)
    return B


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('p_pad', [1, 3, 11, 16])
def test_features(p_pad, dtype):
    """astro_features of a live state == oracle.features.batched exactly, with
    the default rows = p_pad + b_cap and with fewer rows than an env has
    objects (the objects past ``rows`` are left out, nothing is written behind
    the buffer); at 11 and 16 slots also the reference's own get_features of
    the fixture's states."""
    env = _live(p_pad, p_pad, dtype)
    B = _host_batch(env)
    objects = B.nplanets + B.nbullets
    assert (B.nbullets > 0).any() and (B.tick == 0).any() and (B.tick > 0).any() and B.nplanets.max() == p_pad
    D = 1 + 5 * env.S + 4
    got = env.features().cpu().numpy()
    assert got.shape == (N, p_pad + B_CAP, D)
    assert np.array_equal(got.view(np.uint32), features.batched(B, env.S, p_pad + B_CAP).view(np.uint32))
    for rows in (1, max(1, int(objects.max()) - 2)):
        assert rows < objects.max()
        out, big = guarded(torch.zeros((N, rows, D), dtype=torch.float32, device=DEV))
        assert env.features(rows=rows, out=out) is out
        assert np.array_equal(out.cpu().numpy().view(np.uint32), features.batched(B, env.S, rows).view(np.uint32))
        guard_untouched(out, big, 'features, rows %d' % rows)
    assert_guard_intact(env, 'features')
    fx = gio.Features('wide.npz')
    for name, pad in WIDE:
        if pad != p_pad:
            continue
        env, idx, b_cap = _loaded(name, p_pad, dtype)
        got = env.features().cpu().numpy()
        assert got.shape == (idx.size, p_pad + b_cap, 1 + 5 * env.S + 4)
        for r, i in enumerate(idx):
            want = fx.of(i)
            assert np.array_equal(got[r, :want.shape[0]].view(np.uint32), want.view(np.uint32)), (name, i)
            assert (got[r, want.shape[0]:] == -1).all(), (name, i)
        assert_guard_intact(env, 'features of ' + name)


# -------------------------------------------- (g) the acting Q-network kernels

QN = 70
Q_SEED = 5   # the state's controls; see test_qvalues' docstring


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('p_pad,solo', [(3, False), (16, False), (16, True)],
                         ids=['pad3', 'pad16', 'pad16-solo'])
def test_qvalues(p_pad, solo, dtype):
    """astro_qvalues and astro_qvalues_ships on a live state against
    qnet.forward64 of the host's features of that state: within tol = 4 max
    |float32 torch CPU - float64| on the same views; controls by the argmax
    rule, which may skip at most 10 % of the decisions (for Q_SEED the float64
    reference alone, on the oracle's own run of the same games and controls,
    stays far below that: tests/test_wide_host.py::test_qvalues_seed_decides); the
    per-ship kernel equals astro_qvalues bit for bit."""
    from astro_amd import qnet
    kind = qu.kind(1 if solo else 2)
    wts = qu.fixture()[0][kind]['weights']
    net = qnet.QNetwork.from_module(wts, DEV)
    env = _live(p_pad, p_pad, dtype, n=QN, solo=solo, seed=Q_SEED)
    S = env.S
    B = _host_batch(env)
    assert (B.nbullets > 0).sum() > QN // 2 and B.nplanets.max() == p_pad
    q64, e_ref = qu.reference_of(wts, B, S)
    tol = 4.0 * e_ref
    q = torch.full((QN, S, net.nout), float('nan'), device=DEV)
    ctl = env.qcontrols(net, q_out=q)
    assert not torch.isnan(q).any()
    err = np.abs(q.cpu().numpy().astype(F64) - q64).max()
    print('p_pad %d %s %s: e_ref %.3g, error %.3f tol' % (p_pad, kind, str(dtype)[6:], e_ref, err / tol))
    assert err <= tol, (err, tol)
    checked, skipped = qu.check_argmax_rule(q64, ctl.cpu().numpy(), tol)
    print('argmax rule: %d of %d decisions skipped' % (skipped, checked))
    assert checked == QN * S and skipped <= 0.10 * checked
    assert torch.equal(env.qvalues(net).view(torch.int32), q.view(torch.int32))
    per_ship = (net,) * S
    q2 = torch.full((QN, S, net.nout), float('nan'), device=DEV)
    ctl2 = env.qcontrols(per_ship, q_out=q2)
    assert torch.equal(q2.view(torch.int32), q.view(torch.int32)) and torch.equal(ctl2, ctl)
    assert torch.equal(env.qvalues(per_ship).view(torch.int32), q.view(torch.int32))
    assert_guard_intact(env, 'qvalues')
