"""The world-parameter axis on the device: every copy of the physics in the
step library (lane, quad and pair step kernels, counting and plain; the
generic and resident rollouts; astro_game_step; astro_reset's create, the
in-kernel re-create and the host-made create constants; the ScriptBot of
astro_controls and of the rollouts) under configs whose eleven world constants
all differ from DEFAULT_CONFIG's.  Needs an MI355X.

tests/golden/world.npz was written by tools/gen_golden.py from the reference
itself; every value of its configs is inexact in float32 and no power-of-two
multiple of the default, so a dropped ``thrust``, ``gravity`` in place of
``gravity * planet_mass`` or a constant applied as the double where the
reference applies float32(c) changes a result.  tests/test_world_host.py pins
the CPU oracle to the same fixture and shows, on the CPU, that the fixture
sees each constant.

Bars as in tests/test_gpu_parity.py, no tolerance anywhere: float64 state
bit-exact; float32 state equal to the float32 rounding of the reference value
computed from the same float32 input state; integers exact."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

from astro_amd import bots as hbots
from astro_amd.core import roll_ships
from oracle import batched, port
from tests import golden_io as gio
from tests.test_gpu_parity import _assert_same, _auto_reset_vs_oracle, _host_batch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
F32, F64 = np.float32, np.float64
WORLD = gio.world_configs()
DTYPES = [pytest.param(torch.float64, id='f64'), pytest.param(torch.float32, id='f32')]
KERNELS = ['lane', 'quad', 'pair']
STATS = [pytest.param(False, id='plain'), pytest.param(True, id='stats')]
# (kernel, planet slots): every step kernel at 8 slots, the 16-register lane instances
SLOTS = [pytest.param(k, 8, id=k + '-pad8') for k in KERNELS] + [pytest.param('lane', 16, id='lane-pad16')]
N, TICKS, LIFE, B_CAP = 517, 48, 20, 32    # a partial last block; every env re-creates at least twice


def _env(cfg, n, dtype, kernel='auto', p_pad=8, b_cap=B_CAP, auto_reset=False, planets_only=0):
    from astro_amd import BatchedEnv
    env = BatchedEnv(cfg, n, device=DEV, b_cap=b_cap, p_pad=p_pad, dtype=dtype, auto_reset=auto_reset,
                     kernel=kernel, planets_only=planets_only)
    assert kernel == 'auto' or env.step_kernel == ('lane' if p_pad > 8 else kernel)
    env.reward.fill_(float('nan'))     # every launch has to write its outputs
    env.done.fill_(0xff)
    return env


def _rnd(dtype):
    return (lambda a: a.astype(F32).astype(F64)) if dtype == torch.float32 else (lambda a: a)


def _short(name):
    """The config with games of LIFE ticks' worth of max_time (auto-reset tests)."""
    cfg = WORLD[name]
    return cfg._replace(max_time=cfg.dt * LIFE)


@functools.lru_cache(maxsize=None)
def _tr():
    return gio.Transitions('world.npz')


@functools.lru_cache(maxsize=None)
def _z():
    z = gio.load('world.npz')
    return {k: z[k] for k in z.files}


# ------------------------------------------------------------------ (a) create

@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kernel,p_pad', SLOTS + [pytest.param(k, 1, id=k + '-pad1') for k in KERNELS])
def test_create_matches_world_fixture(kernel, p_pad, dtype):
    """reset(seeds=...) == the reference's own create() arrays: every planet
    count, both ship arrangements and both orbit directions under ``world``'s
    constants, and each constant create() reads changed alone.  The reference's
    ship and planet positions are float32, so both state formats hold them
    exactly; its planet velocities are float64."""
    z = _z()
    names = ['world_one'] if p_pad == 1 else [k for k in gio.WORLD_CREATED if k != 'world_one']
    for name in names:
        cfg = WORLD[name]
        seeds = z[name + '__seed']
        env = _env(cfg, seeds.size, dtype, kernel, p_pad, b_cap=4)
        env.ships.fill_(float('nan'))
        env.ships_b.fill_(float('nan'))
        env.reset(seeds=seeds)
        h = env.to_host()
        S, npl = env.S, z[name + '__nplanets']
        assert (h['nplanets'] == npl).all() and not h['tick'].any() and not h['nbullets'].any(), name
        assert np.array_equal(h['ships'][..., 0:2].astype(F64), z[name + '__ships_x'][:, :S].astype(F64)), name
        assert not h['ships'][..., 2:4].any(), name
        assert np.array_equal(h['ships_b'].astype(F64), z[name + '__ships_b'][:, :S].astype(F64)), name
        w = min(p_pad, 8)      # (the fixture's arrays have 8 planet slots)
        pv = np.arange(w)[None, :] < npl[:, None]
        assert pv.sum() == npl.sum()
        assert np.array_equal(h['planets'][:, :w, 0:2][pv].astype(F64),
                              z[name + '__planets_x'][:, :w][pv].astype(F64)), name
        assert np.array_equal(h['planets'][:, :w, 2:4][pv].astype(F64),
                              _rnd(dtype)(z[name + '__planets_dx'][:, :w][pv])), name
        assert (env.game_seed.cpu().numpy().view(np.uint32) == seeds).all(), name


# --------------------------------------------------------------- (b) re-create

RECREATE = {'world': ('world', 0), 'world_mp8': ('world_mp8', 0), 'world_solo': ('world_solo', 0),
            'world_mp8_po3': ('world_mp8', 3)}    # planets_only = 3: the host-made create constants
GAMES = 8


@functools.lru_cache(maxsize=None)
def _recreated(case):
    """(config, life in steps, seeds [N, GAMES], create() of every one of them in
    float64): computed once per case, shared and never written to."""
    name, only = RECREATE[case]
    cfg = _short(name)
    P = batched.make_params(cfg)
    stream = batched.stream_seeds(cfg.seed, N)
    if only:
        seeds = batched.filtered_game_seeds(stream, GAMES, only, cfg.max_planets, draws=60 * GAMES)
    else:
        seeds = batched.game_seeds(stream, GAMES)
    want = batched.create(seeds.reshape(-1), P, p_pad=8, b_cap=1, store='f64')
    for f in want.__dataclass_fields__:
        getattr(want, f).setflags(write=False)
    seeds.setflags(write=False)
    return cfg, P.timeout_tick + 1, seeds, want


def _check_fresh(env, case, game, where):
    """tests/test_gpu_reset_create.py's rule: every env at tick 0 holds create()
    of its stream's game number game[i].  Returns how many were checked."""
    _, _, seeds, want = _recreated(case)
    h = env.to_host()
    fresh = np.nonzero(h['tick'] == 0)[0]
    assert game[fresh].max() < GAMES, where
    k = fresh * GAMES + game[fresh]
    rnd = _rnd(env.dtype)
    assert np.array_equal(env.game_seed.cpu().numpy().view(np.uint32)[fresh], seeds[fresh, game[fresh]]), where
    assert np.array_equal(h['nplanets'][fresh], want.nplanets[k]), where
    assert not h['nbullets'][fresh].any() and not h['flags'][fresh].any(), where
    assert np.array_equal(h['ships'][fresh].astype(F64), rnd(want.ships[k])), where
    assert np.array_equal(h['ships_b'][fresh].astype(F64), rnd(want.ships_b[k])), where
    live = np.arange(8)[None, :] < want.nplanets[k][:, None]
    assert np.array_equal(h['planets'][fresh].astype(F64)[live], rnd(want.planets[k])[live]), where
    return fresh.size


def _recreate_env(case, dtype, kernel):
    cfg, life, _, _ = _recreated(case)
    assert life in (LIFE, LIFE + 1)
    env = _env(cfg, N, dtype, kernel, auto_reset=True, planets_only=RECREATE[case][1])
    assert np.array_equal(env.stream_seeds, batched.stream_seeds(cfg.seed, N))
    env.reset()
    return env, life


@pytest.mark.parametrize('stats', STATS)
@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', sorted(RECREATE))
def test_recreated_games_equal_oracle_create(case, dtype, kernel, stats):
    """48 one-tick launches of 20-tick games: every game the step kernel
    re-creates (the reset pass of the helper waves, the serial create) is the
    oracle's create() of the stream's next seed under these constants."""
    env, life = _recreate_env(case, dtype, kernel)
    ctl = torch.full((N, env.S), 2, dtype=torch.int8, device=DEV)
    game = np.zeros(N, np.int64)
    assert _check_fresh(env, case, game, 'reset') == N
    env.stats.zero_()
    checked = 0
    for t in range(TICKS):
        _, _, done = env.step(ctl, stats=stats)
        d = done.cpu().numpy() != 0
        game += d
        if d.any():
            assert _check_fresh(env, case, game, t) == d.sum()
            checked += int(d.sum())
    assert (game >= TICKS // life).all() and checked >= 2 * N
    if stats:
        assert env.stat_dict()['resets'] == checked
    env.check_errors()


@pytest.mark.parametrize('kernel', ['quad', 'pair'])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', sorted(RECREATE))
def test_rollout_recreated_games_equal_oracle_create(case, dtype, kernel):
    """The K-tick launches (the resident rollout for float32 state, the
    multi-tick instance for float64) run their own reset passes: 48 ticks in
    launches that each end where the timeouts fall."""
    env, life = _recreate_env(case, dtype, kernel)
    game = np.zeros(N, np.int64)
    left = TICKS
    while left > 0:
        k = min(life, left)
        _, done = env.rollout(k, 'nothing', stats=False)
        game += (done.cpu().numpy() != 0).sum(0)
        left -= k
        if k == life:       # every game that did not end by a collision before timed out on the last tick
            assert _check_fresh(env, case, game, 'rollout') >= N - N // 8
    assert (game >= TICKS // life).all()
    env.check_errors()


# ---------------------------------------------------- (c), (g) teacher-forced steps

def _slots(batch, p_pad):
    """The Batch (8 planet slots, as the fixture has) with p_pad >= 8 slots."""
    planets = np.zeros((batch.planets.shape[0], p_pad, 4))
    planets[:, :8] = batch.planets
    return dataclasses.replace(batch, planets=planets)


def _teacher_forced(name, dtype, kernel, p_pad, stats):
    tr = _tr()
    cfg = WORLD[name]
    idx = dict(tr.groups())[name]
    S = 1 if cfg.solo else 2
    b_cap = tr.max_bullets(idx) + 2
    B = _slots(tr.batch_in(idx, S, b_cap=b_cap), p_pad)
    env = _env(cfg, idx.size, dtype, kernel, p_pad, b_cap)
    env.load_host(B.ships, B.ships_b, B.planets, B.bullets, B.tick, B.nplanets, B.nbullets)
    ctl = tr.z['control'][idx, :S].astype(np.int8)
    _, rew, done = env.step(torch.from_numpy(ctl).cuda(), auto_reset=False, stats=stats)
    E, erew, edone = tr.expected(idx, S, b_cap=b_cap)
    E = _slots(E, p_pad)
    done = done.cpu().numpy()
    assert (done == edone).all(), (name, np.nonzero(done != edone)[0][:5])     # 0, 1 collision, 2 timeout
    assert np.array_equal(rew.cpu().numpy(), erew.astype(F32)), name
    _assert_same('world.npz/%s' % name, _host_batch(env), E, done == 0, rounding=dtype == torch.float32)
    env.check_errors()
    return idx.size


@pytest.mark.parametrize('stats', STATS)
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kernel,p_pad', SLOTS)
def test_step_teacher_forced_vs_world_fixture(kernel, p_pad, dtype, stats):
    """One step from every input state of the five ``world`` configs (tick 0 and
    its float32 spawn, bullets, every kind of ending, 1-8 planets, the lone
    float32 planet, one ship) == the reference's own output."""
    assert sum(_teacher_forced(name, dtype, kernel, p_pad, stats) for name in gio.WORLD_FULL) > 1300


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('field', gio.WORLD_FIELDS)
def test_step_teacher_forced_single_constant(field, dtype):
    """The same with one constant changed alone, on the default kernel choice:
    a failure of the combined configs comes with the name of its constant."""
    assert _teacher_forced('only_' + field, dtype, 'auto', 8, True) >= 40


# ------------------------------------------------------------- (d) closed loop

@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('name', ['world', 'world_solo'])
def test_step_auto_reset_vs_oracle(name, kernel):
    """tests/test_gpu_parity.py's auto-reset loop: each tick equals the oracle
    stepped from the kernel's own state, each new game the oracle's create(),
    every counter the oracle's sum."""
    rec = {}
    _auto_reset_vs_oracle(_short(name), name, N, TICKS, B_CAP, kernel, True, record=rec)
    assert (rec['games'] > 2).all(), 'an env did not re-create twice'
    assert rec['stats']['planets'] == rec['planets_read']
    rec['env'].check_errors()


@functools.lru_cache(maxsize=None)
def _free_run(name, store):
    """The oracle's own run of TICKS ticks with auto-reset from reset() under
    fixed random controls: (controls, reward and done of every tick, the final
    Batch, each env's game count, the sums of the library's counters)."""
    cfg = _short(name)
    P = batched.make_params(cfg)
    seeds = batched.game_seeds(batched.stream_seeds(cfg.seed, N), GAMES)
    B = batched.create(seeds[:, 0], P, p_pad=8, b_cap=B_CAP, store=store)
    ctl = np.random.RandomState(48).randint(0, 6, size=(TICKS, N, P.nships)).astype(np.int8)
    games = np.ones(N, np.int64)
    sums = dict.fromkeys(('bullets_in', 'bullets_out', 'overflows', 'planets', 'collisions', 'timeouts'), 0)
    rews, dones = [], []
    for t in range(TICKS):
        c = {}
        B, rew, done = batched.step(B, ctl[t], P, store=store, counts=c)
        for k in sums:
            sums[k] += int(c[k].sum())
        fin = np.nonzero(done)[0]
        if fin.size:
            B.put(fin, batched.create(seeds[fin, games[fin]], P, p_pad=8, b_cap=B_CAP, store=store))
            games[fin] += 1
        rews.append(rew)
        dones.append(done)
    assert games.max() < GAMES and (games > 2).all()
    sums['resets'] = int((games - 1).sum())
    sums['serial_resets'] = None
    return ctl, np.stack(rews), np.stack(dones), B, games, seeds, sums


@pytest.mark.parametrize('path', ['step_many', 'rollout'])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('name', ['world', 'world_solo'])
def test_multi_tick_paths_vs_oracle(name, kernel, dtype, path):
    """step_many (k = 7) and rollout with a control array -- for float32 state
    on quad and pair the resident rollout, one launch per tick on lane --
    free-running for 48 ticks against the oracle's own run of the same games:
    every tick's reward and done, the whole final state, every counter."""
    ctl, wrew, wdone, want, games, seeds, sums = _free_run(name, 'f32' if dtype == torch.float32 else 'f64')
    env = _env(_short(name), N, dtype, kernel, auto_reset=True)
    env.reset()
    env.stats.zero_()
    c = torch.from_numpy(ctl).cuda()
    if path == 'rollout':
        rew, done = env.rollout(TICKS, c)
    else:
        parts = [env.step_many(c[k:k + 7]) for k in range(0, TICKS, 7)]
        rew, done = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    assert np.array_equal(done.cpu().numpy(), wdone)
    assert np.array_equal(rew.cpu().numpy(), wrew)
    got = _host_batch(env)
    _assert_same('%s %s final' % (name, path), got, want, np.ones(N, bool), rounding=False)
    assert (got.overflow == want.overflow).all()
    assert np.array_equal(env.game_seed.cpu().numpy().view(np.uint32), seeds[np.arange(N), games - 1])
    st = env.stat_dict()
    for k, v in sums.items():
        assert v is None or st[k] == v, (k, st[k], v)
    assert sums['collisions'] + sums['timeouts'] == sums['resets'] >= 2 * N and sums['timeouts'] > 0
    assert sums['bullets_in'] > 0 or WORLD[name].solo
    env.check_errors()


# --------------------------------------------------------------- (e) ScriptBot

def _script_env(name, dtype, kernel='auto', b_cap=None):
    tr = _tr()
    cfg = WORLD[name]
    idx = dict(tr.groups())[name]
    S = 1 if cfg.solo else 2
    b_cap = tr.max_bullets(idx) + 2 if b_cap is None else b_cap
    B = tr.batch_in(idx, S, b_cap=b_cap)
    env = _env(cfg, idx.size, dtype, kernel, 8, b_cap)
    env.load_host(B.ships, B.ships_b, B.planets, B.bullets, B.tick, B.nplanets, B.nbullets)
    return env, idx, tr.z['script_control'][idx, :S]


@pytest.mark.parametrize('dtype', DTYPES)
def test_scriptbot_decisions_match_reference(dtype):
    """astro_controls' ScriptBot == the reference ScriptBot on every kept state
    (a decision closer than 1e-9, at tick 0 1e-5, to one of script.py's
    thresholds is left out: at most 1 % of them), under every config of the
    fixture: planet_radius + ship_radius, speed / ship_thrust, ship_rspeed,
    bullet_speed and ship_radius all away from their defaults."""
    checked = dropped = 0
    for name in WORLD:
        env, idx, want = _script_env(name, dtype)
        got = env.controls('script').cpu().numpy()
        kept = want >= 0
        bad = np.nonzero(((got != want) & kept).any(1))[0]
        assert bad.size == 0, (name, idx[bad[:5]], got[bad[:5]], want[bad[:5]])
        checked += int(kept.sum())
        dropped += int((want == -2).sum())
    assert checked > 3500 and dropped <= 0.01 * (checked + dropped)


@pytest.mark.parametrize('kernel,dtype', [pytest.param(k, torch.float64, id=k + '-f64') for k in KERNELS]
                         + [pytest.param(k, torch.float32, id=k + '-f32') for k in ('quad', 'pair')])
def test_scripted_rollout_tick_equals_step_with_reference_decisions(kernel, dtype):
    """One tick of rollout(1, 'script') from every state == astro_step with the
    reference's decisions (the envs of a left-out decision are not compared),
    float64 and float32 state.  (Scripted policies run the bots instance of the
    K-tick kernel also where a control array would run the resident rollout --
    float32 state, b_cap <= 32: the library has no resident ScriptBot instance;
    the resident physics is in test_multi_tick_paths_vs_oracle.)"""
    for name in gio.WORLD_FULL:
        a, idx, want = _script_env(name, dtype, kernel)
        b, _, _ = _script_env(name, dtype, kernel)
        ra, da = a.rollout(1, 'script', auto_reset=False)
        ctl = np.where(want >= 0, want, 2).astype(np.int8)
        _, rb, db = b.step(torch.from_numpy(ctl).cuda(), auto_reset=False)
        kept = torch.from_numpy((want >= 0).all(1)).cuda()
        assert int(kept.sum()) > 0.98 * idx.size
        assert torch.equal(da[0][kept], db[kept]) and torch.equal(ra[0][kept], rb[kept]), name
        run = kept & (db == 0)
        assert int(run.sum()) > 0
        for f in ('ships', 'ships_b', 'planets'):
            assert torch.equal(getattr(a, f)[:, run], getattr(b, f)[:, run]), (name, f)
        assert torch.equal(a.bullets[run], b.bullets[run]) and torch.equal(a.hdr[run], b.hdr[run]), name
        a.check_errors()


def _oracle_play(cfg, seed, bots):
    g = port.Game(cfg)
    st = g.create(int(seed))
    t = 0
    while st is not None:
        ctl = np.array([b(roll_ships(st, i)) for i, b in enumerate(bots)])
        st, rew = g.step(st, ctl)
        t += 1
    return (-1 if np.max(rew) < 1 else int(np.argmax(rew))), t


def test_device_play_nothing_vs_script_matches_oracle():
    """32 NothingBot-vs-ScriptBot games of ``world`` (max_time 20) played on
    the device == the CPU oracle driven by the host bots, closed loop."""
    cfg = WORLD['world']._replace(max_time=20)
    n = 32
    env = _env(cfg, n, torch.float64, b_cap=64, auto_reset=True)
    seeds = env.stream_seeds[:n].copy()
    env.reset(seeds=seeds)
    winner, length = env.play(('nothing', 'script'), games=1)
    bots = [hbots.NothingBot(), hbots.ScriptBot.create(cfg)]
    wins = 0
    for k in range(n):
        w, t = _oracle_play(cfg, seeds[k], bots)
        assert (int(winner[k, 0]), int(length[k, 0])) == (w, t), k
        wins += w == 1
    assert wins > n // 2
    env.check_errors()


# --------------------------------------------------- (f) the single-game drop-in

@pytest.mark.parametrize('name', ['world', 'world_solo'])
def test_whole_games_through_hip_shim(name):
    """astro_amd.core.create / core.step (astro_game_step, one float64 env)
    replay the fixture's whole games bit for bit: every tick's ships, planets
    and bullet count, the length and the outcome, with the reference's dtypes."""
    from astro_amd import core
    for g in gio.world_games():
        if g['cfg'] != name:
            continue
        cfg = WORLD[name]._replace(seed=int(g['seed']))
        S = 1 if cfg.solo else 2
        st = core.create(cfg)
        ticks = g['ships'].shape[0]
        for t in range(ticks):
            n = st.planets.x.shape[0]
            assert st.ships.x.dtype == (F32 if t == 0 else F64), (g['gid'], t)
            assert np.array_equal(st.ships.x, g['ships'][t, :S, 0:2]), (g['gid'], t)
            assert np.array_equal(st.ships.dx, g['ships'][t, :S, 2:4]), (g['gid'], t)
            assert np.array_equal(st.ships.b, g['ships'][t, :S, 4]), (g['gid'], t)
            assert np.array_equal(st.planets.x, g['planets'][t, :n, 0:2]), (g['gid'], t)
            assert np.array_equal(st.planets.dx, g['planets'][t, :n, 2:4]), (g['gid'], t)
            assert st.bullets.x.shape[0] == g['nbullets'][t], (g['gid'], t)
            st, rew = core.step(st, g['controls'][t].astype(np.int64), cfg)
            assert (st is None) == (t == ticks - 1), (g['gid'], t)
        assert (1 if rew.dtype.kind == 'i' else 2) == g['done'], g['gid']
        assert np.array_equal(np.asarray(rew, F64), g['reward'][:S]), g['gid']


def test_play_through_hip_shim_matches_oracle():
    """core.play with ScriptBots on the HIP kernel == the oracle's winner and
    length, for two seeds of ``world`` (max_time 20)."""
    from astro_amd import core
    for seed in (11, 12):
        cfg = WORLD['world']._replace(max_time=20, seed=seed)
        game = core.play(cfg, [hbots.ScriptBot.create(cfg), hbots.ScriptBot.create(cfg)])
        w, t = _oracle_play(cfg, seed, [hbots.ScriptBot.create(cfg), hbots.ScriptBot.create(cfg)])
        assert (-1 if game.winner is None else game.winner, len(game.ticks)) == (w, t), seed
