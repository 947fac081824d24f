"""The games an auto-reset creates, bit for bit against the oracle's create().

The pair kernel's helper waves run a lean reset pass (wave_reset_pass,
astro_kernels.hip): nothing comes from the leader lanes by a shuffle, and with
planets_only > 1 the planet count and create()'s two values that depend on it
and the config alone -- the orbital speed sqrt(gravity * planet_mass * (n - 1)
/ 2) and the angle 2 pi / n between planets -- are scalars made on the host
(UniformCreate).  Every other instance keeps the general pass.  These tests
re-create every env of a batch over and over, on every kernel, and compare
every new game -- ships, bearings, planets, header, game seed -- with the
oracle:

  life 1: max_time ends every game at its first step, so every env re-creates
          every tick, its pending seed still undrawn: the serial create
          (create_env over the env's lanes);
  life 3: the first steps draw and check the pending seed, the third ends the
          game: the reset pass (create_env_row, four games at a time, in the
          helper waves of the quad and pair kernels), and the serial create
          for the filtered stream's seeds not yet found.

N = 517 gives partial waves and a partial workgroup, and a last reset-pass
row group of one (quad: 32 full waves + 5 envs; pair: 16 + 5).
"""
import functools

import numpy as np
import pytest
import torch

from oracle import batched, mt19937
from tests import golden_io as gio

pytestmark = pytest.mark.gpu

CFG = gio.configs()
N = 517
TICKS = 12
F32, F64 = np.float32, np.float64
# (planets_only, max_planets): the c3 games; 1..4 planets (the n <= 1 planet
# branch); 1..8 planets (the 8-slot row create)
CASES = {'po3_mp4': (3, 4), 'po0_mp4': (0, 4), 'po0_mp8': (0, 8)}


def _config(max_planets, life):
    cfg = CFG['default']._replace(max_planets=max_planets)
    return cfg._replace(max_time=cfg.dt * life)


@functools.lru_cache(maxsize=None)
def _reference(case):
    """(seeds [N, G], create() of every one of them as a float64 Batch of N * G
    games): computed once per case and shared, never written to."""
    planets_only, max_planets = CASES[case]
    cfg = _config(max_planets, 1)
    stream_seeds = batched.stream_seeds(cfg.seed, N)
    games = TICKS + 1
    if planets_only:
        seeds = batched.filtered_game_seeds(stream_seeds, games, planets_only, max_planets, draws=40 * games)
    else:
        seeds = batched.game_seeds(stream_seeds, games)
    want = batched.create(seeds.reshape(-1), batched.make_params(cfg), p_pad=max_planets, b_cap=8, store='f64')
    for f in want.__dataclass_fields__:
        getattr(want, f).setflags(write=False)
    seeds.setflags(write=False)
    return seeds, want


def _check_fresh(env, case, game, where):
    """Every env whose game is at tick 0 holds create() of its stream's game
    number game[i]; returns how many were checked."""
    seeds, want = _reference(case)
    h = env.to_host()
    fresh = np.nonzero(h['tick'] == 0)[0]
    k = fresh * seeds.shape[1] + game[fresh]
    rnd = (lambda a: a.astype(F32).astype(F64)) if env.dtype == torch.float32 else (lambda a: a)
    got_seed = env.game_seed.cpu().numpy().view(np.uint32)
    assert np.array_equal(got_seed[fresh], seeds[fresh, game[fresh]]), where
    assert np.array_equal(h['nplanets'][fresh], want.nplanets[k]), where
    assert not h['nbullets'][fresh].any() and not h['flags'][fresh].any(), where
    assert np.array_equal(h['ships'][fresh].astype(F64), rnd(want.ships[k])), where
    assert np.array_equal(h['ships_b'][fresh].astype(F64), rnd(want.ships_b[k])), where
    live = np.arange(env.p_pad)[None, :] < want.nplanets[k][:, None]
    assert np.array_equal(h['planets'][fresh].astype(F64)[live], rnd(want.planets[k])[live]), where
    return fresh.size


def _env(case, life, dtype, kernel):
    from astro_amd import BatchedEnv
    planets_only, max_planets = CASES[case]
    env = BatchedEnv(_config(max_planets, life), N, device='cuda:0', b_cap=8, dtype=dtype,
                     planets_only=planets_only, kernel=kernel)
    assert np.array_equal(env.stream_seeds, batched.stream_seeds(env.config.seed, N))
    env.reset()
    return env


@pytest.mark.parametrize('stats', [False, True])
@pytest.mark.parametrize('kernel', ['lane', 'quad', 'pair'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('case', sorted(CASES))
def test_recreated_games_equal_oracle_create(case, dtype, kernel, stats):
    ctl = torch.full((N, 2), 2, dtype=torch.int8, device='cuda')
    for life in (1, 3):
        env = _env(case, life, dtype, kernel)
        game = np.zeros(N, np.int64)
        assert _check_fresh(env, case, game, (life, 'reset')) == N
        env.stats.zero_()
        checked = 0
        for t in range(TICKS):
            _, _, done = env.step(ctl, stats=stats)
            d = done.cpu().numpy() != 0
            if (t + 1) % life == 0:   # (a game also ends when its ships collide: none does this early)
                assert d.all(), (life, t)
            game += d
            if d.any():
                assert _check_fresh(env, case, game, (life, t)) == d.sum()
                checked += int(d.sum())
        assert checked >= N * (TICKS // life)
        if stats and kernel != 'lane':
            s = env.stat_dict()
            assert s['resets'] == checked
            if life == 1:   # an undrawn pending seed: every reset by the serial create
                assert s['serial_resets'] == checked
            elif CASES[case][0] == 0:   # unfiltered, seed and key known: every reset by the reset pass
                assert s['serial_resets'] == 0
            else:   # filtered: both paths
                assert 0 < s['serial_resets'] < checked


@pytest.mark.parametrize('kernel', ['quad', 'pair'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('case', sorted(CASES))
def test_rollout_recreated_games_equal_oracle_create(case, dtype, kernel):
    """The K-tick launches (the resident rollout for float32 state, quad_tick's
    multi-tick instance for float64): their step waves run the reset passes
    themselves.  12 ticks of 3-tick games: every env ends on its fourth new game."""
    env = _env(case, 3, dtype, kernel)
    _, done = env.rollout(TICKS, 'nothing', stats=False)
    d = done.cpu().numpy() != 0
    assert d[2::3].all()
    assert _check_fresh(env, case, d.sum(0).astype(np.int64), 'rollout') == N


@pytest.mark.parametrize('kernel', ['quad', 'pair'])
@pytest.mark.parametrize('n', [517, 701])
def test_serial_resets_counted_in_a_partial_last_block(n, kernel):
    """Every game ends at its first step, so every reset takes the serial path
    and is counted by the helper wave that ran it, in the stats row of the
    step wave it serves -- also the helper of a partial last workgroup's first
    step wave, whose own wave index names a row past the last env."""
    from astro_amd import BatchedEnv
    cfg = _config(4, 1)
    env = BatchedEnv(cfg, n, device='cuda:0', b_cap=8, planets_only=3, kernel=kernel)
    assert env.launch_waves()[1] > 0, 'not a helper-wave instance'
    env.reset()
    env.stats.zero_()
    ctl = torch.full((n, 2), 2, dtype=torch.int8, device='cuda')
    steps, want = 5, 0
    for _ in range(steps):
        _, _, done = env.step(ctl, stats=True)
        want += int((done != 0).sum())   # the oracle's count: a game of one tick always times out
    assert want == n * steps
    s = env.stat_dict()
    assert s['resets'] == want and s['timeouts'] == want
    assert s['serial_resets'] == want


def test_planet_speeds_for_every_planet_count():
    """Games of every planet count 1..8 from explicit seeds (astro_reset's
    create, the device's own float64 sqrt and division), for two parameter
    sets one after the other in one process, against the oracle's create()."""
    from astro_amd import BatchedEnv
    base = CFG['default']._replace(max_planets=8)
    cand = np.arange(1, 4001, dtype=np.uint32)
    count = 1 + (mt19937.first_words(cand) & np.uint32(7)).astype(np.int64)
    seeds = np.concatenate([cand[count == k][:8] for k in range(1, 9)])
    assert seeds.size == 64
    for cfg in (base, base._replace(gravity=base.gravity * 1.7, planet_mass=base.planet_mass * 0.3), base):
        want = batched.create(seeds, batched.make_params(cfg), p_pad=8, b_cap=8, store='f64')
        assert np.array_equal(want.nplanets, np.repeat(np.arange(1, 9), 8))
        for dtype in (torch.float32, torch.float64):
            for kernel in ('lane', 'pair'):
                env = BatchedEnv(cfg, seeds.size, device='cuda:0', b_cap=8, dtype=dtype, kernel=kernel)
                env.reset(seeds=seeds)
                h = env.to_host()
                rnd = (lambda a: a.astype(F32).astype(F64)) if dtype == torch.float32 else (lambda a: a)
                assert np.array_equal(h['nplanets'], want.nplanets)
                live = np.arange(8)[None, :] < want.nplanets[:, None]
                assert np.array_equal(h['planets'].astype(F64)[live], rnd(want.planets)[live]), (cfg.gravity, dtype)
                assert np.array_equal(h['ships'].astype(F64), rnd(want.ships))


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
def test_host_made_constants_for_every_planet_count(dtype):
    """No symbol exports the host-made constants, so they are checked through
    what they produce: planets_only = n for every n in 2..8 (max_planets 8,
    a second parameter set for the odd n) on the pair kernel's helper waves,
    3-tick games, every re-created game against the oracle's create()."""
    from astro_amd import BatchedEnv
    n_env, ticks = 96, 6
    ctl = torch.full((n_env, 2), 2, dtype=torch.int8, device='cuda')
    rnd = (lambda a: a.astype(F32).astype(F64)) if dtype == torch.float32 else (lambda a: a)
    for n in range(2, 9):
        cfg = _config(8, 3)
        if n & 1:
            cfg = cfg._replace(gravity=cfg.gravity * 1.7, planet_mass=cfg.planet_mass * 0.3)
        env = BatchedEnv(cfg, n_env, device='cuda:0', b_cap=8, dtype=dtype, planets_only=n, kernel='pair')
        assert env.launch_waves()[1] > 0, 'not a helper-wave instance'
        env.reset()
        seeds = batched.filtered_game_seeds(env.stream_seeds, 1 + ticks // 3, n, 8, draws=400)
        game = np.zeros(n_env, np.int64)
        for t in range(ticks):
            _, _, done = env.step(ctl, stats=False)
            game += done.cpu().numpy() != 0
        assert (game == ticks // 3).all()
        want = batched.create(seeds[np.arange(n_env), game], batched.make_params(cfg), p_pad=8, b_cap=8, store='f64')
        h = env.to_host()
        assert (h['tick'] == 0).all() and (h['nplanets'] == n).all() and (want.nplanets == n).all()
        assert np.array_equal(env.game_seed.cpu().numpy().view(np.uint32), seeds[np.arange(n_env), game])
        assert np.array_equal(h['planets'].astype(F64)[:, :n], rnd(want.planets)[:, :n]), n
        assert np.array_equal(h['ships'].astype(F64), rnd(want.ships)), n
        assert np.array_equal(h['ships_b'].astype(F64), rnd(want.ships_b)), n
