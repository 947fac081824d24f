#!/usr/bin/env python3
"""Generate the golden fixtures under tests/golden/ by running the REFERENCE.

Test infrastructure only.  This script imports DouglasOrr/Astro's own
``astro/core.py`` / ``astro/util.py`` / ``astro/script.py`` from
``/root/reference`` (read-only, via a synthetic package so that
``astro/__init__.py``'s imports of ``rl``/``server`` -- which need the absent
``tensorboardX``/``lru`` -- are skipped) and records inputs and outputs of
``core.create`` (core.py:86-135), ``core.generate_configs`` (core.py:77-83) and
``core.step`` (core.py:215-303), ``rl.ValueNetwork.get_features`` /
``to_batch`` (rl.py:36-112), ``rl.ValueNetwork.forward`` (rl.py:137-155) and
``rl.QBotTrainer``'s experience bookkeeping (rl.py:249-258, 303-328) and
counts of ``rl.EpsilonGreedy``'s transitions (rl.py:10-29),
as small ``.npz``/``.json`` fixtures.  ``wide.npz`` (``gen_wide``) holds
create, steps, ScriptBot decisions and features of configs with 11 and 16
planets; ``python tools/gen_golden.py wide`` rewrites it alone, byte for byte.
``world.npz`` (``gen_world``) holds create, steps, ScriptBot decisions, fire
schedules and whole games of configs with every world constant changed;
``python tools/gen_golden.py world`` rewrites it alone, byte for byte.

It refuses to run when ``/root/reference`` is absent, so it never runs on the
GPU box; the fixtures it writes are plain data (inputs + expected outputs) and
are committed.  Nothing here is imported by the product package.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden.py
"""
import io
import itertools as it
import json
import os
import sys
import types

import numpy as np

REF = '/root/reference/astro'
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden')
P_PAD = 8          # planet padding used by every fixture
S_PAD = 2          # ship padding


def _import_reference():
    if not os.path.isdir(REF):
        sys.exit('gen_golden: /root/reference is absent -- this script only '
                 'runs in the build container')
    sys.dont_write_bytecode = True
    pkg = types.ModuleType('astro')
    pkg.__path__ = [REF]
    sys.modules['astro'] = pkg
    from astro import core, util, script  # noqa: E402
    return core, util, script


core, util, script = _import_reference()

# Named configurations exercised by the fixtures (all derived from the
# reference presets, core.py:52-74).
CONFIGS = {
    'default': core.DEFAULT_CONFIG,
    'solo': core.SOLO_CONFIG,
    'solo_easy': core.SOLO_EASY_CONFIG,
    'mp8': core.DEFAULT_CONFIG._replace(max_planets=8),
    'mp3': core.DEFAULT_CONFIG._replace(max_planets=3),    # masked rejection
    'mp6_solo': core.SOLO_CONFIG._replace(max_planets=6),  # rejection + solo
    'rapid': core.DEFAULT_CONFIG._replace(reload_time=0.01),  # fires at tick 0
    'short': core.DEFAULT_CONFIG._replace(max_time=3.0, reload_time=0.05),
    'solo20': core.SOLO_CONFIG._replace(max_time=20),
}


def cfg_json():
    return {k: dict(v._asdict()) for k, v in CONFIGS.items()}


# ---------------------------------------------------------------------------
# State <-> padded arrays

def pack_state(state, nships, p_pad=P_PAD):
    """Reference State -> padded float64 arrays + counts + dtype flags."""
    ships = np.zeros((S_PAD, 5))
    ships[:nships, 0:2] = state.ships.x
    ships[:nships, 2:4] = state.ships.dx
    ships[:nships, 4] = state.ships.b
    npl = state.planets.x.shape[0]
    planets = np.zeros((p_pad, 4))
    planets[:npl, 0:2] = state.planets.x
    planets[:npl, 2:4] = state.planets.dx
    bullets = np.concatenate([state.bullets.x, state.bullets.dx], axis=1).astype(np.float64)
    flags = (int(state.ships.x.dtype == np.float32) |
             int(state.planets.x.dtype == np.float32) << 1 |
             int(state.planets.dx.dtype == np.float32) << 2 |
             int(state.bullets.x.dtype == np.float32) << 3)
    return ships, planets, npl, bullets, flags


def round_state(state):
    """Round every array of a State to float32 VALUES, keeping its dtype.

    This is the state a float32-storing implementation hands to step(): the
    reference's own promotion path (core.py:234-303) is kept because each
    array keeps its numpy dtype."""
    def r(a):
        return None if a is None else a.astype(np.float32).astype(a.dtype)
    B = core.Bodies
    return core.State(
        ships=B(x=r(state.ships.x), dx=r(state.ships.dx), b=r(state.ships.b)),
        planets=B(x=r(state.planets.x), dx=r(state.planets.dx), b=None),
        bullets=B(x=r(state.bullets.x), dx=r(state.bullets.dx), b=None),
        reload=state.reload, t=state.t)


class TransitionWriter:
    """Ragged store of teacher-forced (state_in, control) -> ref outputs."""

    def __init__(self, configs=None, p_pad=P_PAD):
        self.rows = []
        self.configs = CONFIGS if configs is None else configs
        self.p_pad = p_pad

    def add(self, cfg_name, tick, state_in, control, config):
        nships = state_in.ships.x.shape[0]
        out_state, reward = core.step(state_in, np.asarray(control), config)
        ships, planets, npl, bullets, flags = pack_state(state_in, nships, self.p_pad)
        if out_state is None:
            done = 1 if reward.dtype.kind == 'i' else 2
            o_ships = np.zeros((S_PAD, 5))
            o_planets = np.zeros((self.p_pad, 4))
            o_bullets = np.zeros((0, 4))
        else:
            done = 0
            o_ships, o_planets, _, o_bullets, _ = pack_state(out_state, nships, self.p_pad)
        rew = np.zeros(S_PAD)
        rew[:nships] = reward
        ctl = np.full(S_PAD, 2, dtype=np.int64)
        ctl[:nships] = control
        self.rows.append(dict(
            cfg=list(self.configs).index(cfg_name), tick=tick, nships=nships,
            nplanets=npl, flags=flags, ships=ships, planets=planets,
            bullets=bullets, control=ctl, done=done, reward=rew,
            reward_int=int(reward.dtype.kind == 'i'),
            o_ships=o_ships, o_planets=o_planets, o_bullets=o_bullets))
        return out_state, reward

    def save(self, path):
        np.savez_compressed(path, **self.arrays())
        print('wrote', path, len(self.rows), 'transitions')

    def arrays(self):
        R = self.rows

        def ragged(key):
            arrs = [r[key] for r in R]
            off = np.zeros(len(arrs) + 1, dtype=np.int64)
            off[1:] = np.cumsum([a.shape[0] for a in arrs])
            flat = np.concatenate(arrs, axis=0) if arrs else np.zeros((0, 4))
            return flat, off
        bi, bio = ragged('bullets')
        bo, boo = ragged('o_bullets')
        return dict(
            cfg=np.array([r['cfg'] for r in R], dtype=np.int32),
            tick=np.array([r['tick'] for r in R], dtype=np.int32),
            nships=np.array([r['nships'] for r in R], dtype=np.int32),
            nplanets=np.array([r['nplanets'] for r in R], dtype=np.int32),
            dtype_flags=np.array([r['flags'] for r in R], dtype=np.int32),
            in_ships=np.stack([r['ships'] for r in R]),
            in_planets=np.stack([r['planets'] for r in R]),
            in_bullets=bi, in_bullets_off=bio,
            control=np.stack([r['control'] for r in R]),
            out_done=np.array([r['done'] for r in R], dtype=np.int8),
            out_reward=np.stack([r['reward'] for r in R]),
            out_reward_int=np.array([r['reward_int'] for r in R], dtype=np.int8),
            out_ships=np.stack([r['o_ships'] for r in R]),
            out_planets=np.stack([r['o_planets'] for r in R]),
            out_bullets=bo, out_bullets_off=boo,
            cfg_names=np.array(list(self.configs)),
        )


# ---------------------------------------------------------------------------
# 1. create() + generate_configs()

def gen_create(k=256):
    out = {}
    for name, base in CONFIGS.items():
        configs = list(it.islice(core.generate_configs(base), k))
        seeds = np.array([c.seed for c in configs], dtype=np.uint32)
        npl = np.zeros(k, dtype=np.int32)
        sx = np.zeros((k, S_PAD, 2), np.float32)
        sdx = np.zeros((k, S_PAD, 2), np.float32)
        sb = np.zeros((k, S_PAD), np.float32)
        px = np.zeros((k, P_PAD, 2), np.float32)
        pdx = np.zeros((k, P_PAD, 2), np.float64)
        for i, c in enumerate(configs):
            s = core.create(c)
            n = s.ships.x.shape[0]
            assert s.ships.x.dtype == np.float32 and s.ships.b.dtype == np.float32
            npl[i] = s.planets.x.shape[0]
            sx[i, :n] = s.ships.x
            sdx[i, :n] = s.ships.dx
            sb[i, :n] = s.ships.b
            px[i, :npl[i]] = s.planets.x
            pdx[i, :npl[i]] = s.planets.dx
        for key, val in dict(seed=seeds, nplanets=npl, ships_x=sx, ships_dx=sdx,
                             ships_b=sb, planets_x=px, planets_dx=pdx).items():
            out['%s__%s' % (name, key)] = val
    np.savez_compressed(os.path.join(OUT, 'create.npz'), **out)
    print('wrote create.npz')

    gc = {}
    for seed in [42, 0, 1, 7, 123456789, (1 << 30) - 1, (1 << 32) - 1]:
        c = core.DEFAULT_CONFIG._replace(seed=seed)
        gc['seed_%d' % seed] = np.array(
            [x.seed for x in it.islice(core.generate_configs(c), 300)], dtype=np.uint32)
    np.savez_compressed(os.path.join(OUT, 'generate_configs.npz'), **gc)
    print('wrote generate_configs.npz')


# ---------------------------------------------------------------------------
# 2. Teacher-forced step transitions along reference games

def _controls(policy, rng, nships, state, bots):
    if policy == 'random':
        return rng.randint(0, 6, size=nships)
    if policy == 'nothing':
        return np.full(nships, 2)
    if policy == 'spin_fwd':
        return np.full(nships, 5)
    if policy == 'left_fwd':
        return np.full(nships, 1)
    if policy == 'script':
        return core.Bots.control(bots, state)
    raise ValueError(policy)


def gen_steps():
    w = TransitionWriter()
    plan = [
        # (config, policy, games, keep_every)
        ('default', 'random', 24, 1),
        ('default', 'nothing', 6, 2),
        ('default', 'script', 4, 3),
        ('solo', 'random', 6, 1),
        ('solo_easy', 'nothing', 2, 4),
        ('mp8', 'random', 16, 1),
        ('mp3', 'random', 6, 1),
        ('mp6_solo', 'spin_fwd', 4, 2),
        ('rapid', 'random', 6, 1),
        ('rapid', 'left_fwd', 3, 1),
        ('short', 'random', 8, 1),
        ('solo20', 'script', 2, 25),
    ]
    for cfg_name, policy, games, keep in plan:
        base = CONFIGS[cfg_name]
        for g, config in enumerate(it.islice(core.generate_configs(base), games)):
            rng = np.random.RandomState(1000 + g)
            nships = 1 if config.solo else 2
            bots = [script.ScriptBot.create(config) for _ in range(nships)]
            state = core.create(config)
            tick = 0
            while state is not None:
                ctl = _controls(policy, rng, nships, state, bots)
                nb_before = state.bullets.x.shape[0]
                # free-running reference step decides the trajectory
                nxt, reward = core.step(state, ctl, config)
                interesting = (tick == 0 or nxt is None or
                               (nxt is not None and nxt.bullets.x.shape[0] != nb_before))
                if interesting or tick % keep == 0:
                    w.add(cfg_name, tick, round_state(state), ctl, config)
                state = nxt
                tick += 1
    w.save(os.path.join(OUT, 'steps.npz'))


# ---------------------------------------------------------------------------
# 3. Hand-built edge cases through the reference step

def _mk(ships_x, ships_dx, ships_b, planets_x, planets_dx, bullets_x=(), bullets_dx=(),
        reload=0.0, t=0.0):
    f = lambda a, n: np.asarray(a, dtype=np.float64).reshape(n)  # noqa: E731
    B = core.Bodies
    nb = len(bullets_x)
    return core.State(
        ships=B(x=f(ships_x, (-1, 2)), dx=f(ships_dx, (-1, 2)), b=f(ships_b, (-1,))),
        planets=B(x=f(planets_x, (-1, 2)), dx=f(planets_dx, (-1, 2)), b=None),
        bullets=B(x=f(bullets_x, (nb, 2)), dx=f(bullets_dx, (nb, 2)), b=None),
        reload=reload, t=t)


def gen_edges():
    w = TransitionWriter()
    c = CONFIGS['default']
    solo = CONFIGS['solo']
    far = [[0.6, 0.6], [-0.6, -0.6]]
    still = [[0, 0], [0, 0]]
    cases = [
        # (name, config, state, control, tick)
        ('cull_quirk_kept', c, _mk(far, still, [0, 1], [[0, 0]], [[0, 0]],
                                   [[0.999, 0.0], [0.999, 0.999], [1.5, 0.0], [1.5, 1.5]],
                                   [[1, 0], [1, 1], [1, 0], [1, 1]]), [2, 2], 5),
        ('bullet_in_planet', c, _mk(far, still, [0, 1], [[0, 0]], [[0, 0]],
                                    [[0.19, 0.0], [0.0, -0.2], [0.3, 0.3]],
                                    [[0, 0], [0, 0], [0, 0]]), [2, 2], 5),
        ('coincident_bullets', c, _mk(far, still, [0, 1], [[0, 0]], [[0, 0]],
                                      [[0.4, 0.4], [0.4, 0.4]], [[0, 0.1], [0, 0.1]]), [2, 2], 5),
        ('planet_overlap_not_terminal', c, _mk(far, still, [0, 1],
                                               [[0.1, 0], [-0.1, 0]], [[0, 0.1], [0, -0.1]]),
         [2, 2], 5),
        ('ship_ship', c, _mk([[0.6, 0.6], [0.62, 0.6]], still, [0, 1], [[0, 0]], [[0, 0]]),
         [2, 2], 5),
        ('bullet_hits_ship1', c, _mk([[0.6, 0.6], [-0.6, -0.6]], still, [0, 1], [[0, 0]], [[0, 0]],
                                     [[-0.6, -0.61]], [[0, 1.5]]), [2, 2], 5),
        ('bullet_hits_ship0', c, _mk([[0.6, 0.6], [-0.6, -0.6]], still, [0, 1], [[0, 0]], [[0, 0]],
                                     [[0.6, 0.6249]], [[0, 1.5]]), [2, 2], 5),
        ('wrap_x', c, _mk([[0.999, 0.2], [-0.999, -0.2]], [[1, 0], [-1, 0]], [0, 1],
                          [[0, 0]], [[0, 0]]), [2, 2], 5),
        ('wrap_corner', c, _mk([[0.9999, -0.9999], [-0.5, 0.5]], [[1, -1], [0, 0]], [1, 2],
                               [[0, 0]], [[0, 0]]), [3, 0], 5),
        ('gravity_1_over_r', c, _mk([[0.1, 0.0], [0.0, 0.3]], still, [0, 0], [[0, 0]], [[0, 0]]),
         [2, 2], 5),
        ('thrust_rotate_all_controls_a', c, _mk(far, [[0.1, -0.2], [0.3, 0.05]], [0.3, 2.0],
                                                [[0, 0]], [[0, 0]]), [0, 1], 5),
        ('thrust_rotate_all_controls_b', c, _mk(far, [[0.1, -0.2], [0.3, 0.05]], [-40.0, 123.0],
                                                [[0, 0]], [[0, 0]]), [4, 5], 5),
        ('negative_and_large_controls', c, _mk(far, still, [0.5, 1.0], [[0, 0]], [[0, 0]]),
         [-1, 7], 5),
        ('fire_geometry', c, _mk([[0.6, 0.6], [-0.6, -0.6]], [[0.1, 0], [0, -0.1]], [0.7, 4.0],
                                 [[0, 0]], [[0, 0]], reload=0.29), [3, 3], 14),
        ('timeout_plain', c, _mk(far, still, [0, 1], [[0, 0]], [[0, 0]], t=59.98000000000378),
         [2, 2], 2999),
        ('timeout_solo_win', solo, _mk([[0.6, 0.6]], [[0, 0]], [0], [[0, 0]], [[0, 0]],
                                       t=59.98000000000378), [2], 2999),
        ('collision_beats_timeout', c, _mk([[0.6, 0.6], [-0.6, -0.6]], still, [0, 1],
                                           [[0, 0]], [[0, 0]], [[-0.6, -0.6]], [[0, 0]],
                                           t=59.98000000000378), [2, 2], 2999),
        ('planets_8', CONFIGS['mp8'], _mk(far, [[0.05, 0], [0, 0.05]], [0, 1],
                                          [[0.5 * np.sin(a), 0.5 * np.cos(a)] for a in
                                           np.linspace(0, 2 * np.pi, 8, endpoint=False) + 0.1],
                                          [[0.3 * np.cos(a), -0.3 * np.sin(a)] for a in
                                           np.linspace(0, 2 * np.pi, 8, endpoint=False) + 0.1]),
         [1, 5], 5),
        ('ship_in_planet_1e12_floor', c, _mk([[0.0, 0.0], [-0.6, -0.6]], still, [0, 1],
                                             [[0, 0], [0.5, 0]], [[0, 0], [0, 0]]), [2, 2], 5),
    ]
    names = []
    for name, cfg, state, ctl, tick in cases:
        cfg_name = [k for k, v in CONFIGS.items() if v == cfg][0]
        w.add(cfg_name, tick, round_state(state), ctl, cfg)
        names.append(name)
    w.save(os.path.join(OUT, 'edge_steps.npz'))
    with open(os.path.join(OUT, 'edge_steps_names.json'), 'w') as f:
        json.dump(names, f, indent=1)


# ---------------------------------------------------------------------------
# 4. Free-running open-loop games (exact float64 trajectories)

def gen_games():
    """Whole games under open-loop controls: the full float64 ship trajectory,
    bullet counts, outcome.  A float64-storing implementation must reproduce
    these bit for bit; a float32-storing one statistically."""
    out = {}
    index = []
    plan = [('default', 'random', 24), ('default', 'nothing', 8), ('solo', 'random', 8),
            ('mp8', 'random', 12), ('rapid', 'random', 4), ('short', 'random', 6),
            ('solo_easy', 'nothing', 2)]
    gid = 0
    for cfg_name, policy, games in plan:
        base = CONFIGS[cfg_name]
        for g, config in enumerate(it.islice(core.generate_configs(base), 100, 100 + games)):
            nships = 1 if config.solo else 2
            rng = np.random.RandomState(5000 + gid)
            tmax = int(round(config.max_time / config.dt)) + 2
            if policy == 'random':
                ctl = rng.randint(0, 6, size=(tmax, nships))
            else:
                ctl = np.full((tmax, nships), 2)
            state = core.create(config)
            ships, nbul, planets = [], [], []
            tick = 0
            while True:
                sp, pp, _, _, _ = pack_state(state, nships)
                ships.append(sp)
                planets.append(pp)
                nbul.append(state.bullets.x.shape[0])
                state, reward = core.step(state, ctl[tick], config)
                tick += 1
                if state is None:
                    break
            rew = np.zeros(2)
            rew[:nships] = reward
            key = 'g%03d' % gid
            out[key + '__seed'] = np.uint32(config.seed)
            out[key + '__controls'] = ctl[:tick].astype(np.int8)
            out[key + '__ships'] = np.stack(ships)
            out[key + '__planets'] = np.stack(planets)
            out[key + '__nbullets'] = np.array(nbul, dtype=np.int32)
            out[key + '__reward'] = rew
            winner = None if np.max(reward) < 1 else int(np.argmax(reward))
            index.append(dict(gid=gid, cfg=cfg_name, policy=policy, seed=int(config.seed),
                              ticks=tick, winner=winner,
                              done=1 if reward.dtype.kind == 'i' else 2))
            gid += 1
    np.savez_compressed(os.path.join(OUT, 'games.npz'), **out)
    with open(os.path.join(OUT, 'games.json'), 'w') as f:
        json.dump(index, f, indent=0)
    print('wrote games.npz', gid, 'games')


# ---------------------------------------------------------------------------
# 5. Fire / timeout schedule, measured through the reference step

def gen_schedule():
    """Fire ticks and the timeout tick of several configs, observed from the
    reference step itself (a solo ship parked far from a massless planet, so
    nothing ever collides): fire <=> the bullet count grows."""
    sched = {}
    variants = {
        'default': {}, 'rapid': dict(reload_time=0.01), 'r005': dict(reload_time=0.05),
        'r007': dict(reload_time=0.07), 'r02': dict(reload_time=0.2),
        'short': dict(max_time=3.0, reload_time=0.05), 'mt1': dict(max_time=1.0),
        'dt003': dict(dt=0.03, max_time=7.0, reload_time=0.1),
        'never': dict(reload_time=1000.0, max_time=5.0),
    }
    for name, kw in variants.items():
        cfg = core.DEFAULT_CONFIG._replace(solo=True, planet_mass=0.0, **kw)
        B = core.Bodies
        state = core.State(
            ships=B(x=np.array([[0.9, 0.9]]), dx=np.zeros((1, 2)), b=np.array([0.785])),
            planets=B(x=np.zeros((1, 2)), dx=np.zeros((1, 2)), b=None),
            bullets=B(x=np.zeros((0, 2)), dx=np.zeros((0, 2)), b=None), reload=0.0, t=0.0)
        fires, tick = [], 0
        reloads, ts = [], []
        while True:
            nb = state.bullets.x.shape[0]
            reloads.append(state.reload)
            ts.append(state.t)
            nxt, reward = core.step(state, np.array([2]), cfg)
            if nxt is None:
                break
            # fire <=> reload was decremented by reload_time (core.py:263,280)
            new = nxt.reload != state.reload + cfg.dt
            if new:
                fires.append(tick)
            state = nxt
            tick += 1
        sched[name] = dict(config=dict(cfg._asdict()), fire_ticks=fires, timeout_tick=tick,
                           reload=reloads[:50], t=ts[:50], t_last=ts[-1])
    with open(os.path.join(OUT, 'schedule.json'), 'w') as f:
        json.dump(sched, f)
    print('wrote schedule.json')


# ---------------------------------------------------------------------------
# 6. Known-answer tests from the reference's own tests, as data

def gen_kats():
    kat = {}
    x = np.array([[0, 0], [1.9, 1.9], [3.8, 1.9], [3.8, 0.0]])
    r = np.array([1, 1, 2, 0])
    kat['collisions'] = dict(x=x.tolist(), r=r.tolist(),
                             out=core._collisions(x, r).tolist())  # test_core.py:6-17
    b = np.arange(0, 2 * np.pi + 1e-3, np.pi / 2)
    kat['direction'] = dict(b=b.tolist(), out=util.direction(b).tolist())  # test_util.py:59-64
    w = np.array([[1.01, -0.95], [0.95, -1.01]])
    kat['wrap_unit_square'] = dict(x=w.tolist(), out=util.wrap_unit_square(w).tolist())
    rng = np.random.RandomState(3)
    wx = np.concatenate([rng.uniform(-3, 3, 200), [-1, 1, -3, 3, 0, -1e-17, 1 - 1e-16, -1 + 1e-17]])
    kat['wrap_random'] = dict(x=wx.tolist(), out=util.wrap_unit_square(wx).tolist())
    bb = np.concatenate([rng.uniform(-300, 300, 2000), np.arange(-20, 20, 0.125)]).astype(np.float32)
    dd = util.direction(bb)
    kat['direction_f32'] = dict(b=bb.astype(np.float64).tolist(),
                                out_bits=dd.view(np.uint32).tolist())
    with open(os.path.join(OUT, 'kat.json'), 'w') as f:
        json.dump(kat, f)
    print('wrote kat.json')


# ---------------------------------------------------------------------------
# 6. Observation features: rl.ValueNetwork.get_features / to_batch
#    (rl.py:36-112) of every input state of steps.npz

def _import_rl():
    """astro/rl.py imports tensorboardX at module level for its training
    logger; it is absent here and unused by get_features/to_batch, so an empty
    placeholder module is registered before the import (nothing of rl.py's
    feature code is touched)."""
    sys.modules.setdefault('tensorboardX', types.ModuleType('tensorboardX'))
    from astro import rl  # noqa: E402
    return rl


def gen_features():
    rl = _import_rl()
    z = load_fixture('steps.npz')
    names = list(z['cfg_names'])
    feats, rows, dims = [], [], []
    for i in range(z['tick'].shape[0]):
        S = int(z['nships'][i])
        npl = int(z['nplanets'][i])
        fl = int(z['dtype_flags'][i])
        sh = z['in_ships'][i, :S]
        pl = z['in_planets'][i, :npl]
        off = z['in_bullets_off']
        bl = z['in_bullets'][off[i]:off[i + 1]]
        f32 = np.float32
        sdt = f32 if fl & 1 else np.float64
        B = core.Bodies
        state = core.State(
            ships=B(x=sh[:, 0:2].astype(sdt), dx=sh[:, 2:4].astype(sdt), b=sh[:, 4].astype(sdt)),
            planets=B(x=pl[:, 0:2].astype(f32 if fl & 2 else np.float64),
                      dx=pl[:, 2:4].astype(f32 if fl & 4 else np.float64), b=None),
            bullets=B(x=bl[:, 0:2].astype(f32 if fl & 8 else np.float64),
                      dx=bl[:, 2:4].astype(f32 if fl & 8 else np.float64), b=None),
            reload=0.0, t=0.0)
        f = rl.ValueNetwork.get_features(state)
        assert f.dtype == np.float32
        feats.append(f)
        rows.append(f.shape[0])
        dims.append(f.shape[1])
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    off[1:] = np.cumsum(rows)
    flat = np.zeros((int(off[-1]), 15), dtype=np.float32)
    for i, f in enumerate(feats):
        flat[off[i]:off[i + 1], :f.shape[1]] = f
    # to_batch of a few groups of same-ship-count states (ragged rows -> -1 padding)
    groups, batches = [], []
    for name in ('default', 'solo', 'rapid'):
        idx = [i for i in range(len(rows)) if names[z['cfg'][i]] == name][:40:5]
        b = rl.ValueNetwork.to_batch([feats[i] for i in idx])
        groups.append(np.array(idx, dtype=np.int64))
        batches.append(b)
    np.savez_compressed(os.path.join(OUT, 'features.npz'), features=flat, features_off=off,
                        dims=np.array(dims, dtype=np.int32),
                        **{'batch_idx_%d' % k: g for k, g in enumerate(groups)},
                        **{'batch_%d' % k: b for k, b in enumerate(batches)})
    print('wrote features.npz', len(rows), 'states', int(off[-1]), 'rows')


# ---------------------------------------------------------------------------
# 6b. Q values: rl.ValueNetwork.forward (rl.py:137-155) of every ship's ego
#     view of every input state of steps.npz, for one duo and one solo network

def _steps_state(z, i):
    """Input state i of steps.npz as a reference State (gen_features' rule)."""
    S = int(z['nships'][i])
    npl = int(z['nplanets'][i])
    fl = int(z['dtype_flags'][i])
    sh = z['in_ships'][i, :S]
    pl = z['in_planets'][i, :npl]
    off = z['in_bullets_off']
    bl = z['in_bullets'][off[i]:off[i + 1]]
    f32 = np.float32
    sdt = f32 if fl & 1 else np.float64
    bdt = f32 if fl & 8 else np.float64
    B = core.Bodies
    return core.State(
        ships=B(x=sh[:, 0:2].astype(sdt), dx=sh[:, 2:4].astype(sdt), b=sh[:, 4].astype(sdt)),
        planets=B(x=pl[:, 0:2].astype(f32 if fl & 2 else np.float64),
                  dx=pl[:, 2:4].astype(f32 if fl & 4 else np.float64), b=None),
        bullets=B(x=bl[:, 0:2].astype(bdt), dx=bl[:, 2:4].astype(bdt), b=None),
        reload=0.0, t=0.0)


def _forward64(w, x):
    """ValueNetwork.forward of one state's features [rows, nf] in float64
    (w: state_dict name -> array)."""
    softsign = lambda a: a / (1.0 + np.abs(a))  # noqa: E731
    lin = lambda a, k: a @ w[k + '.weight'].astype(np.float64).T + w[k + '.bias'].astype(np.float64)  # noqa: E731
    h = lin(x.astype(np.float64), 'f0')
    for k in ('f.0', 'f.1'):
        h = lin(softsign(h), k)
    v = h.max(0)
    for k in ('v.0', 'v.1'):
        v = softsign(lin(v, k))
    return np.tanh(lin(v, 'v0'))


def gen_qnet():
    import torch
    rl = _import_rl()
    z = load_fixture('steps.npz')
    n = z['tick'].shape[0]
    out = dict(torch=np.array(torch.__version__), numpy=np.array(np.__version__))
    nets = {}
    for solo in (False, True):
        torch.manual_seed(7)
        net = rl.ValueNetwork(solo, 6)
        with torch.no_grad():
            for p in net.parameters():
                p.mul_(3.0)
        name = 'solo' if solo else 'duo'
        w = {k: v.numpy().copy() for k, v in net.state_dict().items()}
        for k, v in w.items():
            assert v.dtype == np.float32
            out['%s__%s' % (name, k)] = v
        nets[name] = (net, w)
    q32 = np.zeros((n, 2, 6), dtype=np.float32)
    q64 = np.zeros((n, 2, 6), dtype=np.float64)
    err = dict(duo=0.0, solo=0.0)
    for i in range(n):
        S = int(z['nships'][i])
        name = 'solo' if S == 1 else 'duo'
        net, w = nets[name]
        state = _steps_state(z, i)
        for s in range(S):
            ego = core.roll_ships(state, s)
            with torch.no_grad():
                a = net.evaluate(ego).data.numpy()
            b = _forward64(w, rl.ValueNetwork.get_features(ego))
            assert a.dtype == np.float32 and a.shape == (6,)
            q32[i, s], q64[i, s] = a, b
            err[name] = max(err[name], float(np.abs(a.astype(np.float64) - b).max()))
    out.update(q32=q32, q64=q64, e_ref_duo=np.float64(err['duo']), e_ref_solo=np.float64(err['solo']))
    np.savez_compressed(os.path.join(OUT, 'qnet.npz'), **out)
    print('wrote qnet.npz', n, 'states, e_ref', err)


# ---------------------------------------------------------------------------
# 7. A game log written by the reference (core.save_log, core.py:413-426)

def gen_log():
    config = CONFIGS['short']
    game = core.play(config, [script.NothingBot(), script.NothingBot()])
    import gzip
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 'log.jsonl')
        core.save_log(path, game)
        data = open(path, 'rb').read()
    with gzip.GzipFile(os.path.join(OUT, 'log_short_nothing.jsonl.gz'), 'wb', mtime=0) as f:
        f.write(data)
    print('wrote log_short_nothing.jsonl.gz', len(game.ticks), 'ticks, winner', game.winner)


# ---------------------------------------------------------------------------
# 8. ScriptBot decisions (script.py:13-83) on every input state of steps.npz,
#    for each ship's ego view (core.roll_ships, core.py:306-327)

def gen_script_controls():
    z = load_fixture('steps.npz')
    names = list(z['cfg_names'])
    out = np.full((z['tick'].shape[0], S_PAD), -1, dtype=np.int8)
    bots = {}
    for i in range(z['tick'].shape[0]):
        name = names[z['cfg'][i]]
        config = CONFIGS[name]
        if name not in bots:
            bots[name] = script.ScriptBot.create(config)
        S = int(z['nships'][i])
        npl = int(z['nplanets'][i])
        fl = int(z['dtype_flags'][i])
        sh = z['in_ships'][i, :S]
        pl = z['in_planets'][i, :npl]
        off = z['in_bullets_off']
        bl = z['in_bullets'][off[i]:off[i + 1]]
        f32 = np.float32
        sdt = f32 if fl & 1 else np.float64
        B = core.Bodies
        state = core.State(
            ships=B(x=sh[:, 0:2].astype(sdt), dx=sh[:, 2:4].astype(sdt), b=sh[:, 4].astype(sdt)),
            planets=B(x=pl[:, 0:2].astype(f32 if fl & 2 else np.float64),
                      dx=pl[:, 2:4].astype(f32 if fl & 4 else np.float64), b=None),
            bullets=B(x=bl[:, 0:2].astype(f32 if fl & 8 else np.float64),
                      dx=bl[:, 2:4].astype(f32 if fl & 8 else np.float64), b=None),
            reload=0.0, t=0.0)
        for k in range(S):
            out[i, k] = bots[name](core.roll_ships(state, k))
    np.savez_compressed(os.path.join(OUT, 'script_controls.npz'), control=out)
    print('wrote script_controls.npz', out.shape[0], 'states')


# ---------------------------------------------------------------------------
# 8b. ScriptBot with non-default arguments: its decision on every input state
#     of steps.npz, both ego views, for six (avoid_distance, avoid_threshold)
#     sets, and an eight-step ScriptBot.mutate chain (script.py:93-108)

SCRIPT_ARG_SETS = [(0.0, 0.45), (0.3, 0.45), (0.1, 0.05), (0.1, 1.5), (-0.1, 0.9), (0.2371, 0.3119)]


def gen_script_args():
    z = load_fixture('steps.npz')
    names = list(z['cfg_names'])
    n = z['tick'].shape[0]
    out = np.full((len(SCRIPT_ARG_SETS), n, S_PAD), -1, dtype=np.int8)
    for a, (distance, threshold) in enumerate(SCRIPT_ARG_SETS):
        args = dict(avoid_distance=distance, avoid_threshold=threshold)
        bots = {}
        for i in range(n):
            name = names[z['cfg'][i]]
            if name not in bots:
                bots[name] = script.ScriptBot.create(CONFIGS[name], args)
            state = _steps_state(z, i)
            for k in range(int(z['nships'][i])):
                out[a, i, k] = bots[name](core.roll_ships(state, k))
    random = np.random.RandomState(42)
    args = dict(script.ScriptBot.DEFAULT_ARGS)
    chain = [[args['avoid_distance'], args['avoid_threshold']]]
    for _ in range(8):
        args = script.ScriptBot.mutate(args, scale=0.05, random=random)
        chain.append([args['avoid_distance'], args['avoid_threshold']])
    save_npz_fixed(os.path.join(OUT, 'script_args.npz'),
                   dict(args=np.array(SCRIPT_ARG_SETS, dtype=np.float64), control=out,
                        mutate_chain=np.array(chain, dtype=np.float64), mutate_seed=np.array(42),
                        mutate_scale=np.array(0.05)))
    print('wrote script_args.npz', out.shape)


# ---------------------------------------------------------------------------
# 9. BASELINE.json config 1: DEFAULT_CONFIG (seed 42), 1000 ticks of
#    RandomState(0).randint(0, 6, (1000, 2)) controls, re-created on done

def gen_config1():
    config = core.DEFAULT_CONFIG
    ctl = np.random.RandomState(0).randint(0, 6, (1000, 2))
    state = core.create(config)
    ships, planets, npl, bl, boff, rew, done, gtick = [], [], [], [], [0], [], [], []
    g = 0
    for t in range(1000):
        sp, pp, n, b, _ = pack_state(state, 2)
        ships.append(sp)
        planets.append(pp)
        npl.append(n)
        bl.append(b)
        boff.append(boff[-1] + b.shape[0])
        gtick.append(g)
        state, reward = core.step(state, ctl[t], config)
        rew.append(np.asarray(reward, np.float64))
        if state is None:
            done.append(1 if reward.dtype.kind == 'i' else 2)
            state = core.create(config)
            g = 0
        else:
            done.append(0)
            g += 1
    np.savez_compressed(os.path.join(OUT, 'config1.npz'), control=ctl.astype(np.int8),
                        ships=np.stack(ships), planets=np.stack(planets), nplanets=np.array(npl, np.int32),
                        bullets=np.concatenate(bl).reshape(-1, 4), bullets_off=np.array(boff, np.int64),
                        reward=np.stack(rew), done=np.array(done, np.int8), game_tick=np.array(gtick, np.int32))
    print('wrote config1.npz', int(np.sum(np.array(done) > 0)), 'games ended')


# ---------------------------------------------------------------------------
# 10. Whole games to the end under the reference's own bots (core.play):
#     test_script's invariants (test/test_core.py:88-98, max_time=20) and
#     games that reach the full 3000-tick timeout (core.py:257-260)

def _record_play(key, config, bots, out, index, extra):
    game = core.play(config, bots)
    nships = 1 if config.solo else 2
    ctl = np.stack([t.control for t in game.ticks]).astype(np.int8)
    ships = np.stack([pack_state(t.state, nships)[0] for t in game.ticks])
    nbul = np.array([t.state.bullets.x.shape[0] for t in game.ticks], np.int32)
    reward = game.ticks[-1].reward
    rew = np.zeros(2)
    rew[:nships] = reward
    out[key + '__controls'] = ctl
    out[key + '__ships'] = ships
    out[key + '__nbullets'] = nbul
    out[key + '__reward'] = rew
    index.append(dict(key=key, config=dict(config._asdict()), ticks=len(game.ticks), winner=game.winner,
                      done=1 if reward.dtype.kind == 'i' else 2, **extra))
    return game


def gen_long_games():
    out, index = {}, {}
    rows = []
    # test_script (test_core.py:88-98)
    for k, config in enumerate(it.islice(core.generate_configs(core.SOLO_CONFIG._replace(max_time=20)), 3)):
        _record_play('script_solo%d' % k, config, [script.ScriptBot.create(config)], out, rows,
                     dict(bots=['script']))
    for k, config in enumerate(it.islice(core.generate_configs(core.DEFAULT_CONFIG._replace(max_time=20)), 3)):
        _record_play('nothing_script%d' % k, config, [script.NothingBot(), script.ScriptBot.create(config)],
                     out, rows, dict(bots=['nothing', 'script']))
    # a full-length game: the first SOLO game ScriptBot survives to the
    # 3000-tick timeout (no 1v1 ScriptBot game of the first 40 DEFAULT_CONFIG
    # configs lasts that long)
    for name, base, mk in [('solo_timeout', core.SOLO_CONFIG, lambda c: [script.ScriptBot.create(c)])]:
        for config in it.islice(core.generate_configs(base), 40):
            game = core.play(config, mk(config))
            if len(game.ticks) == 3000:
                _record_play(name, config, mk(config), out, rows,
                             dict(bots=['script'] * (1 if config.solo else 2)))
                break
        else:
            print('no', name, 'game found')
    index = rows
    np.savez_compressed(os.path.join(OUT, 'long_games.npz'), **out)
    with open(os.path.join(OUT, 'long_games.json'), 'w') as f:
        json.dump(index, f, indent=0)
    print('wrote long_games.npz', [(r['key'], r['ticks'], r['winner']) for r in index])


# ---------------------------------------------------------------------------
# 11. The learner's experience bookkeeping: rl.QBotTrainer's n-step flush
#     (rl.py:249-258, 303-328) through core.play, with the optimisation step
#     (_step) replaced by a no-op so that only the replay list is exercised

def gen_replay():
    import torch
    rl = _import_rl()
    n_steps, games = 7, 3
    config0 = CONFIGS['short']
    torch.manual_seed(7)
    net = rl.ValueNetwork(solo=False, nout=6)
    trainer = rl.QNetworkTrainer(net, writer=None)
    bots = [rl.QBotTrainer(trainer, seed=n) for n in range(2)]
    for b in bots:
        b.n_steps = n_steps
        b._step = lambda: None
    game_ticks, game_reward, game_winner = [], [], []
    start = [[0], [0]]
    for config in it.islice(core.generate_configs(config0), games):
        game = core.play(config, bots)
        game_ticks.append(len(game.ticks))
        game_reward.append(np.asarray(game.ticks[-1].reward, dtype=np.float64))
        game_winner.append(-1 if game.winner is None else game.winner)
        for s, b in enumerate(bots):
            assert not b._nstep_buffer and len(b._replay_buffer) == sum(game_ticks)
            start[s].append(len(b._replay_buffer))
    out = dict(n_steps=np.int32(n_steps), discount=np.float64(bots[0].discount),
               game_ticks=np.array(game_ticks, np.int32), game_reward=np.stack(game_reward),
               game_winner=np.array(game_winner, np.int32), config=np.array(json.dumps(dict(config0._asdict()))))
    for s, b in enumerate(bots):
        xps = b._replay_buffer
        game = np.zeros(len(xps), np.int32)
        tick = np.zeros(len(xps), np.int32)
        for g in range(games):
            game[start[s][g]:start[s][g + 1]] = g
            tick[start[s][g]:start[s][g + 1]] = np.arange(game_ticks[g])
        nxt = np.full(len(xps), -1, np.int64)
        for i, d in enumerate(xps):
            if d.new_state_f is None:
                continue
            hits = [j for j in range(start[s][game[i]], start[s][game[i] + 1])
                    if xps[j].state_f.shape == d.new_state_f.shape and np.array_equal(xps[j].state_f, d.new_state_f)]
            later = [j for j in hits if j > i]
            assert later, (s, i)
            nxt[i] = later[0]
        rows = np.array([d.state_f.shape[0] for d in xps], np.int64)
        off = np.zeros(len(xps) + 1, np.int64)
        off[1:] = np.cumsum(rows)
        p = 's%d_' % s
        out[p + 'game'], out[p + 'tick'] = game, tick
        out[p + 'action'] = np.array([d.action for d in xps], np.int8)
        out[p + 'reward'] = np.array([d.reward for d in xps], np.float64)
        out[p + 'discount'] = np.array([d.discount for d in xps], np.float64)
        out[p + 'terminal'] = np.array([d.new_state_f is None for d in xps], np.uint8)
        out[p + 'next'] = nxt
        out[p + 'state_f'] = np.concatenate([d.state_f for d in xps]).astype(np.float32)
        out[p + 'state_off'] = off
        assert all(d.state_f.dtype == np.float32 and np.isinf(d.loss) for d in xps)
    np.savez_compressed(os.path.join(OUT, 'replay.npz'), **out)
    print('wrote replay.npz', game_ticks, game_winner, [r.tolist() for r in game_reward])


# ---------------------------------------------------------------------------
# 14. rl.EpsilonGreedy (rl.py:10-29) as rl.QBotTrainer constructs it
#     (rl.py:235-238): counts of its two-state process, no program text

def gen_explore(seeds=8, ticks=200000, game=1500, dt=0.02):
    """The reference's own EpsilonGreedy(t_in=1.0, t_out=0.1, seed) called once
    per tick with state.t = tick * dt, the tick jumping back to 0 every ``game``
    ticks (a new game).  Per seed: the calls made with no policy held and with
    one held (t = 0 calls apart), the entries and exits among them, the
    histogram of entered controls, and the transitions on t = 0 calls."""
    rl = _import_rl()
    State = types.SimpleNamespace
    out = dict(out_ticks=[], entries=[], in_ticks=[], exits=[], hist=[], t0_ticks=[], t0_transitions=[])
    for seed in range(seeds):
        bot = rl.EpsilonGreedy(t_in=1.0, t_out=0.1, seed=seed)
        c = dict(out_ticks=0, entries=0, in_ticks=0, exits=0, t0_ticks=0, t0_transitions=0)
        hist = np.zeros(6, np.int64)
        for k in range(ticks):
            tick = k % game
            before = bot._policy
            after = bot(State(t=tick * dt))
            moved = (before is None) != (after is None)
            if tick == 0:
                c['t0_ticks'] += 1
                c['t0_transitions'] += int(moved)
                continue
            if before is None:
                c['out_ticks'] += 1
                if moved:
                    c['entries'] += 1
                    hist[int(after)] += 1
            else:
                assert after is None or after == before
                c['in_ticks'] += 1
                c['exits'] += int(moved)
        for k, v in c.items():
            out[k].append(v)
        out['hist'].append(hist)
    out = {k: np.array(v, np.int64) for k, v in out.items()}
    np.savez_compressed(os.path.join(OUT, 'explore.npz'), seeds=np.int32(seeds), ticks=np.int64(ticks),
                        game=np.int32(game), dt=np.float64(dt), t_in=np.float64(1.0), t_out=np.float64(0.1), **out)
    print('wrote explore.npz', {k: v.sum(0).tolist() for k, v in out.items()})


# ---------------------------------------------------------------------------
# 15. More than 8 planets: create, teacher-forced steps, ScriptBot decisions
#     and get_features at max_planets 11 and 16 (wide.npz, 16 planet slots).
#     These configs stay out of configs.json: sorted(configs.json) parametrises
#     tests that run with 8 planet slots.

WIDE_P_PAD = 16
WIDE_CONFIGS = {
    'mp11': core.DEFAULT_CONFIG._replace(max_planets=11),   # randint's rejection path above 8
    'mp16': core.DEFAULT_CONFIG._replace(max_planets=16),
    'mp16_solo': core.SOLO_CONFIG._replace(max_planets=16),
}


def save_npz_fixed(path, arrays):
    """np.savez_compressed with a fixed member date, so that the same arrays
    give the same bytes on every run (numpy stamps each member with the
    current time)."""
    import zipfile
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
        for key, val in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(val), allow_pickle=False)
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o600 << 16
            zf.writestr(info, buf.getvalue())


def _wide_create_seeds(base, per_count):
    """Seeds of generate_configs(base), the first per_count of each planet
    count 1..max_planets (create()'s first draw, core.py:90), in stream order."""
    mp = base.max_planets
    have = {k: 0 for k in range(1, mp + 1)}
    seeds = []
    for c in it.islice(core.generate_configs(base), 20000):
        n = int(np.random.RandomState(c.seed).randint(1, mp + 1))
        if have[n] < per_count:
            have[n] += 1
            seeds.append(c.seed)
        if all(v == per_count for v in have.values()):
            return seeds
    raise RuntimeError('not every planet count found')


def _wide_games(base, counts):
    """For each planet count of ``counts``, the next config of
    generate_configs(base) whose create() draws that many planets."""
    stream = core.generate_configs(base)
    for want in counts:
        for c in stream:
            if int(np.random.RandomState(c.seed).randint(1, base.max_planets + 1)) == want:
                yield c
                break


def _planet_collision(state, ctl, config):
    """True if core.step ends this state with a ship inside a planet's radius."""
    nxt, reward = core.step(state, ctl, config)
    if nxt is not None or reward.dtype.kind != 'i':
        return False
    d = state.ships.x[:, None, :].astype(np.float64) - state.planets.x[None, :, :].astype(np.float64)
    return bool(((d ** 2).sum(-1) < (config.ship_radius + config.planet_radius) ** 2).any())


def gen_wide():
    rl = _import_rl()
    out = dict(configs=np.array(json.dumps({k: dict(v._asdict()) for k, v in WIDE_CONFIGS.items()})),
               numpy=np.array(np.__version__))
    # create(): every planet count 1..max_planets, about 64 seeds per config
    for name, base in WIDE_CONFIGS.items():
        mp = base.max_planets
        seeds = _wide_create_seeds(base, -(-64 // mp))
        k = len(seeds)
        npl = np.zeros(k, dtype=np.int32)
        sx = np.zeros((k, S_PAD, 2), np.float32)
        sdx = np.zeros((k, S_PAD, 2), np.float32)
        sb = np.zeros((k, S_PAD), np.float32)
        px = np.zeros((k, WIDE_P_PAD, 2), np.float32)
        pdx = np.zeros((k, WIDE_P_PAD, 2), np.float64)
        first = np.zeros(k, dtype=np.uint32)
        for i, seed in enumerate(seeds):
            s = core.create(base._replace(seed=seed))
            n = s.ships.x.shape[0]
            assert s.ships.x.dtype == np.float32 and s.ships.b.dtype == np.float32
            npl[i] = s.planets.x.shape[0]
            sx[i, :n] = s.ships.x
            sdx[i, :n] = s.ships.dx
            sb[i, :n] = s.ships.b
            px[i, :npl[i]] = s.planets.x
            pdx[i, :npl[i]] = s.planets.dx
            first[i] = np.random.RandomState(seed).randint(0, 1 << 32, dtype=np.uint64)
        assert set(npl.tolist()) == set(range(1, mp + 1)), name
        if name == 'mp11':   # randint(1, 12): word & 15 until <= 10
            assert ((first & 15) > 10).sum() >= 3
        for key, val in dict(seed=np.array(seeds, dtype=np.uint32), first_word=first, nplanets=npl, ships_x=sx,
                             ships_dx=sdx, ships_b=sb, planets_x=px, planets_dx=pdx).items():
            out['%s__%s' % (name, key)] = val

    # teacher-forced transitions along reference games
    w = TransitionWriter(WIDE_CONFIGS, WIDE_P_PAD)
    plan = [
        # (config, policy, games, keep_every)
        ('mp11', 'random', 6, 12),
        ('mp11', 'script', 2, 24),
        ('mp16', 'random', 8, 12),
        ('mp16', 'script', 3, 24),
        ('mp16', 'nothing', 2, 16),
        ('mp16_solo', 'random', 4, 12),
        ('mp16_solo', 'script', 2, 48),
    ]
    planet_ends = 0
    for cfg_name, policy, games, keep in plan:
        base = WIDE_CONFIGS[cfg_name]
        # game g has the g-th planet count of this walk: full slots first, then down through the rest
        mp = base.max_planets
        counts = [mp, 9, mp - 1, 1, 12 if mp > 12 else 10, 5, mp, 3, 13 if mp > 12 else 8, 2, 10, 7, 14 if mp > 12 else 6, 4]
        for g, config in enumerate(_wide_games(base, counts[:games])):
            rng = np.random.RandomState(3000 + g)
            nships = 1 if config.solo else 2
            bots = [script.ScriptBot.create(config) for _ in range(nships)]
            state = core.create(config)
            tick = 0
            while state is not None and tick < 400:
                ctl = _controls(policy, rng, nships, state, bots)
                nb_before = state.bullets.x.shape[0]
                nxt, reward = core.step(state, ctl, config)
                interesting = (tick == 0 or nxt is None or nxt.bullets.x.shape[0] != nb_before)
                if interesting or tick % keep == 0:
                    rs = round_state(state)
                    w.add(cfg_name, tick, rs, ctl, config)
                    planet_ends += _planet_collision(rs, np.asarray(ctl), config)
                state = nxt
                tick += 1
    tr = w.arrays()
    assert planet_ends > 0 and (tr['tick'] == 0).any() and np.diff(tr['in_bullets_off']).max() > 0
    assert tr['nplanets'].max() == 16 and (tr['nplanets'][tr['cfg'] == 0] > 8).any()
    out.update(tr)

    # the reference ScriptBot's decision for every ship, and get_features, of every input state
    n = tr['tick'].shape[0]
    names = list(WIDE_CONFIGS)
    ctl = np.full((n, S_PAD), -1, dtype=np.int8)
    bots = {k: script.ScriptBot.create(v) for k, v in WIDE_CONFIGS.items()}
    feats = []
    for i in range(n):
        state = _steps_state(tr, i)
        for k in range(int(tr['nships'][i])):
            ctl[i, k] = bots[names[tr['cfg'][i]]](core.roll_ships(state, k))
        f = rl.ValueNetwork.get_features(state)
        assert f.dtype == np.float32
        feats.append(f)
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum([f.shape[0] for f in feats])
    flat = np.zeros((int(off[-1]), 15), dtype=np.float32)
    for i, f in enumerate(feats):
        flat[off[i]:off[i + 1], :f.shape[1]] = f
    out.update(script_control=ctl, features=flat, features_off=off,
               dims=np.array([f.shape[1] for f in feats], dtype=np.int32))
    save_npz_fixed(os.path.join(OUT, 'wide.npz'), out)
    print('wrote wide.npz', n, 'transitions,', planet_ends, 'end by a planet collision,', int(off[-1]),
          'feature rows,', os.path.getsize(os.path.join(OUT, 'wide.npz')), 'bytes')


# ---------------------------------------------------------------------------
# 16. Away from DEFAULT_CONFIG's world constants (world.npz): create,
#     teacher-forced steps, ScriptBot decisions with their margins, the fire
#     schedule and whole games under configs whose eleven physics constants are
#     all inexact in float32 and no power-of-two multiple of their defaults.
#     These configs stay out of configs.json, as the wide ones do.

WORLD_VALUES = dict(
    gravity=0.08, dt=0.03, bullet_speed=1.3, ship_thrust=0.7, ship_rspeed=3.3, ship_radius=0.03,
    planet_radius=0.17, planet_mass=1.3, planet_orbit=0.55, inner_ship_position=0.23, outer_ship_position=0.85)
_WORLD = core.DEFAULT_CONFIG._replace(reload_time=0.2, **WORLD_VALUES)
WORLD_CONFIGS = {
    'world': _WORLD,
    'world_mp8': _WORLD._replace(max_planets=8),
    'world_one': _WORLD._replace(max_planets=1),      # the planet stays float32 for ever
    'world_solo': _WORLD._replace(solo=True, reload_time=1000, max_planets=6),
    'world_rapid': _WORLD._replace(reload_time=0.02),  # fires at tick 0
}
WORLD_CONFIGS.update({'only_' + k: core.DEFAULT_CONFIG._replace(**{k: v}) for k, v in WORLD_VALUES.items()})
WORLD_FULL = ('world', 'world_mp8', 'world_one', 'world_solo', 'world_rapid')
WORLD_CREATE_ONLY = ('only_gravity', 'only_planet_mass', 'only_planet_orbit', 'only_inner_ship_position',
                     'only_outer_ship_position')
MARGIN_F64, MARGIN_F32, MARGIN_CAP = 1e-9, 1e-5, 0.01


def _record_create(out, name, base, seeds, p_pad):
    k = len(seeds)
    npl = np.zeros(k, dtype=np.int32)
    sx = np.zeros((k, S_PAD, 2), np.float32)
    sdx = np.zeros((k, S_PAD, 2), np.float32)
    sb = np.zeros((k, S_PAD), np.float32)
    px = np.zeros((k, p_pad, 2), np.float32)
    pdx = np.zeros((k, p_pad, 2), np.float64)
    for i, seed in enumerate(seeds):
        s = core.create(base._replace(seed=seed))
        n = s.ships.x.shape[0]
        assert s.ships.x.dtype == np.float32 and s.ships.b.dtype == np.float32 and s.planets.x.dtype == np.float32
        npl[i] = s.planets.x.shape[0]
        sx[i, :n] = s.ships.x
        sdx[i, :n] = s.ships.dx
        sb[i, :n] = s.ships.b
        px[i, :npl[i]] = s.planets.x
        pdx[i, :npl[i]] = s.planets.dx
    for key, val in dict(seed=np.array(seeds, dtype=np.uint32), nplanets=npl, ships_x=sx, ships_dx=sdx,
                         ships_b=sb, planets_x=px, planets_dx=pdx).items():
        out['%s__%s' % (name, key)] = val
    return npl, sx, px, pdx


def _script_margin(config, state):
    """The smallest distance of a quantity that script.py:30-91 compares from
    the threshold it is compared with, along the path ScriptBot takes on this
    ego view: det and -b + sqrt(det) against 0, distance against the reach,
    the turn against +-tolerance and its magnitude against pi."""
    args = script.ScriptBot.DEFAULT_ARGS
    found = [np.inf]

    def near(value, threshold):
        found.append(abs(float(value) - float(threshold)))

    def turn(target, tolerance):
        off = util.norm_angle(target - state.ships.b[0])
        near(off, -tolerance)
        near(off, tolerance)
        near(abs(off), np.pi)
        return float(np.nanmin(found))

    radius = config.planet_radius + config.ship_radius
    with np.errstate(all='ignore'):
        for i in range(state.planets.x.shape[0]):
            x = state.ships.x[0] - state.planets.x[i]
            dx = state.ships.dx[0] - state.planets.dx[i]
            lin = 2 * util.dot(util.norm(dx), x)
            det = lin ** 2 - 4 * (util.mag(x) ** 2 - (radius + args['avoid_distance']) ** 2)
            near(det, 0)
            if 0 < det:
                near(-lin + np.sqrt(det), 0)
                if 0 <= -lin + np.sqrt(det):
                    speed = util.mag(dx)
                    reach = (speed / config.ship_thrust
                             + config.ship_rspeed / abs(util.norm_angle(util.bearing(x) - lin))) * speed
                    near(-lin - np.sqrt(det), reach)
                    if -lin - np.sqrt(det) < reach:
                        return turn(util.bearing(x), args['avoid_threshold'])
        if config.solo:
            return float(np.nanmin(found))
        distance = util.mag(state.ships.x[1] - state.ships.x[0])
        forecast = state.ships.x[1] + distance / config.bullet_speed * (state.ships.dx[1] - state.ships.dx[0])
        return turn(util.bearing(forecast - state.ships.x[0]), config.ship_radius / distance)


def _ram(state):
    """Both ships turn to each other and thrust: the games that end ship on ship."""
    out = []
    for k in range(2):
        off = util.norm_angle(util.bearing(state.ships.x[1 - k] - state.ships.x[k]) - state.ships.b[k])
        out.append(1 if off < -0.1 else 5 if off > 0.1 else 3)
    return np.array(out)


def gen_world():
    out = dict(configs=np.array(json.dumps({k: dict(v._asdict()) for k, v in WORLD_CONFIGS.items()})),
               numpy=np.array(np.__version__))
    # create(): every planet count of the four world configs, 16 seeds of the single-field ones
    for name in ('world', 'world_mp8', 'world_one', 'world_solo'):
        base = WORLD_CONFIGS[name]
        mp = base.max_planets
        npl, sx, px, pdx = _record_create(out, name, base, _wide_create_seeds(base, -(-64 // mp)), P_PAD)
        assert set(npl.tolist()) == set(range(1, mp + 1)), name
        if mp > 1:
            # both ship arrangements of core.py:97-107 (ship 0 outer / inner) and both orbit directions
            outer0 = np.abs(sx[npl > 1, 0, 0]) == np.float32(base.outer_ship_position)
            spin = np.sign(px[npl > 1, 0, 0] * pdx[npl > 1, 0, 1] - px[npl > 1, 0, 1] * pdx[npl > 1, 0, 0])
            assert outer0.any() and not outer0.all() and set(spin.tolist()) == {-1.0, 1.0}, name
    for name in WORLD_CREATE_ONLY:
        base = WORLD_CONFIGS[name]
        _record_create(out, name, base, [c.seed for c in it.islice(core.generate_configs(base), 16)], P_PAD)

    # teacher-forced transitions along reference games
    w = TransitionWriter(WORLD_CONFIGS, P_PAD)
    plan = [
        # (config, policy, planet counts of the games, keep_every, last tick)
        ('world', 'random', [4, 1, 3, 2, 4, 3, 2], 8, 600),
        ('world', 'script', [4, 2, 3, 1], 10, 600),
        ('world', 'nothing', [3, 2], 12, 600),
        ('world', 'ram', [2, 3, 4, 2, 3, 4], 40, 600),
        ('world_mp8', 'random', [8, 1, 7, 2, 6, 3, 5, 4], 8, 600),
        ('world_mp8', 'script', [8, 5, 7, 6, 3, 2], 12, 600),
        ('world_mp8', 'nothing', [8, 4], 12, 600),
        ('world_one', 'random', [1, 1, 1], 8, 300),
        ('world_one', 'script', [1], 12, 300),
        ('world_one', 'nothing', [1], 12, 300),
        ('world_solo', 'random', [6, 1, 5, 2, 4, 3, 6, 3, 1, 5], 8, 600),
        ('world_solo', 'script', [6, 3], 40, 1 << 20),    # to the timeout
        ('world_solo', 'nothing', [2], 12, 600),
        ('world_rapid', 'random', [4, 1, 3, 2, 4, 3, 2, 1], 1, 13),
        ('world_rapid', 'script', [4, 3], 1, 13),
    ]
    for name in WORLD_CONFIGS:
        if name.startswith('only_'):
            mp = WORLD_CONFIGS[name].max_planets
            plan += [(name, 'random', [mp, 2], 8, 240), (name, 'script', [3, 4], 8, 240)]
    for cfg_name, policy, counts, keep, last in plan:
        base = WORLD_CONFIGS[cfg_name]
        for g, config in enumerate(_wide_games(base, counts)):
            rng = np.random.RandomState(7000 + g)
            nships = 1 if config.solo else 2
            bots = [script.ScriptBot.create(config) for _ in range(nships)]
            state = core.create(config)
            tick = 0
            while state is not None and tick <= last:
                ctl = _ram(state) if policy == 'ram' else _controls(policy, rng, nships, state, bots)
                nb_before = state.bullets.x.shape[0]
                nxt, reward = core.step(state, ctl, config)
                interesting = (tick == 0 or nxt is None or nxt.bullets.x.shape[0] != nb_before)
                if interesting or tick % keep == 0:
                    w.add(cfg_name, tick, round_state(state), ctl, config)
                state = nxt
                tick += 1
    tr = w.arrays()
    n = tr['tick'].shape[0]
    names = list(WORLD_CONFIGS)

    # what the set is for (the events are told from the input states by the tests' own rule)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
    from tests.golden_io import world_events
    ev = world_events(tr, WORLD_CONFIGS)
    nin, nout = np.diff(tr['in_bullets_off']), np.diff(tr['out_bullets_off'])
    done = tr['out_done']
    full = np.isin(tr['cfg'], [names.index(k) for k in WORLD_FULL])
    rapid = tr['cfg'] == names.index('world_rapid')
    assert (full & (tr['tick'] == 0)).sum() >= 20
    assert (rapid & (tr['tick'] == 0) & (done == 0) & (nout > 0)).sum() >= 4, 'no fire at tick 0'
    assert (full & (nin > 0)).sum() > 200
    for what in ('ship_ship', 'ship_planet', 'ship_bullet'):
        assert (full & (done == 1) & ev[what]).any(), what
    assert (full & (done == 2)).any(), 'no timeout'
    assert (full & (done == 0) & ev['bullet_planet']).any() and (full & (done == 0) & ev['culled']).any()
    for k in WORLD_FULL:
        got = set(tr['nplanets'][tr['cfg'] == names.index(k)].tolist())
        assert got == set(range(1, WORLD_CONFIGS[k].max_planets + 1)), (k, got)
    per = np.bincount(tr['cfg'], minlength=len(names))
    assert 1300 <= per[:len(WORLD_FULL)].sum() <= 1700 and (per[len(WORLD_FULL):] >= 40).all(), per
    assert (per[len(WORLD_FULL):] <= 100).all(), per
    for key in ('in_ships', 'in_planets', 'in_bullets'):   # float32 values (round_state): stored as such
        assert np.array_equal(tr[key].astype(np.float32).astype(np.float64), tr[key])
        tr[key] = tr[key].astype(np.float32)
    out.update(tr)

    # the reference ScriptBot's decision for every ship of every input state; -2 where its margin is too small
    ctl = np.full((n, S_PAD), -1, dtype=np.int8)
    margin = np.full((n, S_PAD), np.inf)
    bots = {k: script.ScriptBot.create(v) for k, v in WORLD_CONFIGS.items()}
    for i in range(n):
        state = _steps_state(tr, i)
        cfg = WORLD_CONFIGS[names[tr['cfg'][i]]]
        for k in range(int(tr['nships'][i])):
            ego = core.roll_ships(state, k)
            ctl[i, k] = bots[names[tr['cfg'][i]]](ego)
            margin[i, k] = _script_margin(cfg, ego)
    limit = np.where(tr['tick'] == 0, MARGIN_F32, MARGIN_F64)[:, None]
    drop = (ctl >= 0) & (margin < limit)
    decisions = int((ctl >= 0).sum())
    assert drop.sum() <= MARGIN_CAP * decisions, (int(drop.sum()), decisions)
    ctl[drop] = -2
    out.update(script_control=ctl, script_dropped=np.int64(drop.sum()),
               script_margin_min=np.float64(margin[(ctl >= 0)].min()))

    # fire ticks and the timeout tick, gen_schedule's way: fire <=> reload was decremented
    for name, base in WORLD_CONFIGS.items():
        cfg = base._replace(solo=True, planet_mass=0.0)
        B = core.Bodies
        state = core.State(
            ships=B(x=np.array([[0.9, 0.9]]), dx=np.zeros((1, 2)), b=np.array([0.785])),
            planets=B(x=np.zeros((1, 2)), dx=np.zeros((1, 2)), b=None),
            bullets=B(x=np.zeros((0, 2)), dx=np.zeros((0, 2)), b=None), reload=0.0, t=0.0)
        fires, tick = [], 0
        while True:
            nxt, reward = core.step(state, np.array([2]), cfg)
            if nxt is None:
                break
            if nxt.reload != state.reload + cfg.dt:
                fires.append(tick)
            state = nxt
            tick += 1
        out[name + '__fire_ticks'] = np.array(fires, dtype=np.int32)
        out[name + '__timeout_tick'] = np.int32(tick)

    # three whole free-running games per world config (gen_games' record)
    index = []
    for cfg_name in WORLD_FULL:
        base = WORLD_CONFIGS[cfg_name]
        for g, config in enumerate(it.islice(core.generate_configs(base), 200, 203)):
            nships = 1 if config.solo else 2
            tmax = int(round(config.max_time / config.dt)) + 2
            ctl_g = np.random.RandomState(9000 + len(index)).randint(0, 6, size=(tmax, nships))
            state = core.create(config)
            ships, nbul, planets = [], [], []
            tick = 0
            while state is not None:
                sp, pp, _, _, _ = pack_state(state, nships)
                ships.append(sp)
                planets.append(pp)
                nbul.append(state.bullets.x.shape[0])
                state, reward = core.step(state, ctl_g[tick], config)
                tick += 1
            rew = np.zeros(2)
            rew[:nships] = reward
            key = 'game_%s_%d' % (cfg_name, g)
            out[key + '__seed'] = np.uint32(config.seed)
            out[key + '__controls'] = ctl_g[:tick].astype(np.int8)
            out[key + '__ships'] = np.stack(ships)
            out[key + '__planets'] = np.stack(planets)
            out[key + '__nbullets'] = np.array(nbul, dtype=np.int32)
            out[key + '__reward'] = rew
            out[key + '__done'] = np.int8(1 if reward.dtype.kind == 'i' else 2)
            index.append((key, tick))
    path = os.path.join(OUT, 'world.npz')
    save_npz_fixed(path, out)
    size = os.path.getsize(path)
    assert size < PART_BYTES, size
    print('wrote world.npz', n, 'transitions', per.tolist(), 'decisions', decisions, 'dropped', int(drop.sum()),
          'smallest kept margin %.3g' % margin[ctl >= 0].min(), 'games', index, size, 'bytes')
    print({k: int((full & v).sum()) for k, v in ev.items()}, 'timeouts', int((full & (done == 2)).sum()))


def generate():
    if sys.argv[1:] == ['world']:
        gen_world()
        return
    if sys.argv[1:] == ['wide']:
        gen_wide()
        return
    if sys.argv[1:] == ['explore']:
        gen_explore()
        return
    if sys.argv[1:] == ['replay']:
        gen_replay()
        return
    if sys.argv[1:] == ['config1']:
        gen_config1()
        return
    if sys.argv[1:] == ['long']:
        gen_long_games()
        return
    if sys.argv[1:] == ['script']:
        gen_script_controls()
        return
    if sys.argv[1:] == ['script_args']:
        gen_script_args()
        return
    if sys.argv[1:] == ['features']:
        gen_features()
        return
    if sys.argv[1:] == ['qnet']:
        gen_qnet()
        return
    if sys.argv[1:] == ['log']:
        gen_log()
        return
    os.makedirs(OUT, exist_ok=True)
    np.random.seed(0)
    with open(os.path.join(OUT, 'configs.json'), 'w') as f:
        json.dump(dict(configs=cfg_json(), numpy=np.__version__), f, indent=1)
    gen_kats()
    gen_schedule()
    gen_create()
    gen_edges()
    gen_steps()
    gen_games()
    gen_features()
    gen_qnet()
    gen_log()
    gen_script_controls()
    gen_script_args()
    gen_config1()
    gen_long_games()
    gen_replay()
    gen_explore()
    gen_wide()
    gen_world()


# No committed file may exceed 1 MiB: a larger fixture is stored as consecutive
# byte ranges name.00, name.01, ... (tests/golden_io.py: load joins them).
PART_BYTES = 1000000


def fixture_parts(name):
    return sorted(os.path.join(OUT, f) for f in os.listdir(OUT)
                  if f.startswith(name + '.') and f[len(name) + 1:].isdigit())


def load_fixture(name):
    path = os.path.join(OUT, name)
    if os.path.exists(path):
        return np.load(path)
    data = b''
    for f in fixture_parts(name):
        with open(f, 'rb') as fh:
            data += fh.read()
    return np.load(io.BytesIO(data))


def split_large():
    for name in sorted(os.listdir(OUT)):
        path = os.path.join(OUT, name)
        if name.endswith('.npz') and os.path.getsize(path) > PART_BYTES:
            for f in fixture_parts(name):
                os.remove(f)
            with open(path, 'rb') as fh:
                data = fh.read()
            for k in range(0, len(data), PART_BYTES):
                with open('%s.%02d' % (path, k // PART_BYTES), 'wb') as fh:
                    fh.write(data[k:k + PART_BYTES])
            os.remove(path)
            print('split', name, 'into', -(-len(data) // PART_BYTES), 'parts')


def main():
    generate()
    split_large()


if __name__ == '__main__':
    main()
