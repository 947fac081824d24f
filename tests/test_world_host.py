"""The world-parameter axis on the CPU: tests/golden/world.npz (written by
tools/gen_golden.py from the reference itself) holds create, teacher-forced
steps, ScriptBot decisions, fire schedules and whole games of configs whose
eleven physics constants all differ from DEFAULT_CONFIG's, by values that are
inexact in float32 and no power-of-two multiple of the default -- so that a
dropped factor, a swapped constant or a constant applied in the wrong precision
shows.  Here

  * the fixture holds what it is for;
  * the CPU oracle (oracle.batched, oracle.port), the host schedule, the host
    reduction schedule.kernel_constants and the host ScriptBot are pinned to it
    bit for bit: tests/test_gpu_world.py compares the kernels with the fixture
    and, closed loop, with this oracle;
  * the fixture can see each constant: the oracle with one constant put back to
    its default, or applied in float64 where the reference applies float32(c),
    disagrees with it.

Everything here runs on the CPU ("not gpu")."""
import dataclasses

import numpy as np
import pytest

from astro_amd import bots, schedule
from astro_amd.config import DEFAULT_CONFIG
from astro_amd.core import roll_ships
from oracle import batched, port
from tests import golden_io as gio
from tests.test_oracle_golden import _compare, _state_from_row

F32, F64 = np.float32, np.float64
WORLD = gio.world_configs()
FIELDS = gio.WORLD_FIELDS
ONLY = ['only_' + f for f in FIELDS]
MARGIN_CAP = 0.01   # at most this share of the decisions may be marked -2 (margin too small)


@pytest.fixture(scope='module')
def tr():
    return gio.Transitions('world.npz')


@pytest.fixture(scope='module')
def z():
    return gio.load('world.npz')


# ------------------------------------------------------------------ the fixture

def test_world_configs_are_what_the_axis_needs():
    """Every constant of ``world`` differs from the default, is inexact in
    float32 and no power-of-two multiple of the default; every only_ config
    changes exactly its field, to world's value."""
    assert list(WORLD) == list(gio.WORLD_FULL) + ONLY
    w = WORLD['world']
    for f in FIELDS:
        v, d = getattr(w, f), getattr(DEFAULT_CONFIG, f)
        assert v != d and float(F32(v)) != v, f
        assert np.frexp(v / d)[0] != 0.5, f
        assert WORLD['only_' + f] == DEFAULT_CONFIG._replace(**{f: v}), f
    assert float(F32(w.gravity * w.planet_mass)) != w.gravity * w.planet_mass
    assert w == DEFAULT_CONFIG._replace(reload_time=0.2, **{f: getattr(w, f) for f in FIELDS})
    assert WORLD['world_mp8'] == w._replace(max_planets=8)
    assert WORLD['world_one'] == w._replace(max_planets=1)
    assert WORLD['world_solo'] == w._replace(solo=True, reload_time=1000, max_planets=6)
    assert WORLD['world_rapid'] == w._replace(reload_time=0.02)


def test_world_fixture_covers_what_it_is_for(tr, z):
    names = tr.cfg_names
    assert names == list(WORLD)
    cfg, tick, done = tr.z['cfg'], tr.z['tick'], tr.z['out_done']
    nin, nout = np.diff(tr.z['in_bullets_off']), np.diff(tr.z['out_bullets_off'])
    full = np.isin(cfg, [names.index(k) for k in gio.WORLD_FULL])
    per = np.bincount(cfg, minlength=len(names))
    assert 1300 <= per[:5].sum() <= 1700 and (per[5:] >= 40).all() and (per[5:] <= 100).all(), per
    ev = gio.world_events(tr.z, WORLD)
    assert (full & (tick == 0)).sum() >= 20
    rapid = cfg == names.index('world_rapid')
    assert (rapid & (tick == 0) & (done == 0) & (nout > 0)).sum() >= 4    # fires at tick 0
    assert (full & (nin > 0)).sum() > 200
    for what in ('ship_ship', 'ship_planet', 'ship_bullet'):
        assert (full & (done == 1) & ev[what]).any(), what
    assert (full & (done == 2)).any()
    assert (full & (done == 0) & ev['bullet_planet']).any() and (full & (done == 0) & ev['culled']).any()
    for k in gio.WORLD_FULL:
        assert set(tr.z['nplanets'][cfg == names.index(k)].tolist()) == set(range(1, WORLD[k].max_planets + 1)), k
    # input states are float32 values that keep the reference's dtypes (tests/test_gpu_bots.py's rule)
    from tests.test_gpu_bots import _dtype_rule_holds
    assert all(_dtype_rule_holds(tr, i) for i in range(tr.n))
    assert tr.z['in_ships'].dtype == F32 and tr.z['out_ships'].dtype == F64
    # create: every planet count, both ship arrangements of core.py:97-107, both orbit directions
    for k in ('world', 'world_mp8', 'world_one', 'world_solo'):
        npl, mp = z[k + '__nplanets'], WORLD[k].max_planets
        assert set(npl.tolist()) == set(range(1, mp + 1)) and 60 <= npl.size <= 70, k
        if mp > 1:
            many = npl > 1
            outer0 = np.abs(z[k + '__ships_x'][many, 0, 0]) == F32(WORLD[k].outer_ship_position)
            px, pdx = z[k + '__planets_x'][many, 0], z[k + '__planets_dx'][many, 0]
            spin = np.sign(px[:, 0] * pdx[:, 1] - px[:, 1] * pdx[:, 0])
            assert outer0.any() and not outer0.all() and set(spin.tolist()) == {-1.0, 1.0}, k
    for k in gio.WORLD_CREATED[4:]:
        assert z[k + '__seed'].size == 16 and (z[k + '__nplanets'] > 1).any(), k
    # ScriptBot decisions: one per ship, at most 1 % of them left out for their margin
    want = tr.z['script_control']
    ships = np.arange(2)[None, :] < tr.z['nships'][:, None]
    assert (want[~ships] == -1).all() and (want[ships] >= -2).all() and (want[ships] != -1).all()
    dropped = int((want == -2).sum())
    assert dropped == int(z['script_dropped']) <= MARGIN_CAP * ships.sum()
    assert set(want[ships & (want >= 0)].tolist()) == {0, 2, 3, 4}
    assert float(z['script_margin_min']) >= 1e-9
    # the whole games
    games = gio.world_games()
    assert len(games) == 15 and {int(g['done']) for g in games} <= {1, 2}
    assert all(g['ships'].shape[0] == g['controls'].shape[0] == g['nbullets'].size for g in games)


# -------------------------------------------------- the oracle against the fixture

def _assert_create(name, B, z, S):
    assert (B.nplanets == z[name + '__nplanets']).all()
    assert np.array_equal(B.ships[..., 0:2], z[name + '__ships_x'][:, :S].astype(F64)), name
    assert np.array_equal(B.ships[..., 2:4], z[name + '__ships_dx'][:, :S]), name
    assert np.array_equal(B.ships_b, z[name + '__ships_b'][:, :S].astype(F64)), name
    assert np.array_equal(B.planets[..., 0:2], z[name + '__planets_x'].astype(F64)), name
    assert np.array_equal(B.planets[..., 2:4], z[name + '__planets_dx']), name   # float64 in the reference
    assert (B.nbullets == 0).all() and (B.tick == 0).all()


@pytest.mark.parametrize('name', gio.WORLD_CREATED)
def test_create_world(name, z):
    P = batched.make_params(WORLD[name])
    B = batched.create(z[name + '__seed'], P, p_pad=8, b_cap=4, store='f64')
    _assert_create(name, B, z, P.nships)
    g = port.Game(WORLD[name])
    for k, seed in enumerate(z[name + '__seed']):
        s = g.create(int(seed))
        n = s.planets.x.shape[0]
        assert np.array_equal(s.ships.x, z[name + '__ships_x'][k, :g.ns]) and s.ships.x.dtype == F32
        assert np.array_equal(s.ships.b, z[name + '__ships_b'][k, :g.ns])
        assert np.array_equal(s.planets.x, z[name + '__planets_x'][k, :n])
        assert np.array_equal(s.planets.dx, z[name + '__planets_dx'][k, :n])


def _step_group(tr, idx, P):
    B = tr.batch_in(idx, P.nships)
    got, rew, done = batched.step(B, tr.z['control'][idx], P, store='f64')
    return got, rew, done, tr.expected(idx, P.nships, b_cap=B.bullets.shape[1])


def test_step_world_teacher_forced_bit_exact(tr):
    total = 0
    for name, idx in tr.groups():
        got, rew, done, (E, erew, edone) = _step_group(tr, idx, batched.make_params(WORLD[name]))
        _compare('world.npz/' + name, got, rew, done, E, erew, edone)
        total += idx.size
    assert total == tr.n and len(dict(tr.groups())) == len(WORLD)


def test_port_step_world_teacher_forced_bit_exact(tr):
    zz = tr.z
    for name, idx in tr.groups():
        cfg = WORLD[name]
        g = port.Game(cfg)
        S = g.ns
        _, _, ts, reloads = batched.schedule(cfg)
        for i in idx:
            k = int(zz['tick'][i])
            st = _state_from_row(tr, i, S)._replace(t=float(ts[k]), reload=float(reloads[k]))
            out, rew = g.step(st, zz['control'][i, :S].astype(np.int64))
            assert (out is None) == (zz['out_done'][i] != 0), (name, i)
            assert np.array_equal(rew, zz['out_reward'][i, :S]), (name, i)
            assert (rew.dtype.kind == 'i') == (zz['out_done'][i] == 1)
            if out is None:
                continue
            n = zz['nplanets'][i]
            off = zz['out_bullets_off']
            assert np.array_equal(out.ships.x, zz['out_ships'][i, :S, 0:2]), (name, i)
            assert np.array_equal(out.ships.dx, zz['out_ships'][i, :S, 2:4]), (name, i)
            assert np.array_equal(out.ships.b, zz['out_ships'][i, :S, 4]), (name, i)
            assert np.array_equal(out.planets.x, zz['out_planets'][i, :n, 0:2]), (name, i)
            assert np.array_equal(out.planets.dx, zz['out_planets'][i, :n, 2:4]), (name, i)
            assert np.array_equal(out.bullets.x, zz['out_bullets'][off[i]:off[i + 1], 0:2]), (name, i)
            assert np.array_equal(out.bullets.dx, zz['out_bullets'][off[i]:off[i + 1], 2:4]), (name, i)


def test_world_games_free_running_float64_bit_exact():
    for g in gio.world_games():
        cfg = WORLD[g['cfg']]
        P = batched.make_params(cfg)
        S = P.nships
        st = batched.create([g['seed']], P, p_pad=8, b_cap=256, store='f64')
        ticks = g['ships'].shape[0]
        for t in range(ticks):
            n = st.nplanets[0]
            assert np.array_equal(st.ships[0], g['ships'][t, :S, 0:4]), (g['gid'], t)
            assert np.array_equal(st.ships_b[0], g['ships'][t, :S, 4]), (g['gid'], t)
            assert np.array_equal(st.planets[0, :n], g['planets'][t, :n]), (g['gid'], t)
            assert st.nbullets[0] == g['nbullets'][t], (g['gid'], t)
            ctl = np.zeros((1, 2), np.int64)
            ctl[0, :S] = g['controls'][t]
            st, rew, done = batched.step(st, ctl, P, store='f64')
            assert (done[0] != 0) == (t == ticks - 1), (g['gid'], t)
        assert done[0] == g['done'] and not st.overflow.any(), g['gid']
        assert np.array_equal(rew[0], g['reward'][:S].astype(F32))


@pytest.mark.parametrize('name', list(WORLD))
def test_schedule_and_kernel_constants(name, z):
    """The fire ticks and the timeout tick (measured through the reference
    step) from both host schedules, and schedule.kernel_constants field by
    field against the oracle's make_params and the config."""
    cfg = WORLD[name]
    fire, tt, _, _ = batched.schedule(cfg)
    assert tt == int(z[name + '__timeout_tick']) and np.array_equal(np.nonzero(fire)[0], z[name + '__fire_ticks'])
    s = schedule.build(cfg)
    assert s.timeout_tick == tt and np.array_equal(s.fire, fire)
    bits = s.fire_bits()
    assert np.array_equal(np.nonzero((bits[:, None] >> np.arange(32, dtype=np.uint32)[None, :]).reshape(-1) & 1)[0],
                          z[name + '__fire_ticks'])
    k, P = schedule.kernel_constants(cfg), batched.make_params(cfg)
    for f in ('gm', 'db', 'r2_ss', 'r2_sp', 'r2_s0', 'r2_p0', 'timeout_reward', 'nships'):
        assert k[f] == getattr(P, f) and type(k[f]) is type(getattr(P, f)), f
    for f in ('spawn_off', 'bullet_speed'):     # float32 in the reference: the double holds that value
        assert type(k[f]) is float and k[f] == float(getattr(P, f)) and F32(k[f]) == getattr(P, f), f
    assert (k['dt'], k['thrust'], k['gravity'], k['planet_mass']) == (cfg.dt, cfg.ship_thrust, cfg.gravity,
                                                                      cfg.planet_mass)
    assert (k['outer_pos'], k['inner_pos'], k['planet_orbit']) == tuple(
        float(F32(v)) for v in (cfg.outer_ship_position, cfg.inner_ship_position, cfg.planet_orbit))
    assert (k['solo'], k['max_planets']) == (int(cfg.solo), cfg.max_planets)
    assert set(k) == {'gm', 'dt', 'db', 'thrust', 'r2_ss', 'r2_sp', 'r2_s0', 'r2_p0', 'gravity', 'planet_mass',
                      'spawn_off', 'bullet_speed', 'timeout_reward', 'outer_pos', 'inner_pos', 'planet_orbit',
                      'nships', 'solo', 'max_planets'}


# ----------------------------------------------------------------- host ScriptBot

def _decisions(tr, idx, bot, S):
    out = np.full((idx.size, 2), -1, np.int64)
    for r, i in enumerate(idx):
        st = _state_from_row(tr, i, S)
        for k in range(S):
            out[r, k] = bot(roll_ships(st, k))
    return out


def test_host_scriptbot_world_decisions_match_reference(tr):
    checked = 0
    for name, idx in tr.groups():
        S = 1 if WORLD[name].solo else 2
        got = _decisions(tr, idx, bots.ScriptBot.create(WORLD[name]), S)
        want = tr.z['script_control'][idx]
        kept = want >= 0
        assert np.array_equal(got[kept], want[kept]), name
        checked += int(kept.sum())
    assert checked > 3500


# ------------------------------------------------- the fixture can see each constant

def _oracle_disagrees(tr, z, P, create_of=None):
    """True if the oracle under params P (create under config create_of, default
    P.config) differs from the fixture on a create array or a transition of ``world``."""
    name = 'world'
    cfg = P.config if create_of is None else create_of
    B = batched.create(z[name + '__seed'], batched.make_params(cfg), p_pad=8, b_cap=4, store='f64')
    try:
        _assert_create(name, B, z, P.nships)
    except AssertionError:
        return True
    idx = dict(tr.groups())[name]
    got, rew, done, (E, erew, edone) = _step_group(tr, idx, P)
    try:
        _compare(name, got, rew, done, E, erew, edone)
    except AssertionError:
        return True
    return False


def test_unchanged_oracle_agrees(tr, z):
    assert not _oracle_disagrees(tr, z, batched.make_params(WORLD['world']))


@pytest.mark.parametrize('field', FIELDS)
def test_fixture_sees_constant_at_its_default(field, tr, z):
    cfg = WORLD['world']._replace(**{field: getattr(DEFAULT_CONFIG, field)})
    assert _oracle_disagrees(tr, z, batched.make_params(cfg))


def test_fixture_sees_each_constant_in_steps_alone(tr):
    """The constants step() reads, each put back to its default, on the ``world``
    transitions alone (no create): the step kernels' copies are all in view."""
    idx = dict(tr.groups())['world']
    for field in ('gravity', 'dt', 'bullet_speed', 'ship_thrust', 'ship_rspeed', 'ship_radius', 'planet_radius',
                  'planet_mass'):
        cfg = WORLD['world']._replace(**{field: getattr(DEFAULT_CONFIG, field)})
        got, rew, done, (E, erew, edone) = _step_group(tr, idx, batched.make_params(cfg))
        with pytest.raises(AssertionError):
            _compare(field, got, rew, done, E, erew, edone)


def test_fixture_sees_bullet_speed_applied_in_float64(tr, z):
    P = batched.make_params(WORLD['world'])
    wide = dataclasses.replace(P, bullet_speed=F64(P.config.bullet_speed))
    assert wide.bullet_speed != P.bullet_speed and _oracle_disagrees(tr, z, wide)


@pytest.mark.parametrize('field', ['planet_orbit', 'inner_ship_position', 'outer_ship_position'])
def test_fixture_sees_create_constant_applied_in_float64(field, z):
    """create() with the constant as the double c instead of float32(c): the
    values c scales are taken from the oracle's create at c = 1 (an exact
    scaling) and multiplied in float64."""
    cfg = WORLD['world']
    seeds = z['world__seed']
    mk = lambda c: batched.create(seeds, batched.make_params(c), p_pad=8, b_cap=4, store='f64')  # noqa: E731
    B, unit = mk(cfg), mk(cfg._replace(**{field: 1.0}))
    _assert_create('world', B, z, 2)
    scaled = False
    for arr in ('ships', 'planets'):
        a, u = getattr(B, arr), getattr(unit, arr)
        where = a != u                      # what the constant scales
        assert np.array_equal(a[where], (F32(getattr(cfg, field)) * u[where].astype(F32)).astype(F64))
        a[where] = getattr(cfg, field) * u[where]
        scaled |= bool(where.any())
    assert scaled
    with pytest.raises(AssertionError):
        _assert_create('world', B, z, 2)
    if field != 'outer_ship_position':      # (+-c: float32(c) either way)
        for arr in ('ships', 'planets'):    # float32 state would show it too: the rounded product differs
            a = getattr(B, arr)
            a[:] = a.astype(F32).astype(F64)
        with pytest.raises(AssertionError):
            _assert_create('world', B, z, 2)


def test_fixture_sees_tick0_gravity_in_float64(tr, z, monkeypatch):
    """gravity * planet_mass is applied as float32 on a game's first step
    (float32 positions, core.py:151): with that field evaluated in float64 the
    oracle leaves the fixture, on tick-0 transitions only."""
    inner = batched._gravity
    monkeypatch.setattr(batched, '_gravity', lambda T, *a: inner(F64, *a))
    idx = dict(tr.groups())['world']
    P = batched.make_params(WORLD['world'])
    got, rew, done, (E, erew, edone) = _step_group(tr, idx, P)
    t0 = tr.z['tick'][idx] == 0
    with pytest.raises(AssertionError):
        _compare('tick 0', got.take(t0), rew[t0], done[t0], E.take(t0), erew[t0], edone[t0])
    _compare('later', got.take(~t0), rew[~t0], done[~t0], E.take(~t0), erew[~t0], edone[~t0])


def test_fixture_sees_scriptbot_constants(tr):
    """The host bot built from DEFAULT_CONFIG decides differently on kept
    states of ``world``, and so does the bot with any one of the five
    constants ScriptBot reads at its default."""
    idx = dict(tr.groups())['world']
    want = tr.z['script_control'][idx]
    kept = want >= 0
    assert not np.array_equal(_decisions(tr, idx, bots.ScriptBot.create(DEFAULT_CONFIG), 2)[kept], want[kept])
    for field in ('bullet_speed', 'ship_thrust', 'ship_rspeed', 'ship_radius', 'planet_radius'):
        cfg = WORLD['world']._replace(**{field: getattr(DEFAULT_CONFIG, field)})
        got = _decisions(tr, idx, bots.ScriptBot.create(cfg), 2)
        assert not np.array_equal(got[kept], want[kept]), field
