"""The CPU oracle and the host ScriptBot above 8 planets, pinned bit for bit
to the reference (tests/golden/wide.npz: max_planets 11 and 16, one and two
ships, written by tools/gen_golden.py from the reference itself), and the
CPU-side checks of tests/test_gpu_planet_slots.py's helpers.

tests/test_oracle_golden.py pins the oracle up to 8 planets; the GPU tests of
9-16 planet slots compare against the oracle, so it is pinned there too.
Everything here runs on the CPU ("not gpu")."""
import types

import numpy as np
import pytest
import torch

from astro_amd import bots
from astro_amd.core import roll_ships
from oracle import batched, features
from tests import golden_io as gio
from tests import qnet_util as qu
from tests import test_gpu_planet_slots as slots
from tests.test_oracle_golden import _compare, _state_from_row

WIDE = gio.wide_configs()
NAMES = ['mp11', 'mp16', 'mp16_solo']


def test_wide_fixture_covers_what_it_is_for():
    z = gio.load('wide.npz')
    assert sorted(WIDE) == sorted(NAMES)
    assert (WIDE['mp11'].max_planets, WIDE['mp16'].max_planets, WIDE['mp16_solo'].max_planets) == (11, 16, 16)
    assert WIDE['mp16_solo'].solo and not WIDE['mp16'].solo
    for name in NAMES:
        assert set(z[name + '__nplanets'].tolist()) == set(range(1, WIDE[name].max_planets + 1))
        assert 60 <= z[name + '__seed'].size <= 70
    # randint(1, 12) masks a word with 15 and rejects 11..15 (create's first draw)
    assert ((z['mp11__first_word'] & 15) > 10).sum() >= 3
    tr = gio.Transitions('wide.npz')
    assert 200 <= tr.n <= 800 and tr.cfg_names == NAMES
    npl, tick, done = tr.z['nplanets'], tr.z['tick'], tr.z['out_done']
    assert npl.max() == 16 and (npl[tr.z['cfg'] == 0] > 8).any() and (npl == 1).any()
    assert (tick == 0).sum() >= 10 and np.diff(tr.z['in_bullets_off']).max() >= 8
    # steps that end by a ship inside a planet
    r2 = (WIDE['mp16'].ship_radius + WIDE['mp16'].planet_radius) ** 2
    d = tr.z['in_ships'][:, :, None, 0:2] - tr.z['in_planets'][:, None, :, 0:2]
    live = (np.arange(16)[None, None, :] < npl[:, None, None]) & (np.arange(2)[None, :, None] < tr.z['nships'][:, None, None])
    inside = (((d ** 2).sum(-1) < r2) & live).any((1, 2))
    assert ((done == 1) & inside).sum() >= 5 and (done == 0).sum() > 200


@pytest.mark.parametrize('name', NAMES)
def test_create_wide(name):
    z = gio.load('wide.npz')
    P = batched.make_params(WIDE[name])
    B = batched.create(z[name + '__seed'], P, p_pad=16, b_cap=4, store='f64')
    S = P.nships
    assert (B.nplanets == z[name + '__nplanets']).all()
    assert np.array_equal(B.ships[..., 0:2].astype(np.float32), z[name + '__ships_x'][:, :S])
    assert np.array_equal(B.ships[..., 2:4], z[name + '__ships_dx'][:, :S])
    assert np.array_equal(B.ships_b.astype(np.float32), z[name + '__ships_b'][:, :S])
    assert np.array_equal(B.planets[..., 0:2].astype(np.float32), z[name + '__planets_x'])
    assert np.array_equal(B.planets[..., 2:4], z[name + '__planets_dx'])   # float64 in the reference
    assert (B.nbullets == 0).all() and (B.tick == 0).all()


def test_step_wide_teacher_forced_bit_exact():
    tr = gio.Transitions('wide.npz')
    total = 0
    for name, idx in tr.groups():
        P = batched.make_params(WIDE[name])
        S = P.nships
        B = tr.batch_in(idx, S, p_pad=16)
        got, rew, done = batched.step(B, tr.z['control'][idx], P, store='f64')
        E, erew, edone = tr.expected(idx, S, p_pad=16, b_cap=B.bullets.shape[1])
        _compare('wide.npz/' + name, got, rew, done, E, erew, edone)
        total += idx.size
    assert total == tr.n


def test_features_wide_bit_exact():
    """oracle.features.batched (what astro_features is checked against) and
    get_features == the reference's get_features of every input state."""
    tr = gio.Transitions('wide.npz')
    fx = gio.Features('wide.npz')
    for name, idx in tr.groups():
        S = 1 if WIDE[name].solo else 2
        B = tr.batch_in(idx, S, p_pad=16)
        rows = 16 + B.bullets.shape[1]
        got = features.batched(B, S, rows)
        for r, i in enumerate(idx):
            want = fx.of(i)
            assert want.shape == (tr.z['nplanets'][i] + B.nbullets[r], 1 + 5 * S + 4)
            assert np.array_equal(got[r, :want.shape[0]].view(np.uint32), want.view(np.uint32)), (name, i)
            assert (got[r, want.shape[0]:] == -1).all()
            one = features.get_features(_state_from_row(tr, i, S))
            assert np.array_equal(one.view(np.uint32), want.view(np.uint32)), (name, i)


def test_scriptbot_wide_decisions_match_reference():
    tr = gio.Transitions('wide.npz')
    want = tr.z['script_control']
    made = {name: bots.ScriptBot.create(WIDE[name]) for name in NAMES}
    checked = 0
    for i in range(tr.n):
        name = tr.cfg_names[tr.z['cfg'][i]]
        S = int(tr.z['nships'][i])
        st = _state_from_row(tr, i, S)
        for k in range(S):
            assert made[name](roll_ships(st, k)) == want[i, k], (i, k)
        assert (want[i, S:] == -1).all()
        checked += S
    assert checked > 500 and len(set(want[want >= 0].tolist())) >= 4


# ---------------------------------------------------------------------------
# tests/test_gpu_planet_slots.py's helpers, on the CPU

@pytest.mark.parametrize('p_pad,solo', [(3, False), (16, False), (16, True)])
def test_qvalues_seed_decides(p_pad, solo):
    """test_gpu_planet_slots.test_qvalues' argmax rule may skip a decision
    whose top-2 gap is at most 2 tol, up to 10 % of them: on the oracle's run of
    the same games and controls (Q_SEED; the GPU test checks that its state
    is this run's) the float64 reference alone skips well under that, in both
    state formats."""
    S = 1 if solo else 2
    wts = qu.fixture()[0][qu.kind(S)]['weights']
    for store in ('f32', 'f64'):
        B = slots.live_oracle(p_pad, p_pad, slots.QN, solo, slots.Q_SEED, store)
        assert (B.nbullets > 0).sum() > slots.QN // 2 and B.nplanets.max() == p_pad and (B.tick == 0).any()
        q64, e_ref = qu.reference_of(wts, B, S)
        top = np.sort(q64, axis=-1)
        skipped = int(((top[..., -1] - top[..., -2]) <= 2.0 * 4.0 * e_ref).sum())
        assert skipped <= 0.03 * q64.shape[0] * S, (store, skipped)


def _short_env(p_pad, n, dtype):
    """What guard_planets needs of an env, its planets one slot short of p_pad."""
    return types.SimpleNamespace(planets=torch.zeros((p_pad - 1, n, 4), dtype=dtype),
                                 state=types.SimpleNamespace(planets=0))


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('p_pad', [2, 3, 7, 16])
def test_guard_catches_a_view_one_slot_short(p_pad, dtype):
    """The oracle's create() of p_pad slots stored, slot-major as the kernels
    do, at a planets view that has only p_pad - 1: the last slot lands in the
    guard after the view and assert_guard_intact fails; the same store into a
    full view passes, and a single changed element on either side fails."""
    n = slots.GUARD // 4    # one slot of n envs is exactly the guard's length
    cfg = slots._config(p_pad)
    want = batched.create(batched.stream_seeds(cfg.seed, 12 * n), batched.make_params(cfg), p_pad=p_pad, b_cap=1)
    want = want.take(np.argsort(-want.nplanets, kind='stable')[:n])    # the games with the most planets
    assert (want.nplanets == p_pad).any()
    flat = torch.from_numpy(np.ascontiguousarray(want.planets.transpose(1, 0, 2))).to(dtype).flatten()

    env = slots.guard_planets(_short_env(p_pad + 1, n, dtype))     # p_pad slots: room for all
    assert env.planets.data_ptr() % 32 == 0 and env.state.planets == env.planets.data_ptr()
    env.planet_guard[slots.GUARD:slots.GUARD + flat.numel()] = flat
    slots.assert_guard_intact(env)
    for k in (0, slots.GUARD - 1, slots.GUARD + flat.numel(), flat.numel() + 2 * slots.GUARD - 1):
        keep = env.planet_guard[k].clone()
        env.planet_guard[k] = 0.25
        with pytest.raises(AssertionError, match='guard elements'):
            slots.assert_guard_intact(env)
        env.planet_guard[k] = float('nan')      # another NaN than the guard's is a change too
        with pytest.raises(AssertionError, match='guard elements'):
            slots.assert_guard_intact(env)
        env.planet_guard.view(slots.GUARD_BITS[dtype][0])[k] = keep.view(slots.GUARD_BITS[dtype][0])
        slots.assert_guard_intact(env)

    short = slots.guard_planets(_short_env(p_pad, n, dtype))       # one slot short
    slots.assert_guard_intact(short)
    short.planet_guard[slots.GUARD:slots.GUARD + flat.numel()] = flat
    with pytest.raises(AssertionError, match='after the array'):
        slots.assert_guard_intact(short)
    # a read of the missing slot that is used: the guard's NaN reaches the comparison
    short = slots.guard_planets(_short_env(p_pad, n, dtype))
    short.planet_guard[slots.GUARD:slots.GUARD + flat.numel() - 4 * n] = flat[:-4 * n]
    read = short.planet_guard[slots.GUARD:slots.GUARD + flat.numel()].view(p_pad, n, 4).permute(1, 0, 2).numpy()
    live = np.arange(p_pad)[None, :] < want.nplanets[:, None]
    rnd = slots._rnd(dtype)
    assert not np.array_equal(read.astype(np.float64)[live], rnd(want.planets)[live])
    assert np.array_equal(read.astype(np.float64)[:, :p_pad - 1][live[:, :p_pad - 1]],
                          rnd(want.planets)[:, :p_pad - 1][live[:, :p_pad - 1]])
