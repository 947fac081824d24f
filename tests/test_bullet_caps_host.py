"""The designed bullet states of tests/bullet_util.py meet their conditions -- on the oracle alone.

tests/test_gpu_bullet_caps.py compares the kernels with these scenarios' trajectories; here each
scenario is shown to be what it claims (full waves at the packed maxima, the index-window geometry,
the kill patterns, the 16-bit ends, the ship hits), so that a GPU test cannot pass vacuously.  The
oracle's counts are checked against their definitions (include/astro_step.h), and batched.step's
results are the same with and without them.
"""
import numpy as np
import pytest

from oracle import batched
from tests import bullet_util as bu

QWIN = bu.QWIN


def _survivor_check(sc):
    """Step 0 keeps exactly the slots named SURVIVE, in slot order (the velocities a move leaves
    unchanged identify them), then the shots."""
    t = sc.ticks[0]
    fired = sc.P.nships if sc.P.fire[sc.start.tick[0]] else 0
    for i in np.nonzero(t.done == 0)[0]:
        nb = int(sc.start.nbullets[i])
        fate = np.zeros(nb, np.int64) if sc.fates is None else sc.fates[i]
        surv = fate == bu.SURVIVE
        want = min(int(surv.sum()) + fired, sc.b_cap)
        assert t.out.nbullets[i] == want, i
        m = min(int(surv.sum()), sc.b_cap)
        assert np.array_equal(t.out.bullets[i, :m, 2:4], sc.start.bullets[i, :nb][surv][:m, 2:4]), i


def test_counts_leave_the_step_unchanged_and_follow_their_definitions():
    sc = bu.hits()
    P = sc.P
    c = {}
    a = batched.step(sc.start, sc.ctl[0], P, store='f32')
    b = batched.step(sc.start, sc.ctl[0], P, store='f32', counts=c)
    for f in a[0].__dataclass_fields__:
        assert np.array_equal(getattr(a[0], f), getattr(b[0], f)), f
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    done = a[2]
    assert done.any() and not done.all()
    assert np.array_equal(c['bullets_in'], sc.start.nbullets)
    assert np.array_equal(c['planets'], sc.start.nplanets)
    assert np.array_equal(c['bullets_out'], np.where(done == 0, a[0].nbullets, 0))
    assert not c['bullets_out'][done != 0].any() and not c['overflows'][done != 0].any()
    assert np.array_equal(c['collisions'], done == 1) and np.array_equal(c['timeouts'], done == 2)
    # dropped = kept candidates beyond the capacity: the same step with S more slots keeps them
    th = bu.thresholds(1023, 'f32')
    t1 = th.ticks[1]
    S = P.nships
    wide = batched.Batch.zeros(th.n, S, bu.P_PAD, th.b_cap + S)
    for f in ('tick', 'nplanets', 'nbullets', 'ships', 'ships_b', 'planets'):
        getattr(wide, f)[:] = getattr(t1.state, f)
    wide.bullets[:, :th.b_cap] = t1.state.bullets
    w = batched.step(wide, th.ctl[1], P, store='f32')[0]
    assert np.array_equal(t1.counts['overflows'], w.nbullets - t1.out.nbullets)
    assert t1.counts['overflows'].sum() == S * bu.N_FULL


@pytest.mark.parametrize('store', ['f32', 'f64'])
@pytest.mark.parametrize('b_cap', bu.THRESHOLDS)
def test_threshold_states(b_cap, store):
    """64 full envs of survivors: the lane wave, the quad waves and the pair waves sum to b_cap times
    64, 16 and 32 -- at 1023, 4095 and 2047 the largest sums the packed counters hold (65,472, 65,520,
    65,504), one b_cap higher 65,536; nothing ends; the one firing step drops S shots per full env."""
    sc = bu.thresholds(b_cap, store)
    nb = sc.start.nbullets.astype(np.int64)
    assert sc.n == 77 and (nb[:64] == b_cap).all() and (nb[64:] < b_cap - sc.P.nships * len(sc.ticks)).all()
    assert sc.start.tick[0] > 0
    for wave, per in ((64, 1023), (16, 4095), (32, 2047)):
        sums = nb[:64].reshape(-1, wave).sum(1)
        if b_cap == per:
            assert (sums == per * wave).all() and per * wave < 65536 <= (per + 1) * wave
        if b_cap == per + 1:
            assert (sums == 65536).all()
    fire = [bool(sc.P.fire[t.state.tick[0]]) for t in sc.ticks]
    assert fire == [False, True, False, False]
    for k, t in enumerate(sc.ticks):
        assert not t.done.any()
        assert (t.out.nbullets[:64] == b_cap).all()        # every tick reads full waves
        assert t.counts['overflows'][:64].tolist() == [sc.P.nships * fire[k]] * 64
        assert not t.counts['overflows'][64:].any()
        assert t.out.overflow[:64].all() == (k >= 1) and not t.out.overflow[64:].any()
    tot = bu.totals(sc.ticks)
    assert tot['overflows'] == sc.P.nships * 64
    assert tot['bullets_in'] != tot['bullets_out']          # (the tail's kills and shots)
    assert sc.ticks[-1].out.overflow[:64].all() and not sc.ticks[-1].out.overflow[64:].any()
    _survivor_check(sc)
    if store == 'f32':
        for f in ('ships', 'ships_b', 'planets', 'bullets'):
            a = getattr(sc.start, f)
            assert np.array_equal(a, a.astype(np.float32).astype(np.float64)), f


def test_threshold_state_at_tick0():
    """The tick-0 variant (the rapid config: a shot at every tick, the first moved in float32)."""
    sc = bu.thresholds(1024, 'f32', True)
    assert (sc.start.tick == 0).all() and (sc.start.nbullets[:64] == 1024).all()
    assert all(sc.P.fire[t.state.tick[0]] for t in sc.ticks)
    assert bu.totals(sc.ticks)['overflows'] == sc.P.nships * 64 * len(sc.ticks)
    assert not any(t.done.any() for t in sc.ticks)
    _survivor_check(sc)


def test_window_geometry():
    """The first 32 envs' counts, numbered within a quad wave (16 envs) and a pair wave (32)."""
    nb = bu.geometry_counts()
    assert nb.size == 77 and nb.max() == bu.GEOM_BCAP == 4100
    for wave in (16, 32):
        off = bu.wave_offsets(nb, wave)[:wave]
        c = nb[:wave]
        end = off + c
        big = c > 0
        assert (big & (off > 0) & (off % QWIN == 0)).any()           # starts exactly on a window boundary
        assert (big & (end % QWIN == 0)).any()                       # ends exactly on one
        # a window wholly inside one env: no env starts or ends in it or on its edges
        inner = [(i, k) for i in range(wave) for k in range(int(end[-1]) // QWIN)
                 if off[i] < k * QWIN and end[i] > (k + 1) * QWIN]
        assert inner and any(c[i] >= 2049 + off[i] % QWIN for i, _ in inner)
        # ... and an env that is exactly two windows
        assert ((c == 2 * QWIN) & (off % QWIN == 0)).any()
        assert c[0] == 0 and c[-1] == 0                              # empty first and last in the wave
        assert any(c[i] == 0 and c[i - 1] >= QWIN and c[i + 1] >= QWIN for i in range(1, wave - 1))
        assert {1, 2, 3, 5} <= set(c.tolist())                       # idle lanes of the env's group
        assert (c > QWIN).sum() >= 3 and end[-1] > 8 * QWIN
    # the second quad wave numbers its envs from 0 again
    off = bu.wave_offsets(nb, 16)[16:32]
    c = nb[16:32]
    assert ((c > 0) & (off > 0) & (off % QWIN == 0)).any() and ((c > 0) & ((off + c) % QWIN == 0)).any()


@pytest.mark.parametrize('tick0', [False, True])
@pytest.mark.parametrize('pattern', bu.PATTERNS)
def test_window_patterns(pattern, tick0):
    """Each pattern kills the slots it names and keeps the others, in order; the run at another row
    stride (b_cap 4160) holds the same bullets."""
    sc = bu.geometry(pattern, tick0=tick0)
    nb = sc.start.nbullets.astype(np.int64)
    assert np.array_equal(nb, bu.geometry_counts())
    assert (sc.start.tick == 0).all() == tick0
    kills = bu.pattern_kills(pattern, nb, np.random.RandomState(len(pattern)))
    frac = sum(int(k.sum()) for k in kills) / nb.sum()
    if pattern == 'none':
        assert frac == 0
    elif pattern == 'all':
        assert frac == 1
    elif pattern == 'alternate':
        assert all(not (k[1:] & k[:-1]).any() and (k[1:] | k[:-1]).all() for k in kills if k.size > 1)
    elif pattern == 'first_last':
        assert all(k.sum() == min(k.size, 2) and k[0] and k[-1] for k in kills if k.size)
    elif pattern == 'window_edges':
        off = bu.wave_offsets(nb, 32)
        for i in (3, 9, 11):      # both sides of every boundary the env crosses, nothing else in between
            g = off[i] + np.arange(nb[i])
            assert np.array_equal(kills[i] & (g > 0), ((g % QWIN == 0) | (g % QWIN == QWIN - 1)) & (g > 0))
            assert kills[i].sum() >= 4
    else:
        assert 0.25 < frac < 0.35
    for i, k in enumerate(kills):
        assert np.array_equal(sc.fates[i] != bu.SURVIVE, k)
        assert not (sc.fates[i] == bu.SHIP).any()
        if k.sum() > 1:     # hits and culls both
            assert (sc.fates[i] == bu.PLANET).any() and (sc.fates[i] == bu.CULL).any()
    assert not any(t.done.any() for t in sc.ticks)
    _survivor_check(sc)
    other = bu.geometry(pattern, b_cap=bu.GEOM_BCAP + 60, tick0=tick0)
    assert np.array_equal(other.start.bullets[:, :bu.GEOM_BCAP], sc.start.bullets)
    same = np.ones(sc.n, bool)     # envs that have dropped no shot at 4,100 slots
    for a, b in zip(sc.ticks, other.ticks):
        same &= a.counts['overflows'] == 0
        assert np.array_equal(a.out.nbullets[same], b.out.nbullets[same])
        assert np.array_equal(a.out.bullets[same], b.out.bullets[same, :bu.GEOM_BCAP])
    assert bu.totals(other.ticks)['overflows'] == 0
    # at 4,100 slots a full env drops shots unless the pattern freed room for them: 'none' always
    # does; 'first_last' frees two slots, enough for the aged games' one volley, not for a volley
    # at every tick (tick 0, the rapid config)
    assert (bu.totals(sc.ticks)['overflows'] > 0) == (pattern == 'none' or (pattern == 'first_last' and tick0))


def test_ends_state():
    sc = bu.ends()
    assert sc.b_cap == 65535 and sc.start.nbullets.tolist() == [65535, 0, 65534, 1, 32768]
    fire = [bool(sc.P.fire[t.state.tick[0]]) for t in sc.ticks]
    assert fire == [False, True, False]
    assert sc.ticks[1].counts['overflows'].tolist() == [2, 0, 1, 0, 0]
    assert sc.ticks[-1].out.nbullets.tolist() == [65535, 2, 65535, 3, 32770]
    assert sc.ticks[-1].out.overflow.tolist() == [True, False, True, False, False]
    assert not any(t.done.any() for t in sc.ticks)
    _survivor_check(sc)


@pytest.mark.parametrize('store', ['f32', 'f64'])
def test_hit_states(store):
    """Item d's designed envs: the envs HIT_AT names end by the bullet on the named ship's old
    position -- no other cause: the same envs without that bullet go on -- with more than 2,048
    bullets in four of them, the bullet in the first, a middle and the last index window."""
    sc = bu.hits(store)
    t = sc.ticks[0]
    want_done = np.array([1 if i in bu.HIT_AT else 0 for i in range(sc.n)], np.uint8)
    assert np.array_equal(t.done, want_done)
    assert sum(1 for i in bu.HIT_AT if bu.HIT_NB[i] > 2048) >= 4
    for i, hits in bu.HIT_AT.items():
        ships = {s for _, s in hits}
        assert t.reward[i].tolist() == [-1.0 if s in ships else 1.0 for s in range(2)], i
    clean = sc.start.copy()
    for i, hits in bu.HIT_AT.items():
        for slot, _ in hits:
            clean.bullets[i, slot, 0:2] = 5.0     # far outside: culled, hits nothing
    assert not batched.step(clean, sc.ctl[0], sc.P, store=store)[2].any()
    assert t.counts['collisions'].sum() == len(bu.HIT_AT)
    # the oracle leaves a finished env as it was
    fin = t.done != 0
    for f in ('tick', 'nbullets', 'ships', 'ships_b', 'planets', 'bullets'):
        assert np.array_equal(getattr(t.out, f)[fin], getattr(sc.start, f)[fin]), f
    _survivor_check(sc)


@pytest.mark.parametrize('b_cap', [32, 33])
def test_resident_states(b_cap):
    sc = bu.resident(b_cap)
    assert (sc.start.nbullets == b_cap).all() and sc.n == 77
    if b_cap == 32:     # the resident rollout's windows hold 256 live bullets
        assert sc.start.nbullets[:16].sum() == 2 * 256 and sc.start.nbullets[:32].sum() == 4 * 256
    fire = [bool(sc.P.fire[t.state.tick[0]]) for t in sc.ticks]
    assert fire == [False, True, False, False]
    assert all((t.out.nbullets == b_cap).all() and not t.done.any() for t in sc.ticks)
    assert bu.totals(sc.ticks)['overflows'] == sc.P.nships * sc.n
    _survivor_check(sc)
