"""Hand-loaded bullet states for the bullet-capacity tests (tests/test_bullet_caps_host.py,
tests/test_gpu_bullet_caps.py), and the oracle's trajectory and counts from them.

A *scenario* is: a plausible start state (oracle.batched.create, then a few oracle ticks), every
env's bullets overwritten to a prescribed count with a prescribed fate per slot, the controls of
the next ticks, and the oracle's results for those ticks (state, reward, done and the per-env
counts of batched.step).  Everything is made on the host from fixed seeds, so the host test can
prove the designed conditions on the oracle alone and the GPU tests compare the kernels with the
very same trajectory.  Scenarios are cached: treat them as read-only.

Fates are decided on the OLD positions, as the reference does (core.py:241-251):

  SURVIVE  inside the arena, slow, outside every planet disc and away from both ships at every
           tick of the scenario (checked against the ships' and planets' own trajectories);
  PLANET   on a live planet's old position;
  SHIP     on a ship's old position (it ends the game);
  CULL     in the arena's corner farthest from the ships, leaving it on both axes this tick.
"""
import functools
from dataclasses import dataclass

import numpy as np

from oracle import batched
from tests import golden_io as gio

CFG = gio.configs()
SURVIVE, PLANET, SHIP, CULL = 0, 1, 2, 3
QWIN = 1024          # csrc/astro_kernels.hip: live bullets per LDS index window of the quad/pair kernels
COUNTERS = ('bullets_in', 'bullets_out', 'overflows', 'planets', 'collisions', 'timeouts')
P_PAD = 4


@functools.lru_cache(maxsize=None)
def params(name):
    return batched.make_params(CFG[name])


def first_fire(P):
    return int(np.nonzero(P.fire)[0][0])


@dataclass
class Base:
    """n envs of one config at the start tick, without bullets, and where their ships and planets
    are at each of the next ``ticks`` ticks (the old positions each step collides with)."""
    name: str
    store: str
    batch: object        # batched.Batch without bullets
    ctl: np.ndarray      # int8 [ticks, n, S]
    ships_xy: np.ndarray    # [ticks, n, S, 2]
    planets_xy: np.ndarray  # [ticks, n, P_PAD, 2]


@functools.lru_cache(maxsize=None)
def base(name, n, store, tick0, ticks, lead=1):
    """``tick0``: fresh games (create()'s float32 arrays; their first step runs in float32).
    Otherwise games aged by the oracle to ``lead`` ticks before the config's first shot, so that
    the scenario's step number ``lead`` fires.  Candidates whose game ends within the scenario, or
    whose shots at the firing tick are not both kept, are left out."""
    P = params(name)
    S = P.nships
    rng = np.random.RandomState(1000 + n + 7 * ticks + (1 if tick0 else 0))
    m = n + 24
    B = batched.create(np.arange(5000, 5000 + m, dtype=np.uint32), P, P_PAD, (ticks + 1) * S, store=store)
    ok = np.ones(m, bool)
    if not tick0:
        for _ in range(first_fire(P) - lead):
            B, _, done = batched.step(B, rng.randint(0, 6, size=(m, S)).astype(np.int8), P, store=store)
            ok &= done == 0
    ctl = rng.randint(0, 6, size=(ticks, m, S)).astype(np.int8)
    sxy, pxy = [], []
    X = B
    for t in range(ticks):
        sxy.append(X.ships[..., 0:2].copy())
        pxy.append(X.planets[..., 0:2].copy())
        fires = P.fire[X.tick[0]]
        before = X.nbullets.copy()
        X, _, done = batched.step(X, ctl[t], P, store=store)
        ok &= done == 0
        if fires:
            ok &= X.nbullets == before + S
    sel = np.nonzero(ok)[0][:n]
    assert sel.size == n, 'too few candidate games'
    assert len(set(B.tick[sel].tolist())) == 1
    return Base(name, store, B.take(sel), ctl[:, sel], np.stack(sxy)[:, sel], np.stack(pxy)[:, sel])


def _survivors(bs, i, count, rng):
    """``count`` (x, y, dx, dy) that no ship and no planet of env i reaches within the scenario."""
    P = params(bs.name)
    cfg = P.config
    T = bs.ctl.shape[0]
    npl = int(bs.batch.nplanets[i])
    out = np.zeros((0, 4))
    while out.shape[0] < count:
        m = int((count - out.shape[0]) * 1.6) + 16
        c = np.concatenate([rng.uniform(-0.93, 0.93, (m, 2)), rng.uniform(-0.05, 0.05, (m, 2))], 1)
        good = np.ones(m, bool)
        for t in range(T):
            xy = c[:, 0:2] + t * cfg.dt * c[:, 2:4]
            for s in range(P.nships):
                good &= ((xy - bs.ships_xy[t, i, s]) ** 2).sum(1) > (cfg.ship_radius + 0.03) ** 2
            for j in range(npl):
                good &= ((xy - bs.planets_xy[t, i, j]) ** 2).sum(1) > (cfg.planet_radius + 0.03) ** 2
        out = np.concatenate([out, c[good]])
    return out[:count]


def load(bs, b_cap, nb, fates, seed=0):
    """The base's batch with b_cap bullet slots, env i holding nb[i] bullets of fates[i][k]
    (fates: a list of int arrays, or None for all SURVIVE).  Values are float32-valued for the
    float32 store.  Slots past nb[i] hold a finite junk value the kernels must never use."""
    P = params(bs.name)
    n = bs.batch.tick.shape[0]
    nb = np.asarray(nb, np.int64)
    assert nb.shape == (n,) and nb.max() <= b_cap
    B = batched.Batch.zeros(n, P.nships, P_PAD, b_cap)
    for f in ('tick', 'nplanets', 'ships', 'ships_b', 'planets'):
        getattr(B, f)[:] = getattr(bs.batch, f)
    B.nbullets[:] = nb
    B.bullets[:] = 0.25    # dead slots: inside the arena, never to be read
    for i in range(n):
        c = int(nb[i])
        if c == 0:
            continue
        rng = np.random.RandomState(seed * 100003 + i)
        fate = np.zeros(c, np.int64) if fates is None else np.asarray(fates[i], np.int64)
        assert fate.shape == (c,)
        rows = np.zeros((c, 4))
        k = np.nonzero(fate == SURVIVE)[0]
        rows[k] = _survivors(bs, i, k.size, rng)
        k = np.nonzero(fate == PLANET)[0]
        npl = int(bs.batch.nplanets[i])
        rows[k, 0:2] = bs.planets_xy[0, i, k % npl] + rng.uniform(-0.01, 0.01, (k.size, 2))
        rows[k, 2:4] = rng.uniform(-0.05, 0.05, (k.size, 2))
        k = np.nonzero(fate == SHIP)[0]
        rows[k, 0:2] = bs.ships_xy[0, i, k % P.nships] + rng.uniform(-0.001, 0.001, (k.size, 2))
        rows[k, 2:4] = rng.uniform(-0.05, 0.05, (k.size, 2))
        k = np.nonzero(fate == CULL)[0]
        corners = np.array([[1, 1], [1, -1], [-1, 1], [-1, -1]], float)
        far = corners[np.argmax([min(((cr - s) ** 2).sum() for s in bs.ships_xy[0, i]) for cr in corners])]
        rows[k, 0:2] = far * rng.uniform(0.990, 0.999, (k.size, 1))
        rows[k, 2:4] = far * rng.uniform(1.0, 1.4, (k.size, 1))
        B.bullets[i, :c] = rows
    if bs.store == 'f32':
        B.bullets[:] = B.bullets.astype(np.float32).astype(np.float64)
    return B


@dataclass
class Tick:
    state: object       # Batch the step read
    out: object         # Batch after the step (finished envs: unchanged, or re-created by run(seeds=))
    reward: np.ndarray
    done: np.ndarray
    counts: dict        # batched.step's per-env counts, plus 'resets'


def run(B, ctl, P, store, seeds=None, games=None):
    """The oracle's ticks from B under ctl [T, n, S].  seeds [n, G] (auto-reset): a finished env
    becomes batched.create of its next seed (``games`` [n]: games played so far, updated in
    place); otherwise it keeps its input state, as the oracle leaves it."""
    out = []
    for t in range(ctl.shape[0]):
        c = {}
        nxt, rew, done = batched.step(B, ctl[t], P, store=store, counts=c)
        c['resets'] = np.zeros(done.shape, np.int64)
        if seeds is not None:
            fin = np.nonzero(done)[0]
            if fin.size:
                nxt.put(fin, batched.create(seeds[fin, games[fin]], P, B.planets.shape[1], B.bullets.shape[1],
                                            store=store))
                games[fin] += 1
                c['resets'][fin] = 1
        out.append(Tick(B, nxt, rew, done, c))
        B = nxt
    return out


def totals(ticks):
    """The library's stat_dict() after these ticks, as far as the oracle defines it."""
    tot = {k: int(sum(t.counts[k].sum() for t in ticks)) for k in COUNTERS + ('resets',)}
    tot['serial_resets'] = 0    # (max_planets a power of two: no rejected randint word)
    return tot


# ---------------------------------------------------------------------------
# the designed scenarios

@dataclass
class Scenario:
    name: str
    store: str
    b_cap: int
    start: object       # Batch
    ctl: np.ndarray
    ticks: list         # of Tick
    fates: list = None

    @property
    def P(self):
        return params(self.name)

    @property
    def n(self):
        return self.start.tick.shape[0]


N_FULL, N_THRESH = 64, 77
THRESHOLDS = (1023, 1024, 2047, 2048, 4095, 4096)


def tail_fates(c, rng):
    """A ragged env's fates: roughly a third of the slots hit a planet or leave."""
    f = np.zeros(c, np.int64)
    kill = rng.rand(c) < 0.3
    f[kill] = np.where(rng.rand(int(kill.sum())) < 0.5, PLANET, CULL)
    return f


@functools.lru_cache(maxsize=None)
def thresholds(b_cap, store, tick0=False, ticks=4):
    """Packing thresholds (issue item a): envs 0..63 full of survivors -- one lane wave, four quad
    waves, two pair waves, each summing to its kernel's packed maximum or just past it -- and 13
    ragged envs with room for the shots (no overflow there) and some kills.  Step 1 fires (the
    rapid config at tick 0: every step)."""
    name = 'rapid' if tick0 else 'default'
    bs = base(name, N_THRESH, store, tick0, ticks)
    P = params(name)
    rng = np.random.RandomState(b_cap)
    room = b_cap - ticks * P.nships - 2
    nb = np.full(N_THRESH, b_cap, np.int64)
    nb[N_FULL:] = [0, 1, room, room // 2, 3, 0, room, 5, 2, room - 1, 64, 65, 0]
    fates = [np.zeros(int(c), np.int64) for c in nb]
    for i in range(N_FULL, N_THRESH):
        fates[i] = tail_fates(int(nb[i]), rng)
    start = load(bs, b_cap, nb, fates, seed=b_cap)
    return Scenario(name, store, b_cap, start, bs.ctl, run(start, bs.ctl, P, store), fates)


# window geometry (issue item b): bullet counts of the first 32 envs -- quad waves 0 and 1, pair
# wave 0 -- see test_bullet_caps_host.py::test_window_geometry for the conditions they meet
GEOM_BCAP = 4100
GEOM_NB = (0, 1024, 0, 3100, 1, 2, 3, 5, 0, 4100, 981, 2048, 0, 0, 37, 0,
           0, 3, 4100, 0, 1017, 2100, 1, 0, 2, 0, 5, 0, 0, 700, 4099, 0)
GEOM_N = 77
PATTERNS = ('none', 'all', 'alternate', 'window_edges', 'first_last', 'random30')


def wave_offsets(nb, wave):
    """off[i]: number of env i's first bullet among its wave's live bullets (waves of ``wave`` envs)."""
    nb = np.asarray(nb, np.int64)
    off = np.zeros_like(nb)
    for w0 in range(0, nb.size, wave):
        c = np.cumsum(nb[w0:w0 + wave])
        off[w0:w0 + wave] = c - nb[w0:w0 + wave]
    return off


def pattern_kills(pattern, nb, rng):
    """bool [c] per env: the slots the pattern kills."""
    nb = np.asarray(nb, np.int64)
    offs = [wave_offsets(nb, 16), wave_offsets(nb, 32)]
    out = []
    for i, c in enumerate(nb.tolist()):
        k = np.arange(c)
        if pattern == 'none':
            kill = np.zeros(c, bool)
        elif pattern == 'all':
            kill = np.ones(c, bool)
        elif pattern == 'alternate':
            kill = (k + i) % 2 == 0
        elif pattern == 'window_edges':   # the last slot of a window and the first of the next, either numbering
            kill = np.zeros(c, bool)
            for off in offs:
                g = off[i] + k
                kill |= ((g > 0) & (g % QWIN == 0)) | (g % QWIN == QWIN - 1)
        elif pattern == 'first_last':
            kill = (k == 0) | (k == c - 1)
        elif pattern == 'random30':
            kill = rng.rand(c) < 0.3
        else:
            raise ValueError(pattern)
        out.append(kill)
    return out


def geometry_counts():
    rng = np.random.RandomState(41)
    return np.concatenate([GEOM_NB, rng.randint(0, 300, GEOM_N - len(GEOM_NB))]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def geometry(pattern, b_cap=GEOM_BCAP, store='f32', tick0=False, ticks=3):
    """Step 0 reads the designed counts and applies the kill pattern (killed slots alternate
    between a planet hit and a cull); step 1 fires.  The same bullets whatever b_cap >= 4100."""
    name = 'rapid' if tick0 else 'default'
    bs = base(name, GEOM_N, store, tick0, ticks)
    P = params(name)
    nb = geometry_counts()
    kills = pattern_kills(pattern, nb, np.random.RandomState(len(pattern)))
    fates = [np.where(kl, np.where(np.cumsum(kl) % 2 == 1, PLANET, CULL), SURVIVE) for kl in kills]
    start = load(bs, b_cap, nb, fates, seed=7)
    return Scenario(name, store, b_cap, start, bs.ctl, run(start, bs.ctl, P, store), fates)


ENDS_BCAP = 65535
ENDS_NB = (65535, 0, 65534, 1, 32768)


@functools.lru_cache(maxsize=None)
def ends(ticks=3):
    """The 16-bit ends (issue item c): float32, b_cap 65,535, all survivors, step 1 fires."""
    bs = base('default', len(ENDS_NB), 'f32', False, ticks)
    P = params('default')
    start = load(bs, ENDS_BCAP, ENDS_NB, None, seed=3)
    return Scenario('default', 'f32', ENDS_BCAP, start, bs.ctl, run(start, bs.ctl, P, 'f32'))


HIT_BCAP = 2100
HIT_NB = (2100, 0, 2077, 2049, 5, 2060, 300, 2100)
# env: (slot, ship) of its one SHIP bullet -- in the first, the last and a middle index window;
# env 5 has one on each ship
HIT_AT = {0: [(2075, 0)], 2: [(0, 1)], 3: [(2048, 0)], 5: [(1023, 0), (1024, 1)], 6: [(150, 1)]}


def hit_fates():
    rng = np.random.RandomState(9)
    fates = []
    for i, c in enumerate(HIT_NB):
        f = tail_fates(c, rng) if i % 2 else np.zeros(c, np.int64)
        for slot, ship in HIT_AT.get(i, ()):
            f[slot] = SHIP
        fates.append(f)
    return fates


def load_hits(bs, n_front=len(HIT_NB)):
    """The ``n_front`` designed envs of item d (a loaded game ends): bullets of HIT_NB/hit_fates on
    the base's first envs, each SHIP bullet on the ship HIT_AT names."""
    fates = hit_fates()
    B = load(bs, HIT_BCAP, HIT_NB, fates, seed=11)
    for i, hits in HIT_AT.items():
        for slot, ship in hits:
            B.bullets[i, slot, 0:2] = bs.ships_xy[0, i, ship]
    if bs.store == 'f32':
        B.bullets[:] = B.bullets.astype(np.float32).astype(np.float64)
    return B, fates


@functools.lru_cache(maxsize=None)
def hits(store='f32', ticks=3):
    """Item d without auto-reset: the oracle's ticks of the designed envs alone."""
    bs = base('default', len(HIT_NB), store, False, ticks)
    P = params('default')
    start, fates = load_hits(bs)
    return Scenario('default', store, HIT_BCAP, start, bs.ctl, run(start, bs.ctl, P, store), fates)


RES_N = 77


@functools.lru_cache(maxsize=None)
def resident(b_cap, ticks=4):
    """Item f: float32, every env full of survivors (b_cap 32: 512 bullets per quad wave, 1,024 per
    pair wave -- 2 and 4 windows of the resident rollout's 256), step 1 fires."""
    bs = base('default', RES_N, 'f32', False, ticks)
    P = params('default')
    start = load(bs, b_cap, np.full(RES_N, b_cap), None, seed=b_cap)
    return Scenario('default', 'f32', b_cap, start, bs.ctl, run(start, bs.ctl, P, 'f32'))
