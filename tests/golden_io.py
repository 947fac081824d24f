"""Load the committed golden fixtures (tests/golden/) into oracle Batches.

The fixtures were written by tools/gen_golden.py from the reference itself;
this module only reads data (npz with allow_pickle=False, json)."""
import io
import json
import os

import numpy as np

from astro_amd.config import Config
from oracle import batched

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def configs():
    with open(os.path.join(GOLDEN, 'configs.json')) as f:
        raw = json.load(f)['configs']
    return {k: Config(**v) for k, v in raw.items()}


def wide_configs():
    """mp11, mp16 and mp16_solo of wide.npz (tools/gen_golden.py: gen_wide):
    more than 8 planets, so they stay out of configs.json, whose names
    parametrise tests that run with 8 planet slots."""
    raw = json.loads(str(load('wide.npz')['configs']))
    return {k: Config(**v) for k, v in raw.items()}


def world_configs():
    """The configs of world.npz (tools/gen_golden.py: gen_world): ``world`` and
    its variants, every physics constant away from DEFAULT_CONFIG's, and one
    ``only_<field>`` config per constant.  They stay out of configs.json, whose
    sorted names parametrise other tests."""
    raw = json.loads(str(load('world.npz')['configs']))
    return {k: Config(**v) for k, v in raw.items()}


# world.npz: the eleven constants, the five configs that change all of them, and
# the single-field configs whose field create() reads
WORLD_FIELDS = ('gravity', 'dt', 'bullet_speed', 'ship_thrust', 'ship_rspeed', 'ship_radius', 'planet_radius',
                'planet_mass', 'planet_orbit', 'inner_ship_position', 'outer_ship_position')
WORLD_FULL = ('world', 'world_mp8', 'world_one', 'world_solo', 'world_rapid')
WORLD_CREATED = ('world', 'world_mp8', 'world_one', 'world_solo', 'only_gravity', 'only_planet_mass',
                 'only_planet_orbit', 'only_inner_ship_position', 'only_outer_ship_position')


def world_events(tr, configs):
    """Per transition of world.npz, from its input state alone (float64
    arithmetic on the recorded values): which pairs of bodies are within their
    collision distance, and whether a bullet that is not hit leaves the square
    on both axes (core.py:195)."""
    names = [str(x) for x in tr['cfg_names']]
    n = tr['tick'].shape[0]
    ev = {k: np.zeros(n, bool) for k in ('ship_ship', 'ship_planet', 'ship_bullet', 'bullet_planet', 'culled')}
    off = tr['in_bullets_off']

    def d2(a, b):
        return ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    for i in range(n):
        cfg = configs[names[tr['cfg'][i]]]
        S, npl = int(tr['nships'][i]), int(tr['nplanets'][i])
        sh = tr['in_ships'][i, :S, 0:2].astype(np.float64)
        pl = tr['in_planets'][i, :npl, 0:2].astype(np.float64)
        bl = tr['in_bullets'][off[i]:off[i + 1]].astype(np.float64)
        ev['ship_ship'][i] = S == 2 and d2(sh[:1], sh[1:])[0, 0] < (2 * cfg.ship_radius) ** 2
        ev['ship_planet'][i] = (d2(sh, pl) < (cfg.ship_radius + cfg.planet_radius) ** 2).any()
        ev['ship_bullet'][i] = (d2(sh, bl[:, 0:2]) < cfg.ship_radius ** 2).any()
        in_planet = (d2(bl[:, 0:2], pl) < cfg.planet_radius ** 2).any(1)
        hit = in_planet | (d2(bl[:, 0:2], sh) < cfg.ship_radius ** 2).any(1)
        ev['bullet_planet'][i] = in_planet.any()
        moved = bl[:, 0:2] + cfg.dt * bl[:, 2:4]
        ev['culled'][i] = (~hit & (np.abs(moved) > 1).all(1)).any()
    return ev


def world_games():
    """The whole free-running games of world.npz, as ``games()`` gives games.npz's."""
    z = load('world.npz')
    out = []
    for cfg in WORLD_FULL:
        for k in range(3):
            key = 'game_%s_%d' % (cfg, k)
            g = dict(cfg=cfg, gid=key)
            for f in ('seed', 'controls', 'ships', 'planets', 'nbullets', 'reward', 'done'):
                g[f] = z[key + '__' + f]
            out.append(g)
    return out


def load(name):
    """np.load of a fixture.  A fixture too large for one committed file is
    stored as consecutive byte ranges name.00, name.01, ... (tools/
    gen_golden.py: split_large) and read back as one."""
    path = os.path.join(GOLDEN, name)
    if os.path.exists(path):
        return np.load(path, allow_pickle=False)
    parts = sorted(f for f in os.listdir(GOLDEN)
                   if f.startswith(name + '.') and f[len(name) + 1:].isdigit())
    if not parts:
        raise FileNotFoundError(path)
    data = b''
    for f in parts:
        with open(os.path.join(GOLDEN, f), 'rb') as fh:
            data += fh.read()
    return np.load(io.BytesIO(data), allow_pickle=False)


def load_json(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


class Transitions:
    """Teacher-forced (state_in, control) -> reference output records."""

    def __init__(self, fname):
        z = load(fname)
        self.z = {k: z[k] for k in z.files}
        self.n = self.z['tick'].shape[0]
        self.cfg_names = [str(x) for x in self.z['cfg_names']]

    def groups(self):
        """Yield (cfg_name, row indices) per config."""
        for ci, name in enumerate(self.cfg_names):
            idx = np.nonzero(self.z['cfg'] == ci)[0]
            if idx.size:
                yield name, idx

    def max_bullets(self, idx):
        z = self.z
        nin = np.diff(z['in_bullets_off'])[idx]
        nout = np.diff(z['out_bullets_off'])[idx]
        return int(max(nin.max(initial=0), nout.max(initial=0)))

    def batch_in(self, idx, nships, p_pad=8, b_cap=None):
        z = self.z
        if b_cap is None:
            b_cap = max(self.max_bullets(idx), 1)
        B = batched.Batch.zeros(idx.size, nships, p_pad, b_cap)
        B.tick[:] = z['tick'][idx]
        B.nplanets[:] = z['nplanets'][idx]
        B.ships[:] = z['in_ships'][idx, :nships, 0:4]
        B.ships_b[:] = z['in_ships'][idx, :nships, 4]
        B.planets[:] = z['in_planets'][idx, :p_pad]
        off = z['in_bullets_off']
        for r, i in enumerate(idx):
            nb = off[i + 1] - off[i]
            B.nbullets[r] = nb
            B.bullets[r, :nb] = z['in_bullets'][off[i]:off[i + 1]]
        return B

    def expected(self, idx, nships, p_pad=8, b_cap=None):
        """Reference outputs as a Batch (+ reward, done)."""
        z = self.z
        if b_cap is None:
            b_cap = max(self.max_bullets(idx), 1)
        E = batched.Batch.zeros(idx.size, nships, p_pad, b_cap)
        E.ships[:] = z['out_ships'][idx, :nships, 0:4]
        E.ships_b[:] = z['out_ships'][idx, :nships, 4]
        E.planets[:] = z['out_planets'][idx, :p_pad]
        E.nplanets[:] = z['nplanets'][idx]
        off = z['out_bullets_off']
        for r, i in enumerate(idx):
            nb = off[i + 1] - off[i]
            E.nbullets[r] = nb
            E.bullets[r, :nb] = z['out_bullets'][off[i]:off[i + 1]]
        E.tick[:] = z['tick'][idx] + 1
        return E, z['out_reward'][idx, :nships], z['out_done'][idx]


def games():
    z = load('games.npz')
    idx = load_json('games.json')
    out = []
    for g in idx:
        key = 'g%03d' % g['gid']
        g = dict(g)
        for f in ('seed', 'controls', 'ships', 'planets', 'nbullets', 'reward'):
            g[f] = z[key + '__' + f]
        out.append(g)
    return out


class Features:
    """rl.ValueNetwork.get_features of every input state of steps.npz, and a
    few to_batch results (tools/gen_golden.py: gen_features)."""

    def __init__(self, fname='features.npz'):
        z = load(fname)
        self.z = {k: z[k] for k in z.files}

    def of(self, i):
        z = self.z
        a, b = z['features_off'][i], z['features_off'][i + 1]
        return z['features'][a:b, :z['dims'][i]]

    def batches(self):
        k = 0
        while 'batch_%d' % k in self.z:
            yield self.z['batch_idx_%d' % k], self.z['batch_%d' % k]
            k += 1
