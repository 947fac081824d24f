"""The device trace (astro_trace_state / astro_trace_result, include/astro_trace.h)
and what is built on it: ``record.Recorder``, ``record.play`` and
``play_q(record=...)`` / ``QTrainer.validate(record=...)``.

The kernels are checked against the plain copy -- ``env.to_host()`` before the
step and the tensors the step took and returned -- on a ring the test lays out
itself, every array followed by a guard and prefilled with a canary.  Whole
games are checked against ``logs.record_games`` on a twin env, against the numpy
oracle replaying the recorded controls, and the recorded Q values against
``env.qvalues`` on the recorded state.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from astro_amd import (BatchedEnv, DEFAULT_CONFIG, SOLO_CONFIG, SOLO_EASY_CONFIG, _lib, actor, logs, qnet, record,
                       replay, train)
from oracle import batched, port
from tests import qnet_util as qu

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARD = 256
TICKS = 40
CANARY = 0x5A


# ---------------------------------------------------------------------------
# the kernels against the plain copy

class Ring:
    """A ring of ``slots`` slots laid out by hand: every array is followed by GUARD bytes, all of it 0x5A."""

    def __init__(self, env, ids, slots, nout):
        S, m = env.S, len(ids)
        el = 8 if env.dtype == torch.float64 else 4
        self.np_dtype = np.float64 if el == 8 else np.float32
        self.shapes = dict(ships=((slots, m, S, 4), self.np_dtype), ships_b=((slots, m, S), self.np_dtype),
                           planets=((slots, m, env.p_pad, 4), self.np_dtype),
                           bullets=((slots, m, env.b_cap, 4), self.np_dtype), hdr=((slots, m, 4), np.int32),
                           control=((slots, m, S), np.int8), reward=((slots, m, S), np.float32),
                           done=((slots, m), np.uint8))
        if nout:
            self.shapes['q'] = ((slots, m, S, nout), np.float32)
        self.raw = {k: torch.full((int(np.prod(sh)) * np.dtype(dt).itemsize + GUARD,), CANARY, dtype=torch.uint8,
                                  device=DEV) for k, (sh, dt) in self.shapes.items()}
        self.ids = torch.tensor(ids, dtype=torch.int32, device=DEV)
        ptr = {k: v.data_ptr() for k, v in self.raw.items()}
        self.c = _lib.AstroTrace(ids=self.ids.data_ptr(), q=ptr.get('q'), m=m, ticks=slots, nout=nout, reserved=0,
                                 **{k: ptr[k] for k in self.shapes if k != 'q'})

    def host(self):
        """(the arrays, True if every guard still holds the canary)."""
        out, ok = {}, True
        for k, (sh, dt) in self.shapes.items():
            raw = self.raw[k].cpu().numpy()
            n = int(np.prod(sh)) * np.dtype(dt).itemsize
            out[k] = raw[:n].view(dt).reshape(sh)
            ok = ok and bool((raw[n:] == CANARY).all())
        return out, ok


def _env_bytes(env):
    return [t.clone() for t in (env.ships, env.ships_b, env.planets, env.bullets, env.hdr, env.stream, env.stream_ring)]


def _run_case(env, ids, nout, ticks=TICKS, check_every=1):
    """``ticks`` ticks under random controls with a trace call before and after every step; every slot
    against the host copy taken before the step.  Returns what the run saw (for the cases' own asserts)."""
    lib = _lib.load_trace()
    S, N, idx = env.S, env.n_env, np.asarray(ids)
    ring = Ring(env, ids, ticks, nout)
    stream = _lib.stream_ptr(env.device)
    rng = np.random.RandomState(3)
    want = []
    seen = dict(bullets=0, full=0, overflow=0, done=set(), dead_planets=0, max_nb=0)
    for t in range(ticks):
        h = env.to_host()
        seeds = env.game_seed.cpu().numpy()
        ctl = env.controls('random', seed=7, tick0=t)
        q = None
        if nout:
            q = torch.from_numpy(rng.randn(N, S, nout).astype(np.float32)).to(DEV)
        before = _env_bytes(env)
        _lib.check_trace(lib.astro_trace_state(ctypes.byref(env.params), ctypes.byref(env.state), ctypes.byref(ring.c),
                                               t, ctl.data_ptr(), None if q is None else q.data_ptr(), stream),
                         'astro_trace_state')
        assert all(torch.equal(a, b) for a, b in zip(before, _env_bytes(env))), 'state() wrote to the env'
        _, rew, done = env.step(ctl)
        before = _env_bytes(env)
        _lib.check_trace(lib.astro_trace_result(ctypes.byref(ring.c), t, rew.data_ptr(), done.data_ptr(), N, S, stream),
                         'astro_trace_result')
        assert all(torch.equal(a, b) for a, b in zip(before, _env_bytes(env))), 'result() wrote to the env'
        want.append((h, seeds, ctl.cpu().numpy(), None if q is None else q.cpu().numpy(), rew.cpu().numpy(),
                     done.cpu().numpy()))
        if t % check_every and t != ticks - 1:
            continue
        got, guards = ring.host()
        assert guards, 'a guard region was written at tick %d' % t
        for k, a in got.items():       # the slots beyond t keep the canary
            assert (a[t + 1:].view(np.uint8) == CANARY).all(), (k, t)
    got, _ = ring.host()
    p_pad, b_cap = env.p_pad, env.b_cap
    for t, (h, seeds, ctl, q, rew, done) in enumerate(want):
        npl, nb = h['nplanets'][idx], h['nbullets'][idx]
        assert (npl <= p_pad).all() and (nb <= b_cap).all()
        # live rows bit for bit (compared as bytes: no float compare in between), dead rows zero
        assert got['ships'][t].tobytes() == np.ascontiguousarray(h['ships'][idx]).tobytes(), t
        assert got['ships_b'][t].tobytes() == np.ascontiguousarray(h['ships_b'][idx]).tobytes(), t
        pl, bl = h['planets'][idx].copy(), h['bullets'][idx].copy()
        pl[np.arange(p_pad)[None, :] >= npl[:, None]] = 0
        bl[np.arange(b_cap)[None, :] >= nb[:, None]] = 0
        assert got['planets'][t].tobytes() == pl.tobytes(), t
        assert got['bullets'][t].tobytes() == bl.tobytes(), t
        word = got['hdr'][t].view(np.uint32)
        assert (word[:, 0] == h['tick'][idx]).all() and ((word[:, 1] & 0xff) == npl).all()
        assert (((word[:, 1] >> 8) & 0xff) == h['flags'][idx]).all() and ((word[:, 1] >> 16) == nb).all()
        assert (word[:, 2] == seeds[idx].view(np.uint32)).all() and (word[:, 3] == 0).all()
        assert np.array_equal(got['control'][t], ctl[idx]) and got['reward'][t].tobytes() == rew[idx].tobytes()
        assert np.array_equal(got['done'][t], done[idx])
        if q is not None:
            assert got['q'][t].tobytes() == np.ascontiguousarray(q[idx]).tobytes()
        seen['bullets'] += int(nb.sum())
        seen['full'] += int((nb == b_cap).sum())
        seen['overflow'] += int((h['flags'][idx] & 1).sum())
        seen['done'] |= set(done[idx].tolist())
        seen['dead_planets'] += int((p_pad - npl).sum())
        seen['max_nb'] = max(seen['max_nb'], int(nb.max()))
    env.check_errors()
    return seen


FAST = DEFAULT_CONFIG._replace(reload_time=0.05, max_time=0.7)      # a shot every third tick, games of 35 ticks


def _ids(kind, n):
    return {'first': [0], 'last': [n - 1], 'three': [n // 2, 2, n - 1], 'wave+': list(range(3, 3 + 65)),
            'all': list(range(n))}[kind]


# (n_env, ids, b_cap, p_pad, config, dtype, nout, planets_only): every value of every axis once
CASES = {
    'n77-first-b1-f32': (77, 'first', 1, 4, FAST, torch.float32, 0, 0),
    'n77-last-b6-overflow-f64-q6': (77, 'last', 6, 4, FAST, torch.float64, 6, 0),
    'n300-three-b32-p8-q3': (300, 'three', 32, 8, FAST, torch.float32, 3, 0),
    'n300-wave+-b70-f32': (300, 'wave+', 70, 4, FAST, torch.float32, 0, 0),
    'n77-all-b70-f64-p16-q1': (77, 'all', 70, 16, FAST, torch.float64, 1, 0),
    'solo-n77-wave+-b32-f32-q6': (77, 'wave+', 32, 4, SOLO_CONFIG._replace(reload_time=0.05, max_time=0.5),
                                  torch.float32, 6, 0),
    'solo-p1-n300-all-f64': (300, 'all', 6, 1, SOLO_EASY_CONFIG._replace(reload_time=0.05, max_time=0.5),
                             torch.float64, 0, 0),
    'planets-only-3-n300-three': (300, 'three', 32, 4, FAST, torch.float32, 0, 3),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_kernels_equal_the_plain_copy(name):
    n, kind, b_cap, p_pad, cfg, dtype, nout, only = CASES[name]
    env = BatchedEnv(cfg, n, device=DEV, b_cap=b_cap, p_pad=p_pad, dtype=dtype, planets_only=only)
    env.reset()
    seen = _run_case(env, _ids(kind, n), nout, check_every=8)
    assert seen['bullets'] > 0 and seen['done'] >= {0, 2}, seen
    if b_cap <= 6:
        assert seen['overflow'] > 0 and seen['full'] > 0, seen       # flag bit 0, rows that are full
    if p_pad > 1 and not only and len(_ids(kind, n)) > 3:
        assert seen['dead_planets'] > 0, seen


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
def test_kernels_on_rows_loaded_full(dtype):
    """Every bullet row full (nbullets == b_cap = 70: both trips of the lane loop carry live rows), loaded
    through load_host with values whose every bit pattern is distinct."""
    n, b_cap = 77, 70
    env = BatchedEnv(FAST, n, device=DEV, b_cap=b_cap, dtype=dtype)
    env.reset()
    h = env.to_host()
    rng = np.random.RandomState(8)
    h['bullets'] = rng.uniform(-0.9, 0.9, size=h['bullets'].shape).astype(h['bullets'].dtype)
    h['bullets'][..., 2:] *= 1e-3                # slow: they stay on the board
    h['nbullets'] = np.full(n, b_cap)
    env.load_host(**h)
    seen = _run_case(env, [0, 38, n - 1], 0, ticks=4)
    assert seen['full'] >= 3 and seen['max_nb'] == b_cap


def test_a_bad_id_records_nothing():
    """An id outside [0, n_env) -- the host checks keep it out; the kernel must still not touch memory for it."""
    env = BatchedEnv(FAST, 77, device=DEV, b_cap=6)
    env.reset()
    env.rollout(10, 'random', seed=1)
    lib = _lib.load_trace()
    ring = Ring(env, [5, 77, -1, 1 << 30, 76], 2, 0)
    ctl = env.controls('random')
    _lib.check_trace(lib.astro_trace_state(ctypes.byref(env.params), ctypes.byref(env.state), ctypes.byref(ring.c), 1,
                                           ctl.data_ptr(), None, _lib.stream_ptr(env.device)), 'astro_trace_state')
    _, rew, done = env.step(ctl)
    _lib.check_trace(lib.astro_trace_result(ctypes.byref(ring.c), 1, rew.data_ptr(), done.data_ptr(), 77, 2,
                                            _lib.stream_ptr(env.device)), 'astro_trace_result')
    got, guards = ring.host()
    assert guards
    for k, a in got.items():
        flat = a.reshape(a.shape[0], a.shape[1], -1).view(np.uint8)
        assert (flat[0] == CANARY).all() and (flat[1, 1:4] == CANARY).all(), k
        assert not (flat[1, 0] == CANARY).all() and not (flat[1, 4] == CANARY).all(), k
    env.check_errors()


# ---------------------------------------------------------------------------
# whole games

def same_array(got, want, what):
    assert type(got) is type(want) is np.ndarray and got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(got, want), what


def same_state(got, want, what, dtypes=True):
    for part in ('ships', 'planets', 'bullets'):
        for f in ('x', 'dx', 'b'):
            g, w = getattr(getattr(got, part), f), getattr(getattr(want, part), f)
            if w is None:
                assert g is None
            elif dtypes:
                same_array(g, w, (what, part, f))
            else:
                assert g.shape == w.shape and np.array_equal(g, w), (what, part, f)
    assert (got.reload, got.t) == (want.reload, want.t), what


def same_games(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.config == w.config and g.winner == w.winner and type(g.winner) is type(w.winner)
        assert len(g.ticks) == len(w.ticks)
        for t, (x, y) in enumerate(zip(g.ticks, w.ticks)):
            same_state(x.state, y.state, (what, k, t))
            same_array(x.control, y.control, (what, k, t, 'control'))
            same_array(x.reward, y.reward, (what, k, t, 'reward'))
            assert x.bot_data == y.bot_data == [None] * len(x.control)


SHORT = DEFAULT_CONFIG._replace(max_time=3.0)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
def test_play_equals_record_games(dtype):
    n = 70
    ids = [0, 5, n - 1]
    envs = []
    for _ in range(2):
        env = BatchedEnv(SHORT, n, device=DEV, b_cap=32, dtype=dtype, auto_reset=False)
        env.reset()
        envs.append(env)
    policy = lambda env: env.controls('script')     # noqa: E731
    want = logs.record_games(envs[0], ids, policy)
    got = record.play(envs[1], ids, policy)
    assert list(got) == ids and len(want) == 3
    for i, w in zip(ids, want):
        same_games(got[i], [w], i)
    assert len({g.config.seed for g in want}) == 3
    envs[1].check_errors()


def test_games_with_auto_reset_equal_the_oracle():
    """Three consecutive games of four envs of a float64 env under random controls: the oracle, created
    from each game's seed and stepped with the recorded controls, reproduces every recorded state bit for
    bit and ends where the record ends; the seeds are the env's stream's."""
    cfg = DEFAULT_CONFIG._replace(max_time=3.0, reload_time=0.1)
    n, ids, G = 40, [0, 13, 14, 39], 3
    env = BatchedEnv(cfg, n, device=DEV, b_cap=48, dtype=torch.float64, auto_reset=True)
    env.reset()
    tick = [0]

    def policy(env):
        tick[0] += 1
        return env.controls('random', seed=5, tick0=tick[0])
    games = record.play(env, ids, policy, games=G)
    seeds = batched.game_seeds(env.stream_seeds, G)
    endings = set()
    for i in ids:
        assert len(games[i]) == G
        for k, game in enumerate(games[i]):
            assert game.config == cfg._replace(seed=int(seeds[i, k])), (i, k)
            o = port.Game(game.config)
            st = o.create()
            for t, tk in enumerate(game.ticks):
                # (dtypes: the oracle keeps create()'s empty float32 bullet arrays until the first shot,
                # state_of's rule gives float64 from tick 1 on; every array with rows agrees in dtype too)
                same_state(tk.state, st, (i, k, t), dtypes=False)
                for part in ('ships', 'planets'):
                    assert getattr(tk.state, part).x.dtype == getattr(st, part).x.dtype, (i, k, t, part)
                    assert getattr(tk.state, part).dx.dtype == getattr(st, part).dx.dtype, (i, k, t, part)
                if st.bullets.x.shape[0]:
                    assert tk.state.bullets.x.dtype == st.bullets.x.dtype == tk.state.bullets.dx.dtype
                st, rew = o.step(st, tk.control)
                assert (st is None) == (t == len(game.ticks) - 1), (i, k, t)
                if st is None:
                    same_array(tk.reward, rew.astype(tk.reward.dtype), (i, k, 'reward'))
                    assert tk.reward.dtype == (np.int64 if rew.dtype.kind == 'i' else np.float32)
                    assert game.winner == (None if rew.max() < 1 else int(np.argmax(rew)))
                    endings.add(rew.dtype.kind)
                else:
                    same_array(tk.reward, np.zeros(2, np.float32), (i, k, t, 'reward'))
    assert endings, 'no game ended'
    env.check_errors()


# ---------------------------------------------------------------------------
# play_q and validate

@functools.lru_cache(maxsize=None)
def _weights():
    fx, _, _ = qu.fixture()
    rng = np.random.default_rng(11)
    other = {k: (np.asarray(v, np.float32) * (1.0 + 0.3 * rng.standard_normal(v.shape))).astype(np.float32)
             for k, v in fx['duo']['weights'].items()}
    return dict(A=fx['duo']['weights'], B=other)


@pytest.fixture(scope='module')
def nets():
    return {k: qnet.QNetwork.from_module(w, DEV) for k, w in _weights().items()}


N_Q, IDS_Q = 256, [0, 1, 63, 64, 100, 129, 254, 255]
QCFG = DEFAULT_CONFIG._replace(max_time=1.5)


def _fresh(n=N_Q, cfg=QCFG):
    env = BatchedEnv(cfg, n, device=DEV, b_cap=32)
    env.reset()
    return env


def _load_state(env, states):
    """``states`` (reference States, one per env of ``env``) loaded with load_host."""
    n, S = env.n_env, env.S
    h = dict(ships=np.zeros((n, S, 4)), ships_b=np.zeros((n, S)), planets=np.zeros((n, env.p_pad, 4)),
             bullets=np.zeros((n, env.b_cap, 4)), tick=np.zeros(n, np.int64), nplanets=np.zeros(n, np.int64),
             nbullets=np.zeros(n, np.int64))
    for i, (st, tick) in enumerate(states):
        npl, nb = st.planets.x.shape[0], st.bullets.x.shape[0]
        h['ships'][i, :, :2], h['ships'][i, :, 2:], h['ships_b'][i] = st.ships.x, st.ships.dx, st.ships.b
        h['planets'][i, :npl, :2], h['planets'][i, :npl, 2:] = st.planets.x, st.planets.dx
        h['bullets'][i, :nb, :2], h['bullets'][i, :nb, 2:] = st.bullets.x, st.bullets.dx
        h['tick'][i], h['nplanets'][i], h['nbullets'][i] = tick, npl, nb
    env.load_host(**h)


def _check_q(games, net_of_ship, cfg=QCFG):
    """The recorded q of sampled ticks against env.qvalues on a third env loaded with the recorded states."""
    sample = []
    for i, gs in games.items():
        for g in gs:
            for t in sorted({0, 1, len(g.ticks) // 2, len(g.ticks) - 1}):
                sample.append((g.ticks[t], t))
    env = _fresh(len(sample), cfg)
    _load_state(env, [(tk.state, t) for tk, t in sample])
    checked = 0
    for s, net in enumerate(net_of_ship):
        if net is None:
            assert all(tk.bot_data[s] is None for tk, _ in sample)
            continue
        want = env.qvalues(net).cpu().numpy()
        for j, (tk, _) in enumerate(sample):
            q = tk.bot_data[s]['q']
            assert q.dtype == np.float32 and q.shape == (net.nout,)
            assert q.tobytes() == want[j, s].tobytes(), (j, s, q, want[j, s])
            checked += 1
    return checked


@pytest.mark.parametrize('opponent', [None, 'script', 'net'])
def test_play_q_with_a_recorder(nets, opponent):
    A, B = nets['A'], nets['B']
    opp = B if opponent == 'net' else opponent
    G = 2
    twin, env = _fresh(), _fresh()
    winner0, length0 = twin.play_q(A, opponent=opp, games=G)
    rec = record.Recorder(env, IDS_Q, q=True)
    winner, length = env.play_q(A, opponent=opp, games=G, record=rec)
    assert torch.equal(winner, winner0) and torch.equal(length, length0)
    assert torch.equal(env.hdr, twin.hdr) and torch.equal(env.ships, twin.ships)
    assert rec.fill == 0 and rec.nout == A.nout
    w, ln = winner.cpu().numpy(), length.cpu().numpy()
    for i in IDS_Q:
        assert len(rec.games[i]) >= G
        for k in range(G):
            game = rec.games[i][k]
            assert (-1 if game.winner is None else game.winner) == w[i, k] and len(game.ticks) == ln[i, k], (i, k)
            assert game.ticks[0].state.t == 0.0
    assert len({g.config.seed for gs in rec.games.values() for g in gs}) == sum(len(gs) for gs in rec.games.values())
    ships = (A, A) if opponent is None else ((A, None) if opponent == 'script' else (A, B))
    assert _check_q({i: gs[:G] for i, gs in rec.games.items()}, ships) > 50
    if opponent == 'script':     # ship 1's recorded control is ScriptBot's on the recorded state
        sample = [(tk, t) for gs in rec.games.values() for g in gs[:1] for t, tk in enumerate(g.ticks)][:256]
        third = _fresh(len(sample))
        _load_state(third, [(tk.state, t) for tk, t in sample])
        want = third.controls('script').cpu().numpy()
        assert all(tk.bot_data[1] is None for tk, _ in sample)
        assert [int(tk.control[1]) for tk, _ in sample] == want[:, 1].tolist()
    env.check_errors()


def test_validate_with_a_recorder(nets):
    net = nets['A'].clone()
    env = _fresh(64)
    buf = replay.ReplayBuffer(64, env.p_pad + env.b_cap, 2, 6, n_steps=2, device=DEV)
    tr = train.QTrainer(env, net, buf, actor.EpsilonGreedy(env, seed=3), n_samples=32, seed=5)
    want = tr.validate(_fresh(64), games=1, opponent='script')
    ev = _fresh(64)
    rec = record.Recorder(ev, [0, 9, 63], q=True)
    assert tr.validate(ev, games=1, opponent='script', record=rec) == want
    assert all(len(rec.games[i]) >= 1 for i in (0, 9, 63))
    assert rec.games[9][0].ticks[3].bot_data[1] is None and rec.games[9][0].ticks[3].bot_data[0]['q'].shape == (6,)


def test_save_and_load(nets, tmp_path):
    env = _fresh(64)
    rec = record.Recorder(env, [7, 3], q=6)
    env.play_q(nets['A'], opponent='nothing', record=rec)
    paths = rec.save(str(tmp_path / 'logs'))
    assert {'3_0.log', '7_0.log'} <= {p.rsplit('/', 1)[1] for p in paths}
    back = logs.load_log(str(tmp_path / 'logs' / '7_0.log'))
    game = rec.games[7][0]
    assert back.config == game.config and back.winner == game.winner and len(back.ticks) == len(game.ticks)
    for x, y in zip(back.ticks, game.ticks):
        assert np.array_equal(x.bot_data[0]['q'], y.bot_data[0]['q'].astype(np.float64)) and x.bot_data[1] is None
        assert np.array_equal(x.state.ships.x, y.state.ships.x) and np.array_equal(x.control, y.control)


# ---------------------------------------------------------------------------
# misuse

def test_misuse(nets):
    env, other = _fresh(64), _fresh(64)
    rec = record.Recorder(env, [1, 2], ticks=3)
    ctl = env.controls('nothing')
    with pytest.raises(RuntimeError, match='open slot'):
        rec.result(env.reward, env.done)
    for _ in range(3):
        rec.state(ctl)
        with pytest.raises(RuntimeError, match='twice'):
            rec.state(ctl)
        with pytest.raises(RuntimeError, match='open slot'):
            rec.drain()
        _, r, d = env.step(ctl)
        rec.result(r, d)
    assert rec.fill == 3
    with pytest.raises(RuntimeError, match='full'):
        rec.state(ctl)
    first = rec.host()
    assert rec.drain() == [] and rec.fill == 0
    assert [len(v) for v in rec._pending.values()] == [3, 3]
    # reusable: a second run over the same slots records the ticks 3, 4, 5
    for t in range(3):
        h = env.to_host()
        rec.state(ctl)
        _, r, d = env.step(ctl)
        rec.result(r, d)
        got = rec.host()
        assert np.array_equal(got['ships'][t], h['ships'][[1, 2]]) and (got['hdr'][t, :, 0] == 3 + t).all()
    assert not np.array_equal(rec.host()['ships'], first['ships'])
    rec.drain()
    assert [tk.state.t for tk in rec._pending[1]] == [float(env.schedule.t[k]) for k in range(6)]
    # q or no q as the recorder was made; the env's own tensors only
    with pytest.raises(ValueError, match='without q'):
        rec.state(ctl, torch.zeros(64, 2, 6, device=DEV))
    with pytest.raises(ValueError, match='needs the Q'):
        record.Recorder(env, [0], q=True).state(ctl)
    with pytest.raises(ValueError, match='control'):
        rec.state(ctl[:32])
    # play_q: a recorder of this env, with at least 64 slots
    with pytest.raises(ValueError, match='of this env'):
        other.play_q(nets['A'], record=record.Recorder(env, [0], q=True))
    with pytest.raises(ValueError, match='64'):
        env.play_q(nets['A'], record=record.Recorder(env, [0], ticks=8, q=True))
    assert rec.fill == 0 and not rec.open
