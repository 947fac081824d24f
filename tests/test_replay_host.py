"""CPU-only checks of the replay buffer's host side: astro_amd/replay.py's numpy
model against the reference's own bookkeeping (tests/golden/replay.npz,
tools/gen_golden.py: gen_replay), the sampling rule's distribution
and libastro_replay.so's argument checks."""
import ctypes
import itertools

import numpy as np
import pytest

import __graft_entry__
from astro_amd import _lib, replay
from tests import golden_io as gio

def test_push_host_reproduces_the_reference_experiences():
    """One env per recorded game, S = 2, n_steps 7: every experience of both
    QBotTrainers, in order -- action, float32(reward), float32(discount),
    terminal and the experience its new_state_f is the state_f of -- exactly."""
    z = gio.load('replay.npz')
    n_steps, discount = int(z['n_steps']), float(z['discount'])
    lens = z['game_ticks'].astype(int)
    assert n_steps == 7 and discount == 0.995 and lens.tolist() == [91, 45, 150]
    G, ticks = len(lens), int(lens.max()) + 10        # no wrap: row = tick
    control = np.zeros((lens.max(), G, 2), np.int8)
    for s in range(2):
        control[z['s%d_tick' % s], z['s%d_game' % s], s] = z['s%d_action' % s]
    h = replay.new_host(G, 2, ticks)
    for t in range(int(lens.max())):
        done = (lens - 1 == t).astype(np.uint8)
        reward = np.where(done[:, None] != 0, z['game_reward'], 0.0).astype(np.float32)
        replay.push_host(h, t, control[t], reward, done, n_steps, discount)
    checked = dict(terminal=0, flushed=0)
    for s in range(2):
        game, tick = z['s%d_game' % s], z['s%d_tick' % s]
        assert game.shape[0] == lens.sum()
        for i in range(game.shape[0]):
            g, k = int(game[i]), int(tick[i])
            assert h['action'][k, g, s] == z['s%d_action' % s][i]
            assert h['reward'][k, g, s].tobytes() == np.float32(z['s%d_reward' % s][i]).tobytes(), (s, i)
            assert h['discount'][k, g].tobytes() == np.float32(z['s%d_discount' % s][i]).tobytes(), (s, i)
            assert (h['next'][k, g] == replay.NEXT_TERMINAL) == bool(z['s%d_terminal' % s][i])
            j = int(z['s%d_next' % s][i])
            if j < 0:
                assert z['s%d_terminal' % s][i]
                checked['terminal'] += 1
            else:
                assert game[j] == g and h['next'][k, g] == tick[j] % ticks, (s, i)
                checked['flushed'] += 1
    assert checked['terminal'] > 0 and checked['flushed'] > 0
    # the ends: a win and a loss carry +-1 back through the last window, the timeout carries 0
    assert set(np.unique(z['game_reward'])) == {-1.0, 0.0, 1.0}


def _inclusion(weights, picks):
    """Exact inclusion probabilities of successive sampling without replacement."""
    w = np.asarray(weights, dtype=np.float64)
    p = np.zeros(len(w))
    for order in itertools.permutations(range(len(w)), picks):
        left, prob = w.sum(), 1.0
        for i in order:
            prob *= w[i] / left
            left -= w[i]
        p[list(order)] += prob
    return p


def test_sample_host_distribution():
    """Losses 1, 2, 3, 4, 0 and inf, n = 3: the unscored one always, the zero
    one never, the others with the probabilities of successive sampling."""
    loss = np.array([1, 2, 3, 4, 0, np.inf], np.float32)
    draws = 20000
    hits = np.zeros(6)
    for d in range(draws):
        ids = replay.select_host(loss, np.ones(6, bool), 3, seed=12345, draw=d)
        assert ids.shape == (3,) and (np.diff(ids) > 0).all()
        hits[ids] += 1
    assert hits[5] == draws and hits[4] == 0
    p = _inclusion(loss[:4], 2)
    assert abs(p.sum() - 2.0) < 1e-12
    sd = np.sqrt(p * (1 - p) / draws)
    assert (np.abs(hits[:4] / draws - p) <= 5 * sd).all(), (hits[:4] / draws, p, sd)


def test_sample_host_classes_and_eligibility():
    nxt = np.array([[3, -1], [3, -2], [-2, -2], [0, 1], [-1, -1]], np.int32)    # ticks 5, N 2
    loss = np.full((5, 2, 1), np.inf, np.float32)
    # 3 pushes: rows 0..2 written, head 3: row 0 env 0 and row 1 env 0 point at the head
    assert replay.eligible_host(nxt, 3, 1)[..., 0].tolist() == [
        [False, True], [False, False], [False, False], [False, False], [False, False]]
    # 9 pushes: every row written, head 4
    ok = replay.eligible_host(nxt, 9, 1)[..., 0]
    assert ok.tolist() == [[True, True], [True, False], [False, False], [True, True], [False, False]]
    loss[0, 0], loss[0, 1], loss[1, 0], loss[3, 0] = 0.5, 0.0, np.nan, -1.0     # classes 1, 2, 2, 2; row 3 env 1: 0
    assert replay.sample_host(loss, nxt, 9, 1).tolist() == [7]
    assert replay.sample_host(loss, nxt, 9, 2).tolist() == [0, 7]
    assert replay.sample_host(loss, nxt, 9, 4).tolist() == [0, 1, 2, 7]         # class 2 in id order
    assert replay.sample_host(loss, nxt, 9, 99).tolist() == [0, 1, 2, 6, 7]
    assert replay.sample_host(loss, nxt, 9, 0).tolist() == []


def _ring(**kw):
    a = dict(features=0x10000, action=0x20000, reward=0x30000, discount=0x40000, next=0x50000, loss=0x60000,
             wstart=0x70000, gpow=0x80000, gamma=0.995, n_env=40, rows=5, nships=2, ticks=9, n_steps=7, reserved=0)
    a.update(kw)
    return _lib.AstroReplay(**a)


def test_bad_arguments_without_gpu():
    """Every bad argument has its own negative code and a message, and is
    rejected before the device is touched (the pointers are not memory)."""
    __graft_entry__.build()
    lib = _lib.load_replay()
    P = ctypes.c_void_p
    need = lib.astro_replay_sample_workspace_bytes(ctypes.byref(_ring()))
    m = 9 * 40 * 2
    assert need >= 5 * m + 3 * 4096 * 4 and need % 16 == 0
    assert lib.astro_replay_sample_workspace_bytes(None) == 0
    assert lib.astro_replay_sample_workspace_bytes(ctypes.byref(_ring(nships=3))) == 0
    assert lib.astro_replay_sample_workspace_bytes(ctypes.byref(_ring(n_env=2 ** 30, ticks=9))) == 0

    def err(rc):
        return rc, lib.astro_replay_last_error().decode()

    def push(rb=None, t=3, control=P(0x1000), reward=P(0x2000), done=P(0x3000), null_rb=False):
        rb = _ring() if rb is None else rb
        return err(lib.astro_replay_push(None if null_rb else ctypes.byref(rb), t, control, reward, done, None))

    def sample(rb=None, t=3, n=8, ids=P(0x1000), count=P(0x2000), ws=P(0x100000), ws_bytes=need, null_rb=False):
        rb = _ring() if rb is None else rb
        return err(lib.astro_replay_sample(None if null_rb else ctypes.byref(rb), t, n, 1, 2, ids, count, ws, ws_bytes,
                                           None))

    def gather(rb=None, ids=P(0x1000), n=8, f=P(0x2000), a=P(0x3000), r=P(0x4000), d=P(0x5000), nf=P(0x6000),
               term=P(0x7000), null_rb=False):
        rb = _ring() if rb is None else rb
        return err(lib.astro_replay_gather(None if null_rb else ctypes.byref(rb), ids, n, f, a, r, d, nf, term, None))

    def update(rb=None, ids=P(0x1000), loss=P(0x2000), n=8, null_rb=False):
        rb = _ring() if rb is None else rb
        return err(lib.astro_replay_update(None if null_rb else ctypes.byref(rb), ids, loss, n, None))

    shared = [
        (dict(null_rb=True), -100, 'rb is NULL'),
        (dict(rb=_ring(nships=0)), -101, 'nships'),
        (dict(rb=_ring(nships=3)), -101, 'nships'),
        (dict(rb=_ring(n_env=0)), -102, 'n_env'),
        (dict(rb=_ring(rows=0)), -103, 'rows'),
        (dict(rb=_ring(rows=(1 << 16) + 1)), -103, 'rows'),
        (dict(rb=_ring(n_steps=0)), -104, 'n_steps'),
        (dict(rb=_ring(ticks=8)), -105, 'n_steps + 2'),
        (dict(rb=_ring(n_env=2 ** 30, ticks=9)), -106, 'int32'),
        (dict(rb=_ring(gamma=float('nan'))), -107, 'gamma'),
        (dict(rb=_ring(loss=None)), -108, 'NULL'),
        (dict(rb=_ring(loss=0x60002)), -109, 'aligned'),
    ]
    codes = {}
    for fn in (push, sample, gather, update):
        for kw, code, word in shared:
            if fn is gather and code in (-108, -109):    # (gather does not use rb.loss: its own case follows)
                continue
            rc, msg = fn(**kw)
            assert rc == code and word in msg, (fn.__name__, kw, rc, msg)
            codes.setdefault(rc, set()).add(word)
    assert gather(rb=_ring(features=None))[0] == -108 and gather(rb=_ring(features=0x10002))[0] == -109
    assert push(rb=_ring(gpow=None))[0] == -108 and push(rb=_ring(wstart=0x70004))[0] == -109
    own = [
        (push, dict(t=-1), -110, 't < 0'), (sample, dict(t=-1), -110, 't < 0'),
        (sample, dict(n=-1), -111, 'n < 0'), (gather, dict(n=-1), -111, 'n < 0'), (update, dict(n=-1), -111, 'n < 0'),
        (push, dict(control=None), -112, 'control'), (push, dict(reward=None), -112, 'control'),
        (push, dict(done=None), -112, 'control'),
        (sample, dict(ids=None), -113, 'ids is NULL'), (gather, dict(ids=None), -113, 'ids is NULL'),
        (update, dict(ids=None), -113, 'ids is NULL'),
        (sample, dict(count=None), -114, 'count is NULL'),
        (gather, dict(f=None), -115, 'output'), (gather, dict(term=None), -115, 'output'),
        (gather, dict(a=None), -115, 'output'), (update, dict(loss=None), -115, 'loss is NULL'),
        (sample, dict(ws=None), -118, 'workspace'), (sample, dict(ws_bytes=need - 1), -118, 'workspace'),
        (push, dict(reward=P(0x2002)), -119, 'aligned'), (sample, dict(ids=P(0x1002)), -119, 'aligned'),
        (sample, dict(ws=P(0x100008)), -119, 'aligned'), (gather, dict(nf=P(0x6001)), -119, 'aligned'),
        (update, dict(loss=P(0x2001)), -119, 'aligned'),
    ]
    for fn, kw, code, word in own:
        rc, msg = fn(**kw)
        assert rc == code and word in msg, (fn.__name__, kw, rc, msg)
        codes.setdefault(rc, set()).add(word.split()[0])
    assert sorted(codes) == [-119, -118, -115, -114, -113, -112, -111, -110, -109, -108, -107, -106, -105, -104, -103,
                             -102, -101, -100]
    # the ring's scalars come first, then t or n, then the call's own pointers
    assert sample(rb=_ring(ticks=8), n=-1, ids=None)[0] == -105 and sample(n=-1, ids=None)[0] == -111
    # n == 0: gather and update have nothing to do, whatever the arrays are ...
    assert gather(n=0, ids=None, f=None)[0] == 0 and update(n=0, ids=None, loss=None)[0] == 0
    # ... but the ring is still checked
    assert gather(n=0, rb=_ring(ticks=8))[0] == -105 and update(n=0, null_rb=True)[0] == -100


def test_ticks_below_n_steps_plus_two_are_rejected():
    with pytest.raises(ValueError, match='n_steps'):
        replay.ReplayBuffer(4, 5, 2, ticks=8, n_steps=7)
    with pytest.raises(ValueError, match='n_steps'):
        replay.ReplayBuffer(4, 5, 2, ticks=101)
    with pytest.raises(ValueError):
        replay.ReplayBuffer(4, 5, 3, ticks=200)
    with pytest.raises(ValueError, match='HIP device'):
        replay.ReplayBuffer(4, 5, 2, ticks=9, n_steps=7, device='cpu')
    import astro_amd
    assert astro_amd.ReplayBuffer is replay.ReplayBuffer
    assert replay.gpow_table(0.995, 100)[37] == 0.995 ** 37
