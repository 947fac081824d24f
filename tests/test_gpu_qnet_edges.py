"""astro_qvalues (csrc/astro_qnet.hip) where tests/test_gpu_qnet.py does not
reach: a wave's second and third chunk, designed tile and segment edges, the
bearing's wrap points, ties and saturated outputs, every nout with guarded
buffers, live (reset + auto-reset rollout) state and QNetwork.update.

The reference is the host's: tests/qnet_util.py builds the network's input
with oracle.features.batched (pinned bit for bit to the reference's
get_features) and runs astro_amd.qnet.forward64 on it; nothing from the
device enters it.  tol = 4 e_ref, e_ref = max |q32 - q64| of the network in
use over the evaluations of the test (q32: astro_amd.qnet.ValueNetwork in
float32 on the CPU), or the fixture's tol on golden states.  Every q buffer
is filled with NaN before the call, so an unwritten entry fails its test.
"""
import numpy as np
import pytest
import torch

from astro_amd import BatchedEnv, _lib, qnet
from astro_amd.config import DEFAULT_CONFIG
from oracle import batched
from tests import golden_io as gio
from tests import qnet_util as qu

pytestmark = pytest.mark.gpu

CFG = gio.configs()
DEV = 'cuda:0'
F32, F64 = torch.float32, torch.float64
# csrc/astro_qfwd.h: MAX_BLOCKS workgroups of QN_WAVES waves, SEGS (env, ego) segments per chunk
MAX_BLOCKS, QN_WAVES, SEGS = 512, 4, 32


@pytest.fixture(scope='module')
def tr():
    return gio.Transitions('steps.npz')


@pytest.fixture(scope='module')
def fx():
    return qu.fixture()[0]


@pytest.fixture(scope='module')
def nets(fx):
    return {k: qnet.QNetwork.from_module(v['weights'], DEV) for k, v in fx.items()}


@pytest.fixture(scope='module')
def golden(tr):
    """name -> (row indices, Batch of the group's input states, b_cap); built once per group."""
    cache = {}
    groups = dict(tr.groups())

    def get(name):
        if name not in cache:
            idx = groups[name]
            b_cap = tr.max_bullets(idx) + 2
            cache[name] = (idx, tr.batch_in(idx, 1 if CFG[name].solo else 2, b_cap=b_cap), b_cap)
        return cache[name]
    return get


def _cfg(S, p_pad):
    return DEFAULT_CONFIG._replace(solo=S == 1, max_planets=min(DEFAULT_CONFIG.max_planets, p_pad))


def _env_of(B, cfg, dtype, p_pad=None, b_cap=None):
    """A BatchedEnv holding the Batch's states (no auto-reset: it is never stepped)."""
    env = BatchedEnv(cfg, B.tick.shape[0], device=DEV, b_cap=b_cap or B.bullets.shape[1],
                     p_pad=p_pad or B.planets.shape[1], dtype=dtype, auto_reset=False)
    env.load_host(B.ships, B.ships_b, B.planets, B.bullets, B.tick, B.nplanets, B.nbullets)
    return env


def _run(env, net):
    """(q float64 [N, S, nout], control [N, S]) of one call into a NaN-filled q."""
    q = torch.full((env.n_env, env.S, net.nout), float('nan'), device=DEV)
    ctl = env.qcontrols(net, q_out=q).cpu().numpy()
    q = q.cpu().numpy()
    assert not np.isnan(q).any(), 'unwritten q: %d entries, first at %s' % (
        int(np.isnan(q).sum()), np.argwhere(np.isnan(q))[0])
    assert ctl.dtype == np.int8 and np.array_equal(ctl, np.argmax(q, axis=-1))
    return q.astype(np.float64), ctl


def _host_batch(env):
    h = env.to_host()
    return batched.Batch(h['tick'].astype(np.int32), h['nplanets'].astype(np.int32), h['nbullets'].astype(np.int32),
                         h['ships'].astype(np.float64), h['ships_b'].astype(np.float64),
                         h['planets'].astype(np.float64), h['bullets'].astype(np.float64),
                         (h['flags'] & 1).astype(bool))


# ---------------------------------------------------------------------------
# 1. more than one chunk per wave

@pytest.mark.parametrize('name,dtype,n', [('default', F32, 2 * 32768 + 3 * 16 + 5), ('solo', F64, 65536 + 2 * 32 + 7)])
def test_second_and_third_chunk_of_a_wave(golden, fx, nets, name, dtype, n):
    """The launch is capped at 512 workgroups of 4 waves; above 2048 chunks a
    wave walks a second chunk and reuses its LDS images.  Two ships: every
    wave gets two chunks and some a third; solo: the first waves get a
    second; the last chunk has a ragged end (5 / 7 envs).  The golden group
    tiled to that size (an odd period for the two ships, so no two chunks
    hold the same states) against the reference's own q64."""
    idx, B, b_cap = golden(name)
    S = 1 if CFG[name].solo else 2
    nchunks = -(-n // (SEGS // S))
    assert nchunks > S * MAX_BLOCKS * QN_WAVES and n % (SEGS // S) != 0 and idx.size % (SEGS // S) != 0
    rep = np.resize(np.arange(idx.size), n)
    env = _env_of(B.take(rep), CFG[name], dtype, p_pad=8, b_cap=b_cap)
    q, ctl = _run(env, nets[qu.kind(S)])
    want = qu.fixture()[2][idx[rep], :S]
    tol = fx[qu.kind(S)]['tol']
    err = np.abs(q - want).max(axis=(1, 2))
    print('%s %s n %d chunks %d: worst error %.3f tol (first chunk of a wave %.3f, later ones %.3f)'
          % (name, str(dtype)[6:], n, nchunks, err.max() / tol,
             err[:MAX_BLOCKS * QN_WAVES * SEGS // S].max() / tol, err[MAX_BLOCKS * QN_WAVES * SEGS // S:].max() / tol))
    assert err.max() <= tol, (name, np.argmax(err), err.max(), tol)
    checked, skipped = qu.check_argmax_rule(want, ctl, tol)
    assert checked == n * S and skipped == 0


# ---------------------------------------------------------------------------
# 2. designed chunk layouts

def _split(rows, p_pad, k):
    """(nplanets, nbullets) with nplanets + nbullets = rows, the planets varying with k."""
    npl = 1 + k % min(rows, p_pad)
    return npl, rows - npl


def _layout_cases():
    """[(label, S, p_pad, b_cap, tick, counts)]: one launch each."""
    cases = []
    # (a) two ships: per chunk of 16 envs one case -- its first env has r0 rows
    # (both ego segments), the other 15 one row each, so every later segment
    # boundary slides across the 32-row tile edges as r0 runs 1..70; 14 cases
    # per launch and a ragged last chunk of 5 one-row envs (21 envs from the
    # last case's first env on)
    for g in range(5):
        counts = []
        for r0 in range(1 + 14 * g, 15 + 14 * g):
            counts += [_split(r0, 8, r0 - 1)] + [(1, 0)] * 15
        cases.append(('a r0 %d..%d' % (1 + 14 * g, 14 + 14 * g), 2, 8, 80, 3 * (g % 2), counts + [(1, 0)] * 5))
    # (b) every env exactly k rows: a chunk's total is a multiple of 32, or one segment past it
    for S, n in ((1, 32 * 11 + 7), (2, 16 * 4 + 5)):
        for k in (1, 2, 16, 17, 32, 33):
            cases.append(('b S %d k %d' % (S, k), S, 8, 40, 0 if k in (2, 32) else 7, [_split(k, 8, i) for i in range(n)]))
    for S in (1, 2):
        n = 37
        # (c) every planet slot live at p_pad 16 (and a few envs with fewer)
        cases.append(('c p_pad 16 S %d' % S, S, 16, 4, 2, [(16 if i % 5 else 1 + i % 16, i % 4) for i in range(n)]))
        cases.append(('c p_pad 1 S %d' % S, S, 1, 6, 0, [(1, i % 6) for i in range(n)]))
        cases.append(('c b_cap 1 S %d' % S, S, 4, 1, 4, [(1 + i % 4, 0 if i % 7 == 3 else 1) for i in range(n)]))
        # one env of more than three tiles, then one-row envs; another in mid-chunk
        cases.append(('c rows >= 97 S %d' % S, S, 8, 100, 9,
                      [(3, 94 if S == 1 else 97)] + [(1, 0)] * 19 + [(8, 100)] + [(1, 0)] * 14 + [(1, 96)] + [(1, 0)] * 3))
    return cases


@pytest.fixture(scope='module')
def layouts(fx):
    """Every layout's Batch and host reference, once for both state dtypes
    (the values are float32-representable), and e_ref per network over all of them."""
    rng = np.random.RandomState(20260)
    out, e_ref, evals = [], {'duo': 0.0, 'solo': 0.0}, {'duo': 0, 'solo': 0}
    for label, S, p_pad, b_cap, tick, counts in _layout_cases():
        B = qu.synthetic_batch(counts, S, p_pad, rng, tick)
        q64, e = qu.reference_of(fx[qu.kind(S)]['weights'], B, S)
        e_ref[qu.kind(S)] = max(e_ref[qu.kind(S)], e)
        evals[qu.kind(S)] += len(counts) * S
        out.append((label, S, p_pad, b_cap, B, q64))
    assert min(evals.values()) >= 2000, evals
    return out, e_ref, evals


@pytest.mark.parametrize('dtype', [F32, F64])
def test_designed_chunk_layouts(layouts, nets, dtype):
    """Segments that end on a tile edge, one-row segments after long ones,
    chunk totals of exactly 32 k rows, full planet slots at p_pad 16, p_pad 1,
    b_cap 1 with its slot full, a segment of more than three tiles."""
    cases, e_ref, evals = layouts
    print('e_ref %s over %s evaluations' % (e_ref, evals))
    worst = 0.0
    for label, S, p_pad, b_cap, B, q64 in cases:
        rows = B.nplanets + B.nbullets
        seg = np.repeat(rows, S)
        ends = np.concatenate([np.cumsum(seg[a:a + SEGS]) for a in range(0, seg.size, SEGS)])
        env = _env_of(B, _cfg(S, p_pad), dtype, p_pad=p_pad, b_cap=b_cap)
        q, _ = _run(env, nets[qu.kind(S)])
        tol = 4.0 * e_ref[qu.kind(S)]
        err = np.abs(q - q64).max()
        worst = max(worst, err / tol)
        print('%-18s n %3d rows %3d..%3d  segments ending on a tile edge %3d  error %.3f tol'
              % (label, rows.size, rows.min(), rows.max(), int((ends % 32 == 0).sum()), err / tol))
        assert err <= tol, (label, str(dtype), err, tol)
    print('%s worst error %.3f tol' % (str(dtype)[6:], worst))


# ---------------------------------------------------------------------------
# 3. bearing wrap points

def _bearing_values(f32_only):
    pi32, two_pi = np.float32(np.pi), 2.0 * np.pi
    up32, down32 = np.nextafter(pi32, np.float32(4)), np.nextafter(pi32, np.float32(0))
    vals = [0.0, -0.0, two_pi * 5, two_pi * 100]
    for s in (1.0, -1.0):
        vals += [s * float(pi32), s * float(up32), s * float(down32), s * two_pi, s * 3 * np.pi, s * 88.6, s * 1e4]
        if not f32_only:
            vals += [s * np.pi, s * np.nextafter(np.pi, 4.0), s * np.nextafter(np.pi, 0.0),
                     s * float(np.float32(two_pi)), s * float(np.float32(3 * np.pi))]
    if f32_only:
        vals = [float(np.float32(v)) for v in vals]
    return np.array(vals, dtype=np.float64)


@pytest.mark.parametrize('dtype', [F32, F64])
def test_bearing_wrap_points(fx, dtype):
    """util.norm_angle(b) / pi at its wrap points (+-pi and its neighbours in
    both formats, multiples of 2 pi, large angles), in the float32 path of a
    game's first tick and the float64 path after it.  The bearing columns of
    f0 are scaled by 8; the test first shows on the host that a sign flip of
    the ego's bearing feature moves q64 by more than 10 tol in at least 90 %
    of the evaluations.  (A sign flip cannot move a feature that is 0, so the
    values whose feature is within 0.01 of 0 -- 0, -0 and the multiples of
    2 pi -- get one share of the envs each and every other value six.)"""
    w = {k: np.array(v) for k, v in fx['duo']['weights'].items()}
    w['f0.weight'][:, [5, 10]] *= 8
    net = qnet.QNetwork.from_module(w, DEV)
    vals = _bearing_values(dtype == F32)
    feat = ((vals + np.pi) % (2 * np.pi) - np.pi) / np.pi
    pool = np.concatenate([np.repeat(v, 1 if abs(f) < 0.01 else 6) for v, f in zip(vals, feat)])
    n = 600
    i = np.arange(n)
    bear = np.stack([pool[i % pool.size], pool[(5 * i + 3) % pool.size]], 1)
    assert set(bear[:, 0]) == set(vals) and set(bear[:, 1]) == set(vals)
    rng = np.random.RandomState(3)
    runs, e_ref = [], 0.0
    for tick in (0, 5):
        B = qu.synthetic_batch([(1 + k % 4, k % 3) for k in range(n)], 2, 4, rng, tick, bearings=bear)
        views = qu.batch_views(B, 2)
        q64 = qu.q64_of_views(w, views)
        e_ref = max(e_ref, float(np.abs(qu.q32_of_views(w, views) - q64).max()))
        flipped = []
        for v in views:
            v = v.copy()
            v[..., 5] = np.where(v[..., 0] >= 0, -v[..., 5], v[..., 5])
            flipped.append(v)
        runs.append((tick, B, q64, np.abs(qu.q64_of_views(w, flipped) - q64).max(-1)))
    tol = 4.0 * e_ref
    assert 2 * n * 2 >= 2000
    moved = np.mean([(m > 10 * tol).mean() for _, _, _, m in runs])
    print('e_ref %.3g over %d evaluations; a sign flip moves q64 by more than 10 tol in %.1f %% of them'
          % (e_ref, 4 * n, 100 * moved))
    assert moved >= 0.9
    for tick, B, q64, _ in runs:
        env = _env_of(B, _cfg(2, 4), dtype)
        q, _ = _run(env, net)
        err = np.abs(q - q64).max(-1)
        k = np.unravel_index(np.argmax(err), err.shape)
        print('%s tick %d: worst error %.3f tol (bearing %r)' % (str(dtype)[6:], tick, err.max() / tol, bear[k]))
        assert err.max() <= tol, (tick, bear[k], err.max(), tol)


# ---------------------------------------------------------------------------
# 4. ties and saturation

@pytest.fixture(scope='module')
def default_env(golden):
    idx, B, b_cap = golden('default')
    return idx, _env_of(B, CFG['default'], F64, p_pad=8, b_cap=b_cap)


def _with_v0(weights, rows, bias_shift=None):
    w = dict(weights)
    w['v0.weight'] = np.ascontiguousarray(weights['v0.weight'][rows])
    w['v0.bias'] = np.ascontiguousarray(weights['v0.bias'][rows])
    if bias_shift is not None:
        w['v0.bias'] = (w['v0.bias'] + np.asarray(bias_shift, dtype=np.float32)).astype(np.float32)
    return w


def test_ties_take_the_first_maximum(default_env, fx):
    """Duplicated rows of v0 give bit-identical outputs, and the control is
    the FIRST maximal index: 0 for six equal rows, 0 or 1 for rows a b a b a b,
    4 when only outputs 4 and 5 (the upper lane half's) hold the maximum."""
    idx, env = default_env
    wts, tol = fx['duo']['weights'], fx['duo']['tol']
    q64 = qu.fixture()[2][idx]
    bits = lambda a: a.astype(np.float32).view(np.int32)  # noqa: E731

    q, ctl = _run(env, qnet.QNetwork.from_module(_with_v0(wts, [0] * 6), DEV))
    assert all(np.array_equal(bits(q[..., 0]), bits(q[..., o])) for o in range(1, 6))
    worst = [np.abs(q[..., 0] - q64[..., 0]).max()]
    assert worst[-1] <= tol
    assert (ctl == 0).all()

    q, ctl = _run(env, qnet.QNetwork.from_module(_with_v0(wts, [0, 1] * 3), DEV))
    assert all(np.array_equal(bits(q[..., o % 2]), bits(q[..., o])) for o in range(2, 6))
    worst.append(np.abs(q[..., :2] - q64[..., :2]).max())
    assert worst[-1] <= tol
    assert set(ctl.flatten().tolist()) == {0, 1}
    checked, skipped = qu.check_argmax_rule(q64[..., :2], ctl, tol)
    assert skipped == 0 and checked == ctl.size

    q, ctl = _run(env, qnet.QNetwork.from_module(_with_v0(wts, [0] * 6, [-0.5] * 4 + [0, 0]), DEV))
    assert np.array_equal(bits(q[..., 4]), bits(q[..., 5]))
    assert all(np.array_equal(bits(q[..., 0]), bits(q[..., o])) for o in range(1, 4))
    worst.append(np.abs(q[..., 4] - q64[..., 0]).max())
    assert worst[-1] <= tol
    assert (q[..., 0] < q[..., 4]).all()
    assert (ctl == 4).all()
    print('six equal rows, a b a b a b, maximum in 4 and 5: worst error %.3f %.3f %.3f tol' % tuple(w / tol for w in worst))


@pytest.mark.parametrize('scale', [3, 10])
def test_large_weights_and_saturated_outputs(golden, fx, scale):
    """Every weight and bias x3 and x10 (a trained network's range) on the
    golden default and rapid states: within 4 e_ref of that network, and the
    control is the first maximum of the kernel's own q also where tanh has
    saturated to exactly +-1."""
    wts = qu.scaled(fx['duo']['weights'], scale)
    net = qnet.QNetwork.from_module(wts, DEV)
    runs, e_ref, evals = [], 0.0, 0
    for name in ('default', 'rapid'):
        idx, B, b_cap = golden(name)
        q64, e = qu.reference_of(wts, B, 2)
        e_ref = max(e_ref, e)
        evals += 2 * idx.size
        runs.append((name, B, b_cap, q64))
    assert evals >= 2000
    tol = 4.0 * e_ref
    sat = total = checked = skipped = 0
    for name, B, b_cap, q64 in runs:
        q, ctl = _run(_env_of(B, CFG[name], F64, p_pad=8, b_cap=b_cap), net)
        err = np.abs(q - q64).max()
        print('x%d %-8s e_ref %.3g  worst error %.3f tol' % (scale, name, e_ref, err / tol))
        assert err <= tol, (name, err, tol)
        sat += int((np.abs(q) == 1.0).sum())
        total += q.size
        if scale == 3:
            c, s = qu.check_argmax_rule(q64, ctl, tol)
            checked, skipped = checked + c, skipped + s
    print('x%d: %.2f %% of the q entries are exactly +-1' % (scale, 100.0 * sat / total))
    if scale == 10:
        assert sat >= 0.01 * total
    else:
        print('x3: argmax rule skipped %d of %d evaluations (%.2f %%)' % (skipped, checked, 100.0 * skipped / checked))
        assert skipped <= 0.10 * checked


def test_constant_network(default_env):
    """All weights 0: q = tanh(v0.bias) for every ship, control 1 (the first
    of the three maximal outputs 1, 2, 4).  The accumulators are exactly the
    float32 biases, so the only error is tanhf's: within 4 * 2^-24 (two units
    in the last place of a float32 below 1, plus its rounding, with room)."""
    idx, env = default_env
    w = {k: np.zeros(s, dtype=np.float32) for k, s in qnet.shapes(2, 6)}
    w['v0.bias'] = np.array([0.1, 0.3, 0.3, -1, 0.3, 0], dtype=np.float32)
    q, ctl = _run(env, qnet.QNetwork.from_module(w, DEV))
    want = np.tanh(w['v0.bias'].astype(np.float64))
    err = np.abs(q - want).max()
    print('constant network: max |q - tanh(bias)| %.3g' % err)
    assert err <= 4 * 2.0 ** -24
    assert (q == q[0, 0]).all()
    assert (ctl == 1).all()


# ---------------------------------------------------------------------------
# 5. every nout, guarded buffers

@pytest.mark.parametrize('name', ['default', 'solo'])
def test_every_nout_and_guarded_buffers(tr, golden, fx, name):
    """v0 cut to its first nout rows, nout 1..6, on 1, 15, 17, 33 and 517
    envs: q and control are the front of larger buffers whose 64 elements
    after them must stay what they were."""
    idx, B, b_cap = golden(name)
    S = 1 if CFG[name].solo else 2
    kind = qu.kind(S)
    wts, tol = fx[kind]['weights'], fx[kind]['tol']
    q64 = qu.fixture()[2]
    cut = {nout: qnet.QNetwork.from_module(_with_v0(wts, list(range(nout))), DEV) for nout in range(1, 7)}
    seed, tick0 = 99, 13
    worst = 0.0
    for k, n in enumerate((1, 15, 17, 33, 517)):
        sub = np.resize(np.arange(31 * k, idx.size), n)
        env = _env_of(B.take(sub), CFG[name], F32, p_pad=8, b_cap=b_cap)
        for nout, net in cut.items():
            assert net.nout == nout
            qbuf = torch.full((n * S * nout + 64,), float('nan'), device=DEV)
            qbuf[n * S * nout:] = 1234.5
            cbuf = torch.full((n * S + 64,), 77, dtype=torch.int8, device=DEV)
            qv, cv = qbuf[:n * S * nout].view(n, S, nout), cbuf[:n * S].view(n, S)
            env._qvalues(net, qv, cv, None, 0.0)
            q, ctl = qv.cpu().numpy().astype(np.float64), cv.cpu().numpy()
            assert (qbuf[n * S * nout:] == 1234.5).all() and (cbuf[n * S:] == 77).all(), (n, nout)
            assert not np.isnan(q).any(), (n, nout)
            err = np.abs(q - q64[idx[sub], :S, :nout]).max()
            worst = max(worst, err / tol)
            assert err <= tol, (n, nout, err, tol)
            assert np.array_equal(ctl, np.argmax(q, -1)), (n, nout)
            if nout == 1:
                assert (ctl == 0).all()
        # epsilon 1 with three outputs: the random draw is over the six controls of core.step
        pol = _lib.AstroPolicy(kind=_lib.POLICIES['random'], seed=seed, tick0=tick0, env_offset=0)
        cbuf = torch.full((n * S + 64,), 77, dtype=torch.int8, device=DEV)
        env._qvalues(cut[3], None, cbuf[:n * S].view(n, S), pol, 1.0)
        assert torch.equal(cbuf[:n * S].view(n, S), env.controls('random', seed, tick0))
        assert (cbuf[n * S:] == 77).all()
        if n == 517:
            assert int(cbuf[:n * S].max()) == 5
    print('%s: nout 1..6 on 1, 15, 17, 33, 517 envs: worst error %.3f tol' % (name, worst))


# ---------------------------------------------------------------------------
# 6. live state against the host reference

@pytest.mark.parametrize('solo,dtype', [(False, F32), (False, F64), (True, F32)])
def test_live_state_matches_host_reference(fx, nets, solo, dtype):
    """reset() and 150 random auto-reset ticks: bullets in flight, fresh games
    at tick 0.  q against the host
    reference of to_host()'s state; then the header's contract: flag bits
    and the bits above the tick change no bit of q, a planet count of 0 reads as 1 and a bullet count
    above b_cap as b_cap (on envs that are not the batch's last)."""
    n, b_cap = 3001, 32
    S = 1 if solo else 2
    kind = qu.kind(S)
    wts, net = fx[kind]['weights'], nets[kind]
    env = BatchedEnv(DEFAULT_CONFIG._replace(solo=solo), n, device=DEV, b_cap=b_cap, dtype=dtype, auto_reset=True)
    env.reset()
    env.rollout(150, 'random', seed=5)
    B = _host_batch(env)
    assert (B.nbullets > 0).sum() > n // 2 and 0 < (B.tick == 0).sum() < n // 4
    q64, e_ref = qu.reference_of(wts, B, S)
    assert n * S >= 2000
    tol = 4.0 * e_ref
    q, _ = _run(env, net)
    err = np.abs(q - q64).max(-1)
    t0 = B.tick == 0
    print('%s %s: e_ref %.3g, worst error %.3f tol (%d games at tick 0: %.3f tol), most rows %d'
          % (kind, str(dtype)[6:], e_ref, err.max() / tol, t0.sum(), err[t0].max() / tol,
             (B.nplanets + B.nbullets).max()))
    assert err.max() <= tol, (err.max(), tol)

    bits = lambda a: a.astype(np.float32).view(np.int32)  # noqa: E731
    hdr0 = env.hdr.clone()
    env.hdr[:, 0] |= 5 << 22      # the bits above the tick (reset keeps them) are not the tick
    env.hdr[:, 1] |= 3 << 8
    assert int(env.flags.min()) == 3 and torch.equal(env.tick.cpu(), torch.as_tensor(B.tick))
    assert np.array_equal(bits(_run(env, net)[0]), bits(q))
    env.hdr.copy_(hdr0)

    sel = np.arange(7, n - 1, 11)
    dsel = torch.as_tensor(sel, device=DEV)
    assert sel.max() < n - 1 and (B.nplanets[sel] > 1).any()
    # planet count 1, against the host; then 0, against count 1
    env.hdr[dsel, 1] = (hdr0[dsel, 1] & ~0xff) | 1
    B1 = B.copy()
    B1.nplanets[sel] = 1
    q1, _ = _run(env, net)
    assert np.abs(q1[sel] - qu.q64_of_batch(wts, B1.take(sel), S)).max() <= tol
    env.hdr[dsel, 1] = hdr0[dsel, 1] & ~0xff
    assert int(env.nplanets[dsel].max()) == 0
    assert np.array_equal(bits(_run(env, net)[0]), bits(q1))
    env.hdr.copy_(hdr0)
    # bullet count b_cap (every slot read), against the host; then b_cap + 3, against b_cap
    env.hdr[dsel, 1] = (hdr0[dsel, 1] & 0xffff) | (b_cap << 16)
    Bb = B.copy()
    Bb.nbullets[sel] = b_cap
    qb, _ = _run(env, net)
    assert np.abs(qb[sel] - qu.q64_of_batch(wts, Bb.take(sel), S)).max() <= tol
    assert not np.array_equal(bits(qb[sel]), bits(q[sel]))
    env.hdr[dsel, 1] = (hdr0[dsel, 1] & 0xffff) | ((b_cap + 3) << 16)
    assert int(env.nbullets[dsel].min()) == b_cap + 3
    assert np.array_equal(bits(_run(env, net)[0]), bits(qb))
    env.hdr.copy_(hdr0)
    assert np.array_equal(bits(_run(env, net)[0]), bits(q))


# ---------------------------------------------------------------------------
# 7. QNetwork.update

def test_update_repacks_in_place(golden, fx):
    """net.update(module) -- the training loop's call -- makes the device
    buffer that of a fresh from_module(module), in the same allocation."""
    idx, B, b_cap = golden('default')
    sub = np.arange(0, idx.size, 7)
    env = _env_of(B.take(sub), CFG['default'], F32, p_pad=8, b_cap=b_cap)
    net = qnet.QNetwork.from_module(fx['duo']['weights'], DEV)
    ptr = net.weights.data_ptr()
    old, _ = _run(env, net)
    torch.manual_seed(7)
    module2 = qnet.ValueNetwork(solo=False)
    net.update(module2)
    assert net.weights.data_ptr() == ptr == net.c.weights
    new, new_ctl = _run(env, net)
    fresh, fresh_ctl = _run(env, qnet.QNetwork.from_module(module2, DEV))
    assert np.array_equal(new.astype(np.float32).view(np.int32), fresh.astype(np.float32).view(np.int32))
    assert np.array_equal(new_ctl, fresh_ctl)
    assert np.abs(new - old).max() > 1e-3
    assert np.array_equal(net.weights.cpu().numpy(), qnet.pack(module2))
