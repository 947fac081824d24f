"""CPU-only checks of the evolution-strategy library's host side
(libastro_es.so: its row, its binding, its argument codes in the documented
order with pointers that are not memory), of ``es``' numpy mirrors on
hand-written cases, of the estimator's direction on a quadratic, and of the
argument errors of ``Population`` and ``ESTrainer``, which come before any
device call."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
import astro_amd
from astro_amd import BatchedEnv, DEFAULT_CONFIG, SOLO_CONFIG, _lib, es, league
from astro_amd.qnet import QNetwork
from tests import test_libraries as libraries

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = {'astro_es_abi_version', 'astro_es_last_error', 'astro_es_perturb', 'astro_es_score', 'astro_es_gradient'}


# ---------------------------------------------------------------------------
# the row

def test_the_row_is_in_the_third_table():
    row = es.ROW
    assert type(row) is _lib.Lib and _lib.LATER['es'] is row and _lib.row('es') is row
    assert 'es' not in _lib.LIBS and 'es' not in _lib.MORE and row not in _lib.rows()
    assert row in _lib.all_rows() and _lib.all_rows()[:len(_lib.rows())] == _lib.rows()
    assert set(map(id, _lib.all_rows())) == set(map(id, _lib.rows() + list(_lib.LATER.values())))
    assert (row.key, row.file, row.source, row.env, row.abi, row.version, row.error, row.handle) == (
        'es', 'libastro_es.so', 'astro_es.hip', 'ASTRO_ES_LIB', 1, 'astro_es_abi_version', 'astro_es_last_error',
        '_es_lib')
    assert row.symbols is es.SYMBOLS and hasattr(_lib, row.handle)
    assert row.path == os.environ.get(row.env) or row.path == os.path.join(ROOT, 'astro_amd', row.file)
    every = _lib.all_rows()
    assert len({r.key for r in every}) == len({r.file for r in every}) == len({r.handle for r in every}) == len(every)
    for r in every:      # a row of any table is found by its key
        assert _lib.row(r.key) is r
    assert astro_amd.es is es and astro_amd.ESTrainer is es.ESTrainer and astro_amd.Population is es.Population


def test_a_key_is_taken_once_across_the_three_tables():
    before = [list(t) for t in (_lib.LIBS, _lib.MORE, _lib.LATER)]
    for key in ('es', 'search', 'fork', 'hip'):
        for reg in (_lib.register, _lib.register_later):
            with pytest.raises(ValueError, match='taken'):
                reg(key, 'x.so', 'x.hip', 'X_LIB', 1, 'x_', {})
    assert [list(t) for t in (_lib.LIBS, _lib.MORE, _lib.LATER)] == before
    with pytest.raises(KeyError):
        _lib.row('no such library')


# ---------------------------------------------------------------------------
# the binding

def test_header_symbols_and_exports_are_one_set():
    row = es.ROW
    entry.build_lib('es')
    declared = set(libraries.prototypes('es'))
    out = subprocess.check_output(['nm', '-D', '--defined-only', row.path], text=True)
    exported = set(re.findall(r' T (astro_\w+)$', out, re.M))
    assert declared == set(row.symbols) == exported == EXPORTS
    lib = _lib._load('es', row.path)
    (abi,) = re.findall(r'^[ \t]*#[ \t]*define[ \t]+ASTRO_\w*ABI_VERSION[ \t]+(\d+)', libraries.text_of('es'), re.M)
    assert int(abi) == row.abi == getattr(lib, row.version)() == es.ABI_VERSION == 1
    src = os.path.join(entry.CSRC, row.source)
    assert {os.path.basename(d) for d in entry.dependencies(src)} == {'astro_es.hip', 'astro_es.h', 'astro_common.h'}


def test_header_compiles_as_c99_and_the_mirrors_agree(tmp_path):
    found = libraries.structs('es')
    assert list(found) == ['AstroES']
    fields = [f for f, _ in es.AstroES._fields_]
    assert fields == found['AstroES'] == ['seed', 'generation', 'nparams', 'pairs', 'sigma', 'reserved']
    body = ['printf("%zu\\n", sizeof(AstroES));'] + ['printf("%%zu\\n", offsetof(AstroES, %s));' % f for f in fields]
    expect = [ctypes.sizeof(es.AstroES)] + [getattr(es.AstroES, f).offset for f in fields]
    assert libraries.run_c('es', tmp_path, body) == expect == [32, 0, 8, 16, 20, 24, 28]
    protos = libraries.prototypes('es')
    for name, (res, params) in protos.items():
        restype, argtypes = es.SYMBOLS[name]
        assert libraries.c_kind(res, False) == libraries.kind(restype), name
        assert len(params) == len(argtypes), name
        for i, (p, a) in enumerate(zip(params, argtypes)):
            assert libraries.c_kind(p, True) == libraries.kind(a), (name, i, p, a)
    got = libraries.run_c('es', tmp_path, [
        'printf("%d %d %d %d %d %d\\n", ASTRO_ES_ABI_VERSION, ASTRO_ES_MAX_PAIRS, ASTRO_ES_MAX_MEMBERS, '
        'ASTRO_ES_MAX_PARAMS, ASTRO_ES_RANKS, ASTRO_ES_RAW);'])
    assert got == [es.ABI_VERSION, es.MAX_PAIRS, es.MAX_MEMBERS, es.MAX_PARAMS, es.SHAPINGS['ranks'],
                   es.SHAPINGS['raw']] == [1, 512, 1024, 1 << 20, 0, 1]
    assert es.MAX_PARAMS == _lib.QOPT_MAX_PARAMS and es.MAX_MEMBERS == 2 * es.MAX_PAIRS


# ---------------------------------------------------------------------------
# argument codes

V = ctypes.c_void_p


def _es(**kw):
    d = dict(seed=1, generation=0, nparams=100, pairs=8, sigma=0.05, reserved=0)
    d.update(kw)
    return es.AstroES(**d)


def _in_order(calls, order):
    codes = []
    for rc, msg, code, word in calls:
        assert rc == code and word in msg, (rc, msg, code, word)
        if rc not in codes:
            codes.append(rc)
    assert codes == order


def test_perturb_argument_codes_without_gpu():
    entry.build_lib('es')
    lib = es.load()
    good = dict(e=_es(), theta=V(0x10000), first=0, n=8, members=V(0x20000))

    def call(**kw):
        a = dict(good)
        a.update(kw)
        rc = lib.astro_es_perturb(None if a['e'] is None else ctypes.byref(a['e']), a['theta'], a['first'], a['n'],
                                  a['members'], None)
        return rc, lib.astro_es_last_error().decode()

    bad = V(0x20002)     # a misaligned members keeps every call below from reaching a launch
    cases = [
        (dict(e=None), -180, 'NULL'),
        (dict(e=_es(nparams=0)), -181, 'nparams'), (dict(e=_es(nparams=(1 << 20) + 1)), -181, 'nparams'),
        (dict(e=_es(pairs=0)), -182, 'pairs'), (dict(e=_es(pairs=513)), -182, 'pairs'),
        (dict(e=_es(sigma=0.0)), -183, 'sigma'), (dict(e=_es(sigma=-1.0)), -183, 'sigma'),
        (dict(e=_es(sigma=float('nan'))), -183, 'sigma'), (dict(e=_es(sigma=float('inf'))), -183, 'sigma'),
        (dict(first=-1), -184, 'pairs'), (dict(n=-1), -184, 'pairs'), (dict(first=1), -184, 'pairs'),
        (dict(first=2 ** 31 - 1, n=2 ** 31 - 1), -184, 'pairs'),
        (dict(theta=None), -185, 'NULL'), (dict(members=None), -185, 'NULL'),
        (dict(members=V(0x10000)), -186, 'overlaps'), (dict(members=V(0x10000 + 396)), -186, 'overlaps'),
        (dict(members=V(0x10000 - 6400 + 4)), -186, 'overlaps'),
        (dict(theta=V(0x10002)), -189, 'aligned'), (dict(members=bad), -189, 'aligned'),
    ]
    _in_order([call(**kw) + (code, word) for kw, code, word in cases], [-180, -181, -182, -183, -184, -185, -186, -189])
    # wrong in everything later too, the earlier code still wins
    assert call(e=_es(nparams=0, pairs=0, sigma=0.0), first=-1, theta=None)[0] == -181
    assert call(e=_es(pairs=0, sigma=0.0), first=-1, theta=None)[0] == -182
    assert call(e=_es(sigma=0.0), first=-1, theta=None)[0] == -183
    assert call(first=-1, theta=None)[0] == -184
    assert call(theta=None, members=bad)[0] == -185
    assert call(theta=V(0x20002), members=bad)[0] == -186
    # members that ends where theta begins, and theta that ends where members begins, do not overlap
    assert call(theta=V(0x20002 + 6400), members=bad)[0] == -189
    assert call(theta=V(0x20002 - 400), members=bad)[0] == -189
    # nothing to do: npairs == 0 after the scalar checks and before the arrays
    assert call(n=0, theta=None, members=None)[0] == 0 and call(n=0, first=8, members=bad)[0] == 0
    assert call(n=0, first=9)[0] == -184


def test_score_argument_codes_without_gpu():
    entry.build_lib('es')
    lib = es.load()
    good = dict(winner=V(0x1000), ticks=V(0x2000), n_env=64, games=2, k=8, ship=0, draw=0.0, survive=0.0, timeout=500,
                counts=V(0x3000), lost=V(0x4000), fitness=V(0x5002))      # (the fitness is misaligned: no launch)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        rc = lib.astro_es_score(a['winner'], a['ticks'], a['n_env'], a['games'], a['k'], a['ship'], a['draw'],
                                a['survive'], a['timeout'], a['counts'], a['lost'], a['fitness'], None)
        return rc, lib.astro_es_last_error().decode()

    cases = [
        (dict(n_env=-1), -3, 'n_env'),
        (dict(games=0), -187, 'games'), (dict(n_env=2 ** 30, games=2), -187, 'int32'),
        (dict(k=0), -187, 'nmembers'), (dict(k=1025), -187, 'nmembers'), (dict(timeout=0), -187, 'timeout_tick'),
        (dict(ship=-1), -11, 'ship'), (dict(ship=2), -11, 'ship'),
        (dict(draw=float('nan')), -183, 'finite'), (dict(survive=float('inf')), -183, 'finite'),
        (dict(fitness=None), -185, 'fitness'), (dict(winner=None), -185, 'winner'), (dict(ticks=None), -185, 'winner'),
        (dict(), -189, 'aligned'), (dict(fitness=V(0x5000), ticks=V(0x2002)), -189, 'aligned'),
        (dict(fitness=V(0x5000), counts=V(0x3001)), -189, 'aligned'),
        (dict(fitness=V(0x5000), lost=V(0x4004)), -189, 'aligned'),
    ]
    _in_order([call(**kw) + (code, word) for kw, code, word in cases], [-3, -187, -11, -183, -185, -189])
    assert call(n_env=-1, games=0, ship=5, draw=float('nan'), fitness=None)[0] == -3
    assert call(games=0, ship=5, draw=float('nan'), fitness=None)[0] == -187
    assert call(ship=5, draw=float('nan'), fitness=None)[0] == -11
    assert call(draw=float('nan'), fitness=None)[0] == -183
    assert call(winner=None, ticks=None, n_env=0)[0] == -189            # no envs: no arrays needed
    assert call(counts=None, lost=None)[0] == -189                      # the optional outputs


def test_gradient_argument_codes_without_gpu():
    entry.build_lib('es')
    lib = es.load()
    good = dict(e=_es(), fitness=V(0x1000), shaping=0, util=V(0x2000), grad=V(0x3002))   # (grad misaligned: no launch)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        rc = lib.astro_es_gradient(None if a['e'] is None else ctypes.byref(a['e']), a['fitness'], a['shaping'],
                                   a['util'], a['grad'], None)
        return rc, lib.astro_es_last_error().decode()

    cases = [
        (dict(e=None), -180, 'NULL'), (dict(e=_es(nparams=-4)), -181, 'nparams'), (dict(e=_es(pairs=600)), -182, 'pairs'),
        (dict(e=_es(sigma=float('-inf'))), -183, 'sigma'),
        (dict(shaping=2), -188, 'shaping'), (dict(shaping=-1), -188, 'shaping'),
        (dict(fitness=None), -185, 'NULL'), (dict(grad=None), -185, 'NULL'),
        (dict(), -189, 'aligned'), (dict(grad=V(0x3000), fitness=V(0x1001)), -189, 'aligned'),
        (dict(grad=V(0x3000), util=V(0x2002)), -189, 'aligned'), (dict(util=None, shaping=1), -189, 'aligned'),
    ]
    _in_order([call(**kw) + (code, word) for kw, code, word in cases], [-180, -181, -182, -183, -188, -185, -189])
    assert call(e=_es(sigma=0.0), shaping=7, fitness=None)[0] == -183
    assert call(shaping=7, fitness=None)[0] == -188


# ---------------------------------------------------------------------------
# the noise

def test_noise_is_standardised_and_keyed_by_all_four():
    C = float.fromhex('0x1.bb67aep-16')
    assert es.NOISE_SCALE.dtype == F32 and float(es.NOISE_SCALE) == C == float(F32(np.sqrt(3.0 / (2.0 ** 32 - 1.0))))
    e = es.noise_host(seed=7, generation=3, first_pair=0, npairs=256, nparams=4934)
    assert e.dtype == F32 and e.shape == (256, 4934)
    mean, var, big = float(e.astype(np.float64).mean()), float(e.astype(np.float64).var()), float(np.abs(e).max())
    print('noise: mean %.5f variance %.5f max |eps| %.4f' % (mean, var, big))
    assert abs(mean) < 0.005 and abs(var - 1.0) < 0.01 and big <= float(F32(131070) * F32(C))
    # one value by hand: the word, its four fields, one float32 multiply
    z = int(astro_amd.replay.random_words(np.array([(5 << 32) | 9], np.uint64), 7, 3)[0])
    s = (z & 0xffff) + ((z >> 16) & 0xffff) + ((z >> 32) & 0xffff) + (z >> 48)
    assert e[5, 9] == F32(s - 131070) * F32(C)
    # a later run of pairs is the same noise
    assert np.array_equal(es.noise_host(7, 3, 100, 4, 4934), e[100:104])
    # it differs across pair, parameter, generation and seed, and is uncorrelated across them
    a = e[:128].ravel().astype(np.float64)
    others = {'pair': e[128:].ravel(), 'parameter': np.roll(e[:128], 1, axis=1).ravel(),
              'generation': es.noise_host(7, 4, 0, 128, 4934).ravel(), 'seed': es.noise_host(8, 3, 0, 128, 4934).ravel(),
              'generation 2^40': es.noise_host(7, 3 + 2 ** 40, 0, 128, 4934).ravel()}
    for what, b in others.items():
        b = b.astype(np.float64)
        assert (a != b).mean() > 0.99, what
        assert abs(np.corrcoef(a, b)[0, 1]) < 0.01, what


def test_perturb_host_is_antithetic():
    theta = np.linspace(-1, 1, 65).astype(F32)
    sigma = 0.1                                         # inexact in float32
    m = es.perturb_host(theta, sigma, 3, 2, 5, 3)
    eps = es.noise_host(3, 2, 5, 3, 65)
    assert m.dtype == F32 and m.shape == (6, 65)
    d = F32(sigma) * eps
    assert np.array_equal(m[0::2], theta + d) and np.array_equal(m[1::2], theta - d)
    assert not np.array_equal(m[0], m[1]) and es.perturb_host(theta, sigma, 3, 2, 5, 0).shape == (0, 65)


# ---------------------------------------------------------------------------
# score_host and utilities_host by hand

def test_score_host_by_hand():
    # 5 envs x 2 games, 2 members: member 0 owns envs 0-1, member 1 envs 2-4
    winner = np.array([[0, 1], [-1, -2], [1, 1], [0, -1], [3, -2]], np.int8)
    ticks = np.array([[10, 700], [500, 0], [20, 499], [30, 500], [501, 0]], np.int32)
    counts, lost, fit = es.score_host(winner, ticks, 2, ship=0, timeout_tick=500)
    assert counts.dtype == np.int32 and lost.dtype == np.int64 and fit.dtype == F32
    assert counts.tolist() == [[1, 1, 1], [1, 3, 1]] and lost.tolist() == [500, 20 + 499 + 500]   # 700, 501 clipped
    assert fit.tolist() == [0.0, float(F32(-2.0 / 5.0))]
    # draw and survive
    _, _, fit = es.score_host(winner, ticks, 2, ship=0, draw=0.5, survive=0.25, timeout_tick=500)
    assert fit.tolist() == [float(F32((0.0 + 0.5 + 0.25 * 1.0) / 3.0)), float(F32((-2.0 + 0.5 + 0.25 * (1019 / 500)) / 5.0))]
    # the other seat: the code 3 is a loss for either ship, ship 1's wins are ship 0's losses
    counts, lost, fit = es.score_host(winner, ticks, 2, ship=1, timeout_tick=500)
    assert counts.tolist() == [[1, 1, 1], [2, 2, 1]] and lost.tolist() == [10, 30 + 500]
    assert fit.tolist() == [0.0, 0.0]
    # more members than envs: blocks [0,0) [0,1) [1,1) [1,2) ... the empty ones have no fitness
    counts, lost, fit = es.score_host(winner[:2], ticks[:2], 4, ship=0, timeout_tick=500)
    assert es.blocks(2, 4) == [(0, 0), (0, 1), (1, 1), (1, 2)]
    assert counts.tolist() == [[0, 0, 0], [1, 1, 0], [0, 0, 0], [0, 0, 1]] and lost.tolist() == [0, 500, 0, 0]
    assert np.isnan(fit[[0, 2]]).all() and fit[[1, 3]].tolist() == [0.0, 0.0]
    # nothing played yet
    _, _, fit = es.score_host(np.full((3, 1), -2, np.int8), np.zeros((3, 1), np.int32), 1, timeout_tick=9)
    assert np.isnan(fit).all() and fit.view(np.uint32).tolist() == [0x7fc00000]


def test_utilities_host_by_hand():
    u = es.utilities_host(np.array([3.0, 1.0, 2.0, 0.0], F32))
    assert u.dtype == F32 and u.tolist() == [0.5, float(F32(2) / F32(6) - F32(0.5)), float(F32(4) / F32(6) - F32(0.5)), -0.5]
    # ties share the average rank: ranks (0, 1.5, 1.5, 3) of 3
    u = es.utilities_host(np.array([0.0, 1.0, 1.0, 5.0], F32))
    assert u.tolist() == [-0.5, 0.0, 0.0, 0.5]
    assert es.utilities_host(np.full(6, 0.25, F32)).tolist() == [0.0] * 6                   # all equal
    assert es.utilities_host(np.array([1.0, np.nan, 0.0, 2.0], F32)).tolist() == [0.0] * 4  # a NaN
    assert es.utilities_host(np.array([1.0, np.inf], F32), 'raw').tolist() == [0.0, 0.0]     # an infinity
    assert es.utilities_host(np.array([2.0, -1.0], F32)).tolist() == [0.5, -0.5]            # pairs == 1: divisor 2
    assert es.utilities_host(np.array([2.0, 2.0], F32)).tolist() == [0.0, 0.0]
    assert es.utilities_host(np.array([2.0, -1.0, 0.5, 0.5], F32), 'raw').tolist() == [2.0, -1.0, 0.5, 0.5]
    for bad in (np.zeros(3, F32), np.zeros(0, F32)):
        with pytest.raises(ValueError, match='pairs'):
            es.utilities_host(bad)
    with pytest.raises(ValueError, match='shaping'):
        es.utilities_host(np.zeros(2, F32), 'rank')


def test_gradient_host_by_hand():
    f = np.array([1.0, -1.0, 0.0, 2.0], F32)
    eps = es.noise_host(5, 2, 0, 2, 7).astype(np.float64)
    sigma = F32(0.3)
    g = es.gradient_host(f, 7, sigma, 5, 2, 'raw')
    want = -((0.0 + 2.0 * eps[0]) + (-2.0) * eps[1]) / ((2.0 * 2.0) * float(sigma))
    assert g.dtype == F32 and np.array_equal(g, want.astype(F32))
    assert np.array_equal(es.gradient_host(np.array([1.0, np.nan, 0.0, 2.0], F32), 7, sigma, 5, 2), np.zeros(7, F32))
    assert not np.array_equal(g, es.gradient_host(f, 7, sigma, 5, 3, 'raw'))      # the generation is in the key


# ---------------------------------------------------------------------------
# the estimator points the right way

@pytest.mark.parametrize('shaping', ['raw', 'ranks'])
def test_the_estimate_points_down_the_loss(shaping):
    """fitness = -|w - w*|^2 on 64 parameters, 512 pairs, sigma 0.05: the estimate is a gradient of the LOSS
    |w - w*|^2 (the sign is for a minimiser), so its cosine with 2 (w - w*) is near 1."""
    n, pairs, sigma = 64, 512, 0.05
    worst = 1.0
    for seed in range(20):
        rng = np.random.RandomState(seed)
        w, target = rng.normal(size=n).astype(F32), rng.normal(size=n).astype(F32)
        members = es.perturb_host(w, sigma, seed, 0, 0, pairs).astype(np.float64)
        fitness = (-((members - target.astype(np.float64)) ** 2).sum(1)).astype(F32)
        g = es.gradient_host(fitness, n, sigma, seed, 0, shaping).astype(np.float64)
        true = 2.0 * (w.astype(np.float64) - target)
        worst = min(worst, float(g @ true / (np.linalg.norm(g) * np.linalg.norm(true))))
    print('%s: the smallest cosine over 20 seeds is %.3f' % (shaping, worst))
    assert worst >= 0.8


# ---------------------------------------------------------------------------
# Population's and ESTrainer's argument errors: before any device call

def _bare_env(config=DEFAULT_CONFIG, S=2, n_env=64):
    env = BatchedEnv.__new__(BatchedEnv)
    env.config, env.S, env.n_env, env.p_pad, env.b_cap, env.dtype = config, S, n_env, 4, 32, torch.float32
    env.device, env.planets_only = torch.device('cuda:0'), 0
    return env


def _bare_net(nships=2, nout=6):
    net = QNetwork.__new__(QNetwork)
    net.nships, net.nout = nships, nout
    return net


def test_population_value_errors_before_the_device():
    net = _bare_net()
    for args, kw, word in ((('net', 2, 0.05), {}, 'net'), ((net, 0, 0.05), {}, 'pairs'), ((net, 17, 0.05), {}, 'pairs'),
                           ((net, 2.0, 0.05), {}, 'pairs'), ((net, True, 0.05), {}, 'pairs'),
                           ((net, 2, 0.0), {}, 'sigma'), ((net, 2, -1.0), {}, 'sigma'), ((net, 2, float('nan')), {}, 'sigma'),
                           ((net, 2, 1e39), {}, 'sigma'), ((net, 2, 1e-60), {}, 'sigma'), ((net, 2, 'x'), {}, 'sigma'),
                           ((net, 2, 0.05, 1.5), {}, 'seed'),
                           ((net, 2, 0.05), dict(rounds=0), 'rounds'), ((net, 16, 0.05), dict(rounds=33), 'pairs \\* rounds')):
        with pytest.raises(ValueError, match=word):
            es.Population(*args, **kw)


def test_trainer_value_errors_before_the_device():
    env, net = _bare_env(), _bare_net()
    bad_opt = object()
    for e, n, kw, word in ((_bare_env(SOLO_CONFIG, S=1), _bare_net(nships=1), {}, 'two-ship'),
                           (env, 'net', {}, 'net'), (env, _bare_net(nships=1), {}, 'net'),
                           (env, net, dict(pairs=0), 'pairs'), (env, net, dict(pairs=17), 'pairs'),
                           (env, net, dict(rounds=0), 'rounds'), (env, net, dict(pairs=16, rounds=33), 'pairs \\* rounds'),
                           (env, net, dict(games=0), 'games'), (env, net, dict(shaping='rank'), 'shaping'),
                           (env, net, dict(draw=float('nan')), 'draw'), (env, net, dict(survive=float('inf')), 'survive'),
                           (env, net, dict(lr='x'), 'lr'),
                           (env, net, dict(opponent=None), 'opponent'), (env, net, dict(opponent='snapshot'), 'opponent'),
                           (env, net, dict(opponent=[]), 'opponent'), (env, net, dict(opponent=['script', 3]), 'opponent'),
                           (env, net, dict(pairs=16, opponent=['script', 'nothing', league.Script(0.2, 0.3)]), 'envs'),
                           (env, net, dict(pairs=3), 'divisible'),
                           (env, net, dict(pairs=2, opponent='random'), 'random'),
                           (env, net, dict(pairs=2, opponent=['script', 'random']), 'random'),
                           (env, net, dict(pairs=2, optimizer=bad_opt), 'optimizer')):
        with pytest.raises(ValueError, match=word):
            es.ESTrainer(e, n, **kw)
    # the device calls' own shape errors need no device either
    for shaping in ('rank', None):
        with pytest.raises(ValueError, match='shaping'):
            es.gradient(torch.zeros(4), 10, 0.05, shaping=shaping)
    with pytest.raises(ValueError, match='HIP device'):
        es.gradient(torch.zeros(4), 10, 0.05)
    with pytest.raises(ValueError, match='2 \\* pairs'):
        es.gradient(torch.zeros(3), 10, 0.05)
    with pytest.raises(ValueError, match='theta'):
        es.perturb(torch.zeros((2, 2)), torch.zeros((2, 2)), 1, 0.05)
    with pytest.raises(ValueError, match='winner'):
        es.score(torch.zeros(4, dtype=torch.int8), torch.zeros(4, dtype=torch.int32), 2)
