"""CPU-only checks of the search library's host side (libastro_search.so's
argument codes, in the documented order, with pointers that are not memory),
of ``search.reduce_host`` on hand-written cases, and of the argument errors of
``fork.Lookahead``'s new arguments and of ``train.Distiller``, which come
before any device call."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
import astro_amd
from astro_amd import BatchedEnv, DEFAULT_CONFIG, SOLO_CONFIG, _lib, fork, search, train
from astro_amd.qnet import QNetwork
from tests import test_libraries as libraries

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------
# the library: header, constants, argument codes

def test_the_row_is_registered_next_to_the_table():
    """The binding lives in search.py; its row is in _lib.MORE, which build() compiles with _lib.LIBS."""
    row = search.ROW
    assert type(row) is _lib.Lib and _lib.MORE['search'] is row and _lib.row('search') is row
    assert 'search' not in _lib.LIBS and _lib.rows() == list(_lib.LIBS.values()) + [row]
    assert (row.key, row.file, row.source, row.env, row.abi, row.version, row.error, row.handle) == (
        'search', 'libastro_search.so', 'astro_search.hip', 'ASTRO_SEARCH_LIB', 1, 'astro_search_abi_version',
        'astro_search_last_error', '_search_lib')
    assert row.symbols is search.SYMBOLS and hasattr(_lib, row.handle)
    assert row.path == os.environ.get(row.env) or row.path == os.path.join(ROOT, 'astro_amd', row.file)
    assert len({r.key for r in _lib.rows()}) == len({r.file for r in _lib.rows()}) == len(_lib.rows())
    for key in ('search', 'fork'):
        with pytest.raises(ValueError, match='taken'):
            _lib.register(key, 'x.so', 'x.hip', 'X_LIB', 1, 'x_', {})
    assert astro_amd.search is search and astro_amd.Distiller is train.Distiller


def test_header_symbols_and_exports_are_one_set():
    """tests/test_libraries.py's checks of a row, for this one."""
    row = search.ROW
    entry.build_lib('search')
    declared = set(libraries.prototypes('search'))
    out = subprocess.check_output(['nm', '-D', '--defined-only', row.path], text=True)
    exported = set(re.findall(r' T (astro_\w+)$', out, re.M))
    assert declared == set(row.symbols) == exported == {'astro_search_abi_version', 'astro_search_last_error',
                                                        'astro_search_values'}
    lib = _lib._load('search', row.path)
    (abi,) = re.findall(r'^[ \t]*#[ \t]*define[ \t]+ASTRO_\w*ABI_VERSION[ \t]+(\d+)', libraries.text_of('search'), re.M)
    assert int(abi) == row.abi == getattr(lib, row.version)() == search.ABI_VERSION
    # the dependencies are the headers the source reaches
    src = os.path.join(entry.CSRC, row.source)
    assert {os.path.basename(d) for d in entry.dependencies(src)} == {'astro_search.hip', 'astro_search.h',
                                                                      'astro_common.h'}


def test_header_compiles_as_c99_and_the_mirrors_agree(tmp_path):
    """The struct's layout, the prototypes' kinds and the constants, header against search.py."""
    found = libraries.structs('search')
    assert list(found) == ['AstroSearch']
    fields = [f for f, _ in search.AstroSearch._fields_]
    assert fields == found['AstroSearch']
    body = ['printf("%zu\\n", sizeof(AstroSearch));'] + ['printf("%%zu\\n", offsetof(AstroSearch, %s));' % f for f in fields]
    expect = [ctypes.sizeof(search.AstroSearch)] + [getattr(search.AstroSearch, f).offset for f in fields]
    assert libraries.run_c('search', tmp_path, body) == expect and expect[0] == 72
    protos = libraries.prototypes('search')
    for name, (res, params) in protos.items():
        restype, argtypes = search.SYMBOLS[name]
        assert libraries.c_kind(res, False) == libraries.kind(restype), name
        assert len(params) == len(argtypes), name
        for i, (p, a) in enumerate(zip(params, argtypes)):
            assert libraries.c_kind(p, True) == libraries.kind(a), (name, i, p, a)
    got = libraries.run_c('search', tmp_path, ['printf("%d %d\\n", ASTRO_SEARCH_NCONTROL, ASTRO_SEARCH_ABI_VERSION);'])
    assert got == [search.NCONTROL, search.ABI_VERSION] == [6, 1]
    assert search.A == fork.Lookahead.NCONTROL == 6


def _s(**kw):
    d = dict(reward0=0x1000, done0=0x2000, reward=0x3000, done=0x4000, gamma=0x5000, leaf=0x6000, n_env=8, replies=1,
             nships=2, ship=0, horizon=4, reserved=0)
    d.update(kw)
    return search.AstroSearch(**d)


def test_argument_codes_without_gpu():
    """Every argument code of astro_search_values, in the documented order, with no device present."""
    entry.build()
    lib = search.load()
    V = ctypes.c_void_p
    good = dict(s=_s(), value=V(0x10000), own=V(0x11000), control=V(0x12000), first=V(0x13000))

    def call(**kw):
        a = dict(good)
        a.update(kw)
        rc = lib.astro_search_values(None if a['s'] is None else ctypes.byref(a['s']), a['value'], a['own'],
                                     a['control'], a['first'], None)
        return rc, lib.astro_search_last_error().decode()

    cases = [
        (dict(s=None), -170, 's is NULL'),
        (dict(s=_s(n_env=-1)), -3, 'n_env'),
        (dict(s=_s(nships=0)), -11, 'nships'), (dict(s=_s(nships=3)), -11, 'nships'),
        (dict(s=_s(ship=-1)), -171, 'ship'), (dict(s=_s(ship=2)), -171, 'ship'), (dict(s=_s(nships=1, ship=1)), -171, 'ship'),
        (dict(s=_s(horizon=0)), -172, 'horizon'), (dict(s=_s(horizon=-3)), -172, 'horizon'),
        (dict(s=_s(replies=0)), -173, 'replies'), (dict(s=_s(replies=2)), -173, 'replies'),
        (dict(s=_s(replies=36)), -173, 'replies'),
        (dict(s=_s(n_env=2 ** 31 - 1)), -174, 'int32'), (dict(s=_s(n_env=5000000, replies=6)), -174, 'int32'),
        (dict(value=None), -175, 'value'),
        (dict(own=None), -176, 'own'),
        (dict(s=_s(reward0=None)), -177, 'reward0'), (dict(s=_s(done0=None)), -177, 'reward0'),
        (dict(s=_s(gamma=None)), -177, 'reward0'),
        (dict(s=_s(reward=None)), -178, 'horizon > 1'), (dict(s=_s(done=None)), -178, 'horizon > 1'),
        (dict(s=_s(reward0=0x1002)), -179, 'aligned'), (dict(s=_s(reward=0x3001)), -179, 'aligned'),
        (dict(s=_s(gamma=0x5002)), -179, 'aligned'), (dict(s=_s(leaf=0x6002)), -179, 'aligned'),
        (dict(value=V(0x10002)), -179, 'aligned'), (dict(first=V(0x13001)), -179, 'aligned'),
    ]
    codes = []
    for kw, code, word in cases:
        rc, msg = call(**kw)
        assert rc == code and word in msg, (kw, rc, msg)
        if rc not in codes:
            codes.append(rc)
    assert codes == [-170, -3, -11, -171, -172, -173, -174, -175, -176, -177, -178, -179]   # the documented order
    # each case above is wrong in one thing; wrong in everything later too, the earlier code still wins
    later = dict(value=V(0x10002))
    for k, (kw, code, _) in enumerate(cases[:-6]):
        a = dict(later)
        a.update(kw)
        assert call(**a)[0] == code, kw
    assert call(s=_s(n_env=-1, nships=3, ship=9, horizon=0, replies=2), value=None)[0] == -3
    assert call(s=_s(nships=3, ship=9, horizon=0, replies=2), value=None)[0] == -11
    assert call(s=_s(ship=9, horizon=0, replies=2), value=None)[0] == -171
    assert call(s=_s(horizon=0, replies=2), value=None)[0] == -172
    assert call(s=_s(replies=2, n_env=2 ** 30), value=None)[0] == -173
    assert call(s=_s(n_env=2 ** 30), value=None)[0] == -174
    assert call(value=None, own=None)[0] == -175
    assert call(own=None, s=_s(reward0=None))[0] == -176
    assert call(s=_s(reward0=None, reward=None))[0] == -177
    assert call(s=_s(reward=None, gamma=0x5002))[0] == -178
    # the misaligned value keeps every call below from reaching a launch
    assert call(s=_s(horizon=1, reward=None, done=None), **later)[0] == -179      # K == 1: no rollout arrays
    assert call(s=_s(leaf=None), **later)[0] == -179                              # no leaf
    assert call(control=None, own=None, first=None, **later)[0] == -179           # no decision, no first
    assert call(control=None, **later)[0] == -179                                 # own without control is ignored
    # nothing to do: n_env == 0 after the scalar checks and before the arrays
    assert call(s=_s(n_env=0, reward0=None, done0=None, gamma=None), **later)[0] == 0
    assert call(s=_s(n_env=0), value=None)[0] == -175
    assert call(s=_s(n_env=0, horizon=0))[0] == -172


# ---------------------------------------------------------------------------
# reduce_host on hand-written cases

def _case(N, K, S=2, R=1):
    M = N * 6 * R
    return dict(reward0=np.zeros((M, S), F32), done0=np.zeros(M, np.uint8),
                reward=np.zeros((K - 1, M, S), F32) if K > 1 else None,
                done=np.zeros((K - 1, M), np.uint8) if K > 1 else None)


def test_reduce_host_by_hand():
    g = np.array([1.0, 0.5, 0.25, 0.125], F32)                     # K = 3
    c = _case(1, 3)
    # control 0 never ends; 1 ends at tick 0; 2 at tick 1; 3 at tick 2 (the last); 4 twice (tick 1: -1, tick 2: +1);
    # 5 by timeout (byte 2) at tick 2 with reward -0.0
    c['done0'][1], c['reward0'][1] = 1, (3.0, -3.0)
    c['done'][0, 2], c['reward'][0, 2] = 1, (-1.0, 1.0)
    c['done'][1, 3], c['reward'][1, 3] = 1, (2.0, 7.0)
    c['done'][0, 4], c['reward'][0, 4] = 1, (-1.0, 1.0)
    c['done'][1, 4], c['reward'][1, 4] = 1, (1.0, -1.0)
    c['done'][1, 5], c['reward'][1, 5] = 2, (-0.0, 0.0)
    c['reward'][1, 0] = (9.0, 9.0)                                # a reward without done counts for nothing
    v, ctl, first = search.reduce_host(gamma=g, ship=0, own=np.array([0], np.int8), **c)
    assert v.dtype == F32 and v.tolist() == [[0.0, 3.0, -0.5, 0.5, -0.5, -0.0]] and np.signbit(v[0, 5])
    assert first.tolist() == [-1, 0, 1, 2, 1, 2] and ctl.tolist() == [1]
    v1, _, _ = search.reduce_host(gamma=g, ship=1, **c)
    assert v1.tolist() == [[0.0, -3.0, 0.5, 1.75, 0.5, 0.0]] and not np.signbit(v1[0, 5])
    # a leaf values what does not end, at gamma[K], and nothing else; the other ship's rows are not read
    leaf = np.full((6, 2, 6), np.nan, F32)
    leaf[:, 0] = [[1, 2, 3, 4, 5, 6], [9, 9, 9, 9, 9, 9], [0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0],
                  [7, 7, 7, 7, 7, 7]]
    vl, ctl, _ = search.reduce_host(gamma=g, ship=0, leaf=leaf, own=np.array([3], np.int8), **c)
    assert vl.tolist() == [[0.75, 3.0, -0.5, 0.5, -0.5, -0.0]] and ctl.tolist() == [1]
    # K == 1: the rollout arrays are None
    k1 = dict(reward0=c['reward0'], done0=c['done0'], reward=None, done=None)
    v, _, first = search.reduce_host(gamma=g[:2], ship=0, leaf=leaf, **k1)
    assert v.tolist() == [[3.0, 3.0, 0.0, 0.0, 0.0, 3.5]] and first.tolist() == [-1, 0, -1, -1, -1, -1]


def test_reduce_host_replies_and_the_pick():
    g = np.array([1.0, 0.5], F32)
    c = _case(1, 1, R=6)
    c['done0'][:] = 1
    r = np.arange(36, dtype=F32).reshape(6, 6)        # control a: replies worth 6 a .. 6 a + 5
    r[1] = r[1, ::-1]                                 # the minimum last
    r[2, 3] = -5.0                                    # ... in the middle
    r[4] = 7.0                                        # all equal
    c['reward0'][:, 0] = r.reshape(-1)
    v, _, _ = search.reduce_host(gamma=g, ship=0, replies=6, **c)
    assert v.tolist() == [[0.0, 6.0, -5.0, 18.0, 7.0, 30.0]]
    pick = lambda row, own: search.pick_host(np.array([row], F32), np.array([own])).tolist()[0]   # noqa: E731
    assert pick([0, 5, 1, 5, 2, 3], 1) == 1           # own already maximal stays
    assert pick([0, 5, 1, 5, 2, 3], 3) == 3           # own tied with an earlier maximal control stays
    assert pick([0, 5, 1, 5, 2, 6], 1) == 5           # a strictly greater one later wins
    assert pick([0, 5, 1, 5, 2, 3], 0) == 1           # two equal maxima: the first
    assert pick([0, 5, 1, 5, 2, 3], 6) == 1 and pick([0, 5, 1, 5, 2, 3], -1) == 1   # own out of range
    assert pick([0, 0, 0, 0, 0, 0], 4) == 4 and pick([0.0, -0.0, 0, 0, 0, 0], 1) == 1
    assert search.gammas(0.995, 3).dtype == F32
    assert search.gammas(0.995, 3).tolist() == [float(F32(0.995 ** t)) for t in range(4)]


def test_shape_errors():
    c = _case(2, 3)
    g = np.ones(4, F32)
    for kw, word in ((dict(replies=2), 'replies'), (dict(reward0=c['reward0'][:11]), 'multiple'),
                     (dict(done0=c['done0'][:5]), 'done0'), (dict(gamma=np.ones(1, F32)), 'gamma'),
                     (dict(reward=None), 'needed'), (dict(done=c['done'][:1]), 'reward and done'),
                     (dict(leaf=np.zeros((12, 2, 5), F32)), 'leaf'), (dict(own=np.zeros(3, np.int8)), 'own'),
                     (dict(reward0=np.zeros((12, 3), F32)), 'reward0')):
        a = dict(c, gamma=g)
        a.update(kw)
        with pytest.raises(ValueError, match=word):
            search.reduce_host(**a)


# ---------------------------------------------------------------------------
# Lookahead's and Distiller's argument errors: before any device call

def _bare_env(config=DEFAULT_CONFIG, S=2, n_env=20):
    """A BatchedEnv that was never initialised: the checks read its shape only."""
    env = BatchedEnv.__new__(BatchedEnv)
    env.config, env.S, env.n_env, env.p_pad, env.b_cap, env.dtype = config, S, n_env, 4, 32, torch.float32
    env.device, env.planets_only = torch.device('cuda:0'), 0
    return env


def _bare_net(nships=2, nout=6):
    net = QNetwork.__new__(QNetwork)
    net.nships, net.nout = nships, nout
    return net


def _bare_teacher(env, ship=0):
    la = fork.Lookahead.__new__(fork.Lookahead)
    la.env, la.ship, la.leaf = env, ship, None
    return la


def test_lookahead_value_errors_before_the_device():
    two, solo = _bare_env(), _bare_env(SOLO_CONFIG, S=1)
    for env, kw, word in ((solo, dict(reply=True), 'two-ship'), (two, dict(leaf='script'), 'leaf'),
                          (two, dict(leaf=_bare_net(nships=1)), 'leaf'), (two, dict(leaf=_bare_net(nout=5)), 'leaf'),
                          (solo, dict(leaf=_bare_net()), 'leaf'),
                          (two, dict(ship=2, leaf=_bare_net()), 'ship'), (two, dict(horizon=0, reply=True), 'horizon')):
        with pytest.raises(ValueError, match=word):
            fork.Lookahead(env, **kw)
    with pytest.raises(TypeError):      # the new arguments are keyword arguments
        fork.Lookahead(two, 0, 4, 'script', 0.995, None, _bare_net())


def test_distiller_value_errors_before_the_device():
    env, other = _bare_env(), _bare_env()
    net, teacher = _bare_net(), _bare_teacher(env)
    for args, kw, word in (((env, net, 'script'), {}, 'teacher'), ((env, net, _bare_teacher(other)), {}, 'teacher'),
                           ((env, net, _bare_teacher(env, ship=1)), {}, 'ship 0'),
                           ((env, _bare_net(nout=5), teacher), {}, 'net'), ((env, _bare_net(nships=1), teacher), {}, 'net'),
                           ((env, 'net', teacher), {}, 'net'),
                           ((env, net, teacher), dict(opponent='snapshot'), 'opponent'),
                           ((env, net, teacher), dict(opponent=None), 'opponent'),
                           ((env, net, teacher), dict(explore=astro_amd.EpsilonGreedy.__new__(astro_amd.EpsilonGreedy)),
                            'explore'),
                           ((env, net, teacher), dict(envs_per_step=0), 'envs_per_step'),
                           ((env, net, teacher), dict(envs_per_step=21), 'envs_per_step'),
                           ((env, net, teacher), dict(envs_per_step=2.0), 'envs_per_step'),
                           ((env, net, teacher), dict(leaf_sync=-1), 'leaf_sync'),
                           ((env, net, teacher), dict(leaf_sync=True), 'leaf_sync'),
                           ((env, net, teacher), dict(leaf_sync=0.5), 'leaf_sync')):
        with pytest.raises(ValueError, match=word):
            train.Distiller(*args, **kw)
    assert teacher.leaf is None         # nothing was set on the way to an error
