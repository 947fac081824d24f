"""CPU-only checks of the fork library's host side (libastro_fork.so's argument
codes, in the documented order, with pointers that are not memory) and of
astro_amd/fork.py's host half: ``check_ids`` and the ``Fork`` plan's checks
that run before any device call."""
import ctypes

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
import astro_amd
from astro_amd import BatchedEnv, DEFAULT_CONFIG, SOLO_CONFIG, _lib, fork
from tests import test_libraries as libraries


# ---------------------------------------------------------------------------
# the library: header, constants, argument codes

def test_header_compiles_as_c99_and_the_constants_are_mirrored(tmp_path):
    libraries.test_struct_layouts_are_the_ctypes_mirrors('fork', tmp_path)       # (no struct of its own: compiles)
    libraries.test_prototypes_agree_with_restype_and_argtypes('fork', tmp_path)
    libraries.test_header_constants_are_the_python_ones('fork', tmp_path)
    got = libraries.run_c('fork', tmp_path, ['printf("%d %d %d\\n", ASTRO_FORK_GAME, ASTRO_FORK_STREAM, '
                                              'ASTRO_FORK_ABI_VERSION);'])
    assert got == [_lib.FORK_GAME, _lib.FORK_STREAM, _lib.FORK_ABI_VERSION] == [1, 2, 1]
    row = _lib.LIBS['fork']
    assert (row.file, row.source, row.env, row.abi, row.version, row.error, row.handle) == (
        'libastro_fork.so', 'astro_fork.hip', 'ASTRO_FORK_LIB', 1, 'astro_fork_abi_version', 'astro_fork_last_error',
        '_fork_lib')
    assert list(_lib.LIBS)[-1] == 'fork' and len(_lib.LIBS) == 11
    assert set(_lib._FORK_SYMBOLS) == {'astro_fork_abi_version', 'astro_fork_last_error', 'astro_fork'}
    assert astro_amd.fork is fork and astro_amd.Fork is fork.Fork and astro_amd.Lookahead is fork.Lookahead


def _params(**kw):
    d = dict(nships=2, solo=0, p_pad=4, max_planets=4, b_cap=32)
    d.update(kw)
    return _lib.AstroParams(**d)


def _state(base=0, **kw):
    d = dict(ships=base + 0x1000, ships_b=base + 0x2000, planets=base + 0x3000, bullets=base + 0x4000,
             hdr=base + 0x5000, stream=base + 0x6000, stream_ring=base + 0x7000, n_env=8, state_f64=0)
    d.update(kw)
    return _lib.AstroState(**d)


def _dst(**kw):
    return _state(0x100000, **kw)


def test_argument_codes_without_gpu():
    """Every argument code of astro_fork, in the documented order, with no device present."""
    entry.build()
    lib = _lib.load_fork()
    V = ctypes.c_void_p
    G, F = _lib.FORK_GAME, _lib.FORK_STREAM
    good = dict(p=_params(), s=_state(), d=_dst(), si=V(0x20000), di=V(0x21000), m=5, what=G | F)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        ref = lambda x: None if x is None else ctypes.byref(x)   # noqa: E731
        rc = lib.astro_fork(ref(a['p']), ref(a['s']), ref(a['d']), a['si'], a['di'], a['m'], a['what'], None)
        return rc, lib.astro_fork_last_error().decode()

    cases = [
        (dict(p=None), -10, 'params'), (dict(s=None), -2, 'src'), (dict(d=None), -160, 'dst'),
        (dict(p=_params(nships=0)), -11, 'nships'), (dict(p=_params(nships=3)), -11, 'nships'),
        (dict(p=_params(p_pad=0)), -13, 'p_pad'), (dict(p=_params(p_pad=17)), -13, 'p_pad'),
        (dict(p=_params(b_cap=0)), -15, 'b_cap'), (dict(p=_params(b_cap=65536)), -15, 'b_cap'),
        (dict(m=-1), -161, 'm must'),
        (dict(what=0), -162, 'what'), (dict(what=4), -162, 'what'), (dict(what=G | 8), -162, 'what'),
        (dict(what=-1), -162, 'what'),
        (dict(s=_state(state_f64=2), d=_dst(state_f64=2)), -6, 'state_f64'), (dict(d=_dst(state_f64=-1)), -6, 'state_f64'),
        (dict(s=_state(state_f64=1)), -163, 'differ'), (dict(d=_dst(state_f64=1)), -163, 'differ'),
        (dict(s=_state(n_env=-1)), -3, 'n_env'), (dict(d=_dst(n_env=-4)), -3, 'n_env'),
        (dict(s=_state(ships=None)), -4, 'src'), (dict(s=_state(ships_b=None)), -4, 'src'),
        (dict(s=_state(planets=None)), -4, 'src'), (dict(s=_state(hdr=None)), -4, 'src'),
        (dict(s=_state(stream=None)), -4, 'src'), (dict(s=_state(bullets=None)), -4, 'src'),
        (dict(s=_state(stream_ring=None)), -4, 'src'),
        (dict(s=_state(bullets=None), what=G), -4, 'src'), (dict(s=_state(stream_ring=None), what=F), -4, 'src'),
        (dict(d=_dst(ships=None)), -164, 'dst'), (dict(d=_dst(stream=None)), -164, 'dst'),
        (dict(d=_dst(bullets=None), what=G), -164, 'dst'), (dict(d=_dst(stream_ring=None), what=F), -164, 'dst'),
        (dict(s=_state(ships=0x1008)), -5, 'src arrays'), (dict(s=_state(planets=0x3004)), -5, 'src arrays'),
        (dict(s=_state(bullets=0x4008)), -5, 'src arrays'), (dict(s=_state(hdr=0x5004)), -5, 'src arrays'),
        (dict(s=_state(stream=0x6004)), -5, 'src arrays'), (dict(s=_state(stream_ring=0x7008)), -5, 'src arrays'),
        (dict(s=_state(ships_b=0x2002)), -5, 'src arrays'),
        (dict(s=_state(ships_b=0x2004, state_f64=1), d=_dst(state_f64=1)), -5, 'src arrays'),
        (dict(d=_dst(ships=0x101008)), -165, 'dst arrays'), (dict(d=_dst(stream_ring=0x107004)), -165, 'dst arrays'),
        (dict(d=_dst(ships_b=0x102004, state_f64=1), s=_state(state_f64=1)), -165, 'dst arrays'),
        (dict(si=V(0x20002)), -166, 'id arrays'), (dict(di=V(0x21001)), -166, 'id arrays'),
    ]
    codes = set()
    for kw, code, word in cases:
        rc, msg = call(**kw)
        assert rc == code and word in msg, (kw, rc, msg)
        codes.add(rc)
    assert sorted(codes) == [-166, -165, -164, -163, -162, -161, -160, -15, -13, -11, -10, -6, -5, -4, -3, -2]
    # the ids are misaligned in every call below that would otherwise reach the launch: none may
    bad_ids = dict(si=V(0x20002))
    # an array that `what` does not need may be NULL: bullets without GAME, the ring without STREAM
    assert call(s=_state(bullets=None), d=_dst(bullets=None), what=F, **bad_ids)[0] == -166
    assert call(s=_state(stream_ring=None), d=_dst(stream_ring=None), what=G, **bad_ids)[0] == -166
    # float bearings are aligned to 4 bytes
    assert call(s=_state(ships_b=0x2004), d=_dst(ships_b=0x102004), **bad_ids)[0] == -166
    # NULL id arrays are the identity, and aligned
    assert call(si=None, di=V(0x21002))[0] == -166
    # nothing to do: m == 0 after the m check and before `what`; an empty state after the scalar checks
    assert call(m=0)[0] == 0 and call(m=0, what=0, s=_state(ships=None, n_env=-1))[0] == 0
    assert call(m=0, p=_params(b_cap=0))[0] == -15
    empty = _state(n_env=0, ships=None, hdr=None)
    assert call(s=empty)[0] == 0 and call(d=_dst(n_env=0, stream=None, hdr=0x5004))[0] == 0
    assert call(s=empty, what=0)[0] == -162 and call(s=empty, d=_dst(state_f64=1))[0] == -163
    assert call(s=empty, d=_dst(n_env=-1))[0] == -3
    # the order: each call breaks the rule of its code and of every later one
    worst_s = dict(n_env=-1, ships=None, state_f64=2, hdr=0x5004)
    worst = dict(m=-1, what=0, si=V(0x20002))
    assert call(p=_params(nships=3, p_pad=0, b_cap=0), s=_state(**worst_s), d=_dst(**worst_s), **worst)[0] == -11
    assert call(p=_params(p_pad=0, b_cap=0), s=_state(**worst_s), d=_dst(**worst_s), **worst)[0] == -13
    assert call(p=_params(b_cap=0), s=_state(**worst_s), d=_dst(**worst_s), **worst)[0] == -15
    assert call(s=_state(**worst_s), d=_dst(**worst_s), **worst)[0] == -161
    worst.update(m=3)
    assert call(s=_state(**worst_s), d=_dst(**worst_s), **worst)[0] == -162
    worst.update(what=G | F)
    assert call(s=_state(**worst_s), d=_dst(**worst_s), **worst)[0] == -6
    worst_s.update(state_f64=1)
    assert call(s=_state(**worst_s), d=_dst(**dict(worst_s, state_f64=0)), **worst)[0] == -163
    assert call(s=_state(**worst_s), d=_dst(**worst_s), **worst)[0] == -3
    worst_s.update(n_env=8)
    assert call(s=_state(**worst_s), d=_dst(**worst_s), **worst)[0] == -4
    assert call(s=_state(**dict(worst_s, ships=0x1000)), d=_dst(**worst_s), **worst)[0] == -164
    worst_s.update(ships=0x1000)
    assert call(s=_state(**worst_s), d=_dst(**worst_s), **worst)[0] == -5
    assert call(s=_state(state_f64=1), d=_dst(**worst_s), **worst)[0] == -165
    assert call(s=_state(state_f64=1), d=_dst(state_f64=1), **worst)[0] == -166


# ---------------------------------------------------------------------------
# check_ids

def test_check_ids_accepts():
    # the 1 -> 6 fan-out into another batch
    s, d = fork.check_ids(4, 24, np.repeat(np.arange(4), 6), np.arange(24), False)
    assert s.dtype == d.dtype == np.int32 and s.tolist() == [0] * 6 + [1] * 6 + [2] * 6 + [3] * 6
    assert d.tolist() == list(range(24))
    # a fan-out inside one batch: the sources are no destinations
    s, d = fork.check_ids(77, 77, [3, 3, 3, 70], [10, 11, 12, 0], True)
    assert s.tolist() == [3, 3, 3, 70] and d.tolist() == [10, 11, 12, 0]
    # the identity, in all its spellings; on the same arrays every pair is a no-op
    for same in (False, True):
        s, d = fork.check_ids(5, 5, None, None, same)
        assert s.tolist() == d.tolist() == [0, 1, 2, 3, 4]
    assert [a.tolist() for a in fork.check_ids(5, 3, None, None, False)] == [[0, 1, 2]] * 2
    assert [a.tolist() for a in fork.check_ids(5, 9, None, [4, 8], False)] == [[0, 1], [4, 8]]
    assert [a.tolist() for a in fork.check_ids(5, 9, [4, 4], None, False)] == [[4, 4], [0, 1]]
    # overlap between two batches is no overlap: a permutation
    assert [a.tolist() for a in fork.check_ids(3, 3, [0, 1, 2], [1, 2, 0], False)] == [[0, 1, 2], [1, 2, 0]]
    # tensors, tuples, ranges, empty
    assert fork.check_ids(8, 8, torch.tensor([1, 2]), (5, 6), True)[1].tolist() == [5, 6]
    assert fork.check_ids(8, 8, range(2), range(4, 6), True)[0].tolist() == [0, 1]
    assert [a.size for a in fork.check_ids(8, 8, [], [], True)] == [0, 0]
    # a pair onto itself next to others
    assert fork.check_ids(8, 8, [2, 5], [2, 6], True)[1].tolist() == [2, 6]


def test_check_ids_rejects():
    with pytest.raises(ValueError, match='unequal'):
        fork.check_ids(8, 8, [1, 2, 3], [4, 5], False)
    for s, d in (([0, 8], [1, 2]), ([-1, 0], [1, 2])):
        with pytest.raises(ValueError, match='src_ids.*out of range'):
            fork.check_ids(8, 16, s, d, False)
    for s, d in (([0, 1], [1, 16]), ([0, 1], [-2, 3])):
        with pytest.raises(ValueError, match='dst_ids.*out of range'):
            fork.check_ids(8, 16, s, d, False)
    with pytest.raises(ValueError, match='dst_ids.*out of range'):
        fork.check_ids(8, 4, [5, 5, 5, 5, 5], None, False)     # the identity of five pairs names destination 4 of 4
    for same in (False, True):
        with pytest.raises(ValueError, match='duplicate'):
            fork.check_ids(8, 8, [0, 1, 2], [5, 6, 5], same)
    # the same arrays: a destination that is another pair's source -- a swap, a chain, a shift
    for s, d in (([0, 1], [1, 0]), ([0, 1], [1, 2]), ([0, 1, 2], [1, 2, 3]), ([4, 4, 2], [2, 5, 6]),
                 ([2, 2], [2, 6])):
        with pytest.raises(ValueError, match='overlap'):
            fork.check_ids(8, 8, s, d, True)
        fork.check_ids(8, 8, s, d, False)
    with pytest.raises(ValueError, match='integers'):
        fork.check_ids(8, 8, [0.5], [1], False)
    with pytest.raises(ValueError, match='one-dimensional'):
        fork.check_ids(8, 8, [[0]], [[1]], False)


# ---------------------------------------------------------------------------
# the Fork plan's checks: before any device call

def _bare_env(config=DEFAULT_CONFIG, S=2, n_env=20, p_pad=4, b_cap=32, dtype=torch.float32, device='cuda:0',
              planets_only=0):
    """A BatchedEnv that was never initialised: the checks read its shape only."""
    env = BatchedEnv.__new__(BatchedEnv)
    env.config, env.S, env.n_env, env.p_pad, env.b_cap, env.dtype = config, S, n_env, p_pad, b_cap, dtype
    env.device, env.planets_only = torch.device(device), planets_only
    return env


def test_fork_plan_value_errors_before_the_device():
    a = _bare_env()
    for kw, word in ((dict(p_pad=8), 'p_pad'), (dict(b_cap=48), 'b_cap'), (dict(dtype=torch.float64), 'dtype'),
                     (dict(config=SOLO_CONFIG, S=1), 'S'), (dict(config=DEFAULT_CONFIG._replace(dt=0.01)), 'config'),
                     (dict(planets_only=3), 'planets_only'), (dict(device='cuda:1'), 'device')):
        with pytest.raises(ValueError, match='differ in %s' % word):
            fork.Fork(a, _bare_env(**kw))
        with pytest.raises(ValueError, match='differ in %s' % word):
            BatchedEnv.fork_from(_bare_env(**kw), a)
    b = _bare_env(n_env=30)
    with pytest.raises(ValueError, match='game, the stream or both'):
        fork.Fork(a, b, game=False, stream=False)
    with pytest.raises(ValueError, match='duplicate'):
        fork.Fork(a, b, [0, 1], [7, 7])
    with pytest.raises(ValueError, match='out of range'):
        fork.Fork(a, b, [20], [0])
    with pytest.raises(ValueError, match='out of range'):
        fork.Fork(b, a, [0], [20])
    with pytest.raises(ValueError, match='unequal'):
        fork.Fork(a, b, [0], [1, 2])
    with pytest.raises(ValueError, match='overlap'):
        fork.Fork(a, a, [0, 1], [1, 2])
    with pytest.raises(ValueError, match='snapshot'):
        BatchedEnv.restore(a, b)
    # Lookahead's own arguments, before it builds its scratch env
    for kw, word in ((dict(ship=2), 'ship'), (dict(ship=-1), 'ship'), (dict(horizon=0), 'horizon')):
        with pytest.raises(ValueError, match=word):
            fork.Lookahead(a, **kw)
