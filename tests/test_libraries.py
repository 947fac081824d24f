"""CPU-only checks of the library table (astro_amd._lib.LIBS) and of every
row's binding, one parametrised case per library: the header's declarations,
the symbol table and the built library's exports are one set; the header
compiles alone as C99; every struct of the header has a ctypes mirror of the
same layout; every prototype agrees with its restype and argtypes; the
header's constants are the Python ones; __graft_entry__.build_lib's
dependencies are the headers the source reaches.  A library added to LIBS is
covered without an edit here: the literal pins below are compared as a prefix
or per known key, so a row they do not know gets every comparison between its
header, its mirrors and its library, but no literal pin until one is added."""
import ctypes
import os
import re
import subprocess

import pytest

import __graft_entry__ as entry
from astro_amd import _lib, actor, env, optim, qnet, replay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, 'include')
CSRC = os.path.join(ROOT, 'astro_amd', 'csrc')
ALL = list(_lib.LIBS)

# ---------------------------------------------------------------------------
# the literal pins

KEYS = ['hip', 'qnet', 'qtrain', 'replay', 'actor', 'qopt', 'qduel', 'qpool', 'trace']

# key: (file, source, env, abi, version, error, handle)
ROWS = {
    'hip': ('libastro_hip.so', 'astro_kernels.hip', 'ASTRO_LIB', 21, 'astro_abi_version', 'astro_last_error', '_lib'),
    'qnet': ('libastro_qnet.so', 'astro_qnet.hip', 'ASTRO_QNET_LIB', 1, 'astro_qnet_abi_version',
             'astro_qnet_last_error', '_qnet_lib'),
    'qtrain': ('libastro_qtrain.so', 'astro_qtrain.hip', 'ASTRO_QTRAIN_LIB', 1, 'astro_qtrain_abi_version',
               'astro_qtrain_last_error', '_qtrain_lib'),
    'replay': ('libastro_replay.so', 'astro_replay.hip', 'ASTRO_REPLAY_LIB', 1, 'astro_replay_abi_version',
               'astro_replay_last_error', '_replay_lib'),
    'actor': ('libastro_actor.so', 'astro_actor.hip', 'ASTRO_ACTOR_LIB', 1, 'astro_actor_abi_version',
              'astro_actor_last_error', '_actor_lib'),
    'qopt': ('libastro_qopt.so', 'astro_qopt.hip', 'ASTRO_QOPT_LIB', 1, 'astro_qopt_abi_version',
             'astro_qopt_last_error', '_qopt_lib'),
    'qduel': ('libastro_qduel.so', 'astro_qduel.hip', 'ASTRO_QDUEL_LIB', 1, 'astro_qduel_abi_version',
              'astro_qduel_last_error', '_qduel_lib'),
    'qpool': ('libastro_qpool.so', 'astro_qpool.hip', 'ASTRO_QPOOL_LIB', 1, 'astro_qpool_abi_version',
              'astro_qpool_last_error', '_qpool_lib'),
    'trace': ('libastro_trace.so', 'astro_trace.hip', 'ASTRO_TRACE_LIB', 1, 'astro_trace_abi_version',
              'astro_trace_last_error', '_trace_lib'),
}

EXPORTS = {
    'hip': {'astro_abi_version', 'astro_last_error', 'astro_step', 'astro_step_many', 'astro_reset',
            'astro_stream_init', 'astro_keytable_build', 'astro_features', 'astro_rollout', 'astro_controls',
            'astro_host_alloc', 'astro_host_free', 'astro_dev_alloc', 'astro_dev_free', 'astro_game_step'},
    'qnet': {'astro_qnet_abi_version', 'astro_qnet_last_error', 'astro_qvalues'},
    'qtrain': {'astro_qtrain_abi_version', 'astro_qtrain_last_error', 'astro_qforward', 'astro_qgrad_workspace_bytes',
               'astro_qgrad'},
    'replay': {'astro_replay_abi_version', 'astro_replay_last_error', 'astro_replay_push',
               'astro_replay_sample_workspace_bytes', 'astro_replay_sample', 'astro_replay_gather',
               'astro_replay_update'},
    'actor': {'astro_actor_abi_version', 'astro_actor_last_error', 'astro_explore', 'astro_episodes'},
    'qopt': {'astro_qopt_abi_version', 'astro_qopt_last_error', 'astro_qopt_step'},
    'qduel': {'astro_qduel_abi_version', 'astro_qduel_last_error', 'astro_qvalues_ships'},
    'qpool': {'astro_qpool_abi_version', 'astro_qpool_last_error', 'astro_qvalues_pool'},
    'trace': {'astro_trace_abi_version', 'astro_trace_last_error', 'astro_trace_state', 'astro_trace_result'},
}

SIZES = {'AstroQOpt': 64, 'AstroQSpan': 16}

# source: the basenames of dependencies(source)
DEPENDENCIES = {
    'astro_kernels.hip': {'astro_kernels.hip', 'astro_step.h', 'astro_common.h'},
    'astro_qnet.hip': {'astro_qnet.hip', 'astro_qnet.h', 'astro_step.h', 'astro_common.h', 'astro_qfwd.h'},
    'astro_qtrain.hip': {'astro_qtrain.hip', 'astro_qtrain.h', 'astro_qnet.h', 'astro_step.h', 'astro_common.h'},
    'astro_replay.hip': {'astro_replay.hip', 'astro_replay.h', 'astro_common.h'},
    'astro_actor.hip': {'astro_actor.hip', 'astro_actor.h', 'astro_step.h', 'astro_common.h'},
    'astro_qopt.hip': {'astro_qopt.hip', 'astro_qopt.h', 'astro_common.h'},
    'astro_qduel.hip': {'astro_qduel.hip', 'astro_qduel.h', 'astro_qnet.h', 'astro_step.h', 'astro_common.h',
                        'astro_qfwd.h'},
    'astro_qpool.hip': {'astro_qpool.hip', 'astro_qpool.h', 'astro_qnet.h', 'astro_step.h', 'astro_common.h',
                        'astro_qfwd.h'},
    'astro_trace.hip': {'astro_trace.hip', 'astro_trace.h', 'astro_step.h', 'astro_common.h'},
}
CSRC_HEADERS = ['astro_common.h', 'astro_qfwd.h']


def _named(prefix, table, rename=()):
    """(prefix + NAME, value) for every entry of a Python name table."""
    return [(prefix + dict(rename).get(k, k).upper(), v) for k, v in table.items()]


# key: (C expression over the header, the Python value that mirrors it); a name may come twice,
# with a second mirror or with the literal it is pinned to
CONSTANTS = {
    'hip': (_named('ASTRO_KERNEL_', _lib.KERNELS) + _named('ASTRO_MEM_', _lib.MEM)
            + _named('ASTRO_POLICY_', _lib.POLICIES) + _named('ASTRO_BOT_', _lib.BOTS)
            + _named('ASTRO_STAT_', {n: i for i, n in enumerate(_lib.STAT_NAMES)}, [('serial_resets', 'serial')])
            + [('ASTRO_NSTATS', _lib.NSTATS), ('ASTRO_NSTATS', len(_lib.STAT_NAMES)),
               ('ASTRO_QUAD_MAX_ENVS', env.QUAD_MAX_ENVS)]),
    'qnet': [('ASTRO_QNET_HIDDEN', _lib.QNET_HIDDEN), ('ASTRO_QNET_HIDDEN', qnet.HIDDEN), ('ASTRO_QNET_MAX_OUT', 6)],
    'qtrain': [('sizeof(AstroQNet)', ctypes.sizeof(_lib.AstroQNet))],
    'replay': [('ASTRO_REPLAY_NEXT_TERMINAL', replay.NEXT_TERMINAL), ('ASTRO_REPLAY_NEXT_PENDING', replay.NEXT_PENDING)],
    'actor': [('ASTRO_EXPLORE_ONE', actor.ONE), ('ASTRO_EXPLORE_ONE', 9007199254740992)],
    'qopt': (_named('ASTRO_QOPT_', _lib.QOPT_KINDS)
             + [('ASTRO_QOPT_MAX_PARAMS', _lib.QOPT_MAX_PARAMS), ('ASTRO_QOPT_THREADS', _lib.QOPT_THREADS),
                ('ASTRO_QOPT_THREADS', optim.THREADS), ('ASTRO_QOPT_THREADS', 1024)]),
    'qduel': [('ASTRO_QNET_HIDDEN', _lib.QNET_HIDDEN), ('ASTRO_QNET_MAX_OUT', 6),
              ('sizeof(AstroQNet)', ctypes.sizeof(_lib.AstroQNet))],
    'qpool': [('ASTRO_QPOOL_MAX_NETS', _lib.QPOOL_MAX_NETS), ('ASTRO_QPOOL_MAX_NETS', 32),
              ('ASTRO_QPOOL_MAX_SPANS', _lib.QPOOL_MAX_SPANS), ('ASTRO_QPOOL_MAX_SPANS', 64),
              ('sizeof(AstroQNet)', ctypes.sizeof(_lib.AstroQNet))],
    'trace': [('ASTRO_TRACE_MAX_OUT', _lib.TRACE_MAX_OUT), ('ASTRO_TRACE_MAX_OUT', 6)],
}
# every header name of these families has a mirror above
FAMILIES = r'ASTRO_(?:KERNEL|MEM|POLICY|BOT|STAT)_\w+|ASTRO_QOPT_(?:SGD|RMSPROP|ADAGRAD|ADAM)|ASTRO_\w+_MAX_(?:NETS|SPANS|OUT)'

# a second declaration with the binding's argument list compiles only if it is the header's prototype
REDECLARED = {
    'qduel': ['int astro_qvalues_ships(const AstroParams *, const AstroState *, const AstroQNet *const[2], float *,',
              '                        int8_t *, const AstroPolicy *, double, int32_t, void *);'],
    'qpool': ['int astro_qvalues_pool(const AstroParams *, const AstroState *, const AstroQNet *, int32_t,',
              '                       const AstroQSpan *, int32_t, float *, int8_t *, const AstroPolicy *, double,',
              '                       int32_t, void *);'],
    'trace': ['int astro_trace_state(const AstroParams *, const AstroState *, const AstroTrace *, int32_t,',
              '                      const int8_t *, const float *, void *);',
              'int astro_trace_result(const AstroTrace *, int32_t, const float *, const uint8_t *, int32_t, int32_t,',
              '                       void *);'],
}

SCALARS = {'int': ctypes.c_int, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'uint32_t': ctypes.c_uint32,
           'uint64_t': ctypes.c_uint64, 'size_t': ctypes.c_size_t, 'float': ctypes.c_float, 'double': ctypes.c_double}


# ---------------------------------------------------------------------------
# reading a header

def header_of(key):
    return os.path.join(INCLUDE, 'astro_step.h' if key == 'hip' else 'astro_%s.h' % key)


def text_of(key):
    """The header without its comments."""
    return re.sub(r'/\*.*?\*/|//[^\n]*', ' ', open(header_of(key)).read(), flags=re.S)


def prototypes(key):
    """{name: (result, [parameter, ...])} of the header's own astro_* declarations, as C text."""
    out = {}
    for res, name, params in re.findall(r'^[ \t]*([\w \t\*]+?)\b(astro_\w+)[ \t]*\(([^)]*)\)\s*;', text_of(key), re.M):
        assert name not in out, name
        params = [' '.join(p.split()) for p in params.split(',')]
        out[name] = (' '.join(res.split()), [] if params == ['void'] else params)
    return out


def structs(key):
    """{name: [field, ...]} of the header's own `typedef struct ... AstroX;`, the fields in C order.
    A typedef that this does not parse (a nested brace) is an error, not a struct left unchecked."""
    out = {}
    for body, name in re.findall(r'typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;', text_of(key)):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(';'))):
            for piece in decl.split(','):
                fields.append(re.search(r'(\w+)\s*(?:\[\w*\])?\s*$', piece).group(1))
        out[name] = fields
    assert len(out) == len(re.findall(r'\btypedef\s+struct\b', text_of(key)))
    return out


def kind(ctype):
    """'pointer', or the scalar ctypes type itself."""
    if ctype in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(ctype, ctypes._Pointer):
        return 'pointer'
    return ctype


def c_kind(decl, named):
    """The same of a C parameter (named) or result type; an unknown type is an error."""
    if '*' in decl or '[' in decl:
        return 'pointer'
    words = [w for w in decl.split() if w != 'const']
    if named and len(words) == 2:
        words.pop()
    assert len(words) == 1 and words[0] in SCALARS, 'unknown C type: %r' % decl
    return SCALARS[words[0]]


def run_c(key, tmp_path, body, extra=()):
    """Compile (C99, every warning an error) and run a program that includes only the row's header."""
    src, exe = str(tmp_path / 'probe.c'), str(tmp_path / 'probe')
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "%s"' % os.path.basename(header_of(key))]
    with open(src, 'w') as f:
        f.write('\n'.join(lines + list(extra) + ['int main(void){'] + body + ['return 0;}', '']))
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I', INCLUDE, src, '-o', exe])
    return [int(x) for x in subprocess.check_output([exe], text=True).split()]


@pytest.fixture(scope='module')
def built():
    """Every library, compiled as entry.build() compiles it.  Not build() itself: that ends by checking
    every row's ABI at once, so one wrong row would fail the case of every row instead of its own."""
    for key in _lib.LIBS:
        entry.build_lib(key)


# ---------------------------------------------------------------------------
# the table

def test_the_table_is_one_ordered_table():
    assert list(_lib.LIBS)[:9] == KEYS
    rows = list(_lib.LIBS.values())
    for field in ('file', 'source', 'env', 'handle'):
        assert len({getattr(r, field) for r in rows}) == len(rows), field
    assert set(ROWS) == set(EXPORTS) == set(KEYS) and set(DEPENDENCIES) == {r[1] for r in ROWS.values()}


@pytest.mark.parametrize('key', ALL)
def test_table_row(key):
    row = _lib.LIBS[key]
    assert row.key == key and type(row) is _lib.Lib
    assert hasattr(_lib, row.handle)
    assert set(row.symbols) >= {row.version, row.error}
    assert row.path == os.environ.get(row.env) or row.path == os.path.join(ROOT, 'astro_amd', row.file)
    if key in ROWS:
        assert (row.file, row.source, row.env, row.abi, row.version, row.error, row.handle) == ROWS[key]


@pytest.mark.parametrize('key', ALL)
def test_module_names_are_the_tables_objects(key):
    row = _lib.LIBS[key]
    prefix = '' if key == 'hip' else key.upper() + '_'
    assert getattr(_lib, prefix + 'LIB_PATH') is row.path
    assert getattr(_lib, prefix + 'ABI_VERSION') is row.abi
    assert getattr(_lib, '_' + prefix + 'SYMBOLS') is row.symbols
    suffix = '' if key == 'hip' else '_' + key
    assert callable(getattr(_lib, 'load' + suffix)) and callable(getattr(_lib, 'check' + suffix))


# ---------------------------------------------------------------------------
# exports, layout, prototypes, constants

@pytest.mark.parametrize('key', ALL)
def test_header_symbols_and_exports_are_one_set(key, built):
    row = _lib.LIBS[key]
    declared = set(prototypes(key))
    out = subprocess.check_output(['nm', '-D', '--defined-only', row.path], text=True)
    exported = set(re.findall(r' T (astro_\w+)$', out, re.M))
    assert declared == set(row.symbols)
    assert exported == declared, sorted(exported ^ declared)
    if key in EXPORTS:
        assert declared == EXPORTS[key]
    lib = _lib._load(key, row.path)
    for name in declared:
        getattr(lib, name)
    (abi,) = re.findall(r'^[ \t]*#[ \t]*define[ \t]+ASTRO_\w*ABI_VERSION[ \t]+(\d+)', text_of(key), re.M)
    assert int(abi) == row.abi == getattr(lib, row.version)()


@pytest.mark.parametrize('key', ALL)
def test_struct_layouts_are_the_ctypes_mirrors(key, tmp_path):
    """Also the case that shows the header compiles alone as C99 with -Wall -Werror."""
    found = structs(key)
    body, expect = [], []
    for name, c_fields in found.items():
        mirror = getattr(_lib, name, None)
        assert mirror is not None and issubclass(mirror, ctypes.Structure), '%s has no ctypes mirror' % name
        fields = [f for f, _ in mirror._fields_]
        assert [f.rstrip('_') for f in fields] == c_fields, name
        body.append('printf("%%zu\\n", sizeof(%s));' % name)
        expect.append(ctypes.sizeof(mirror))
        for f in fields:
            body.append('printf("%%zu\\n", offsetof(%s, %s));' % (name, f.rstrip('_')))
            expect.append(getattr(mirror, f).offset)
        if name in SIZES:
            assert ctypes.sizeof(mirror) == SIZES[name]
    assert run_c(key, tmp_path, body) == expect


def test_every_ctypes_structure_is_a_struct_of_one_header():
    found = [name for key in ALL for name in structs(key)]
    mirrors = [n for n, v in vars(_lib).items() if isinstance(v, type) and issubclass(v, ctypes.Structure)]
    assert sorted(found) == sorted(mirrors) and set(SIZES) <= set(found)


@pytest.mark.parametrize('key', ALL)
def test_prototypes_agree_with_restype_and_argtypes(key, tmp_path):
    row = _lib.LIBS[key]
    protos = prototypes(key)
    assert set(protos) == set(row.symbols)
    for name, (res, params) in protos.items():
        restype, argtypes = row.symbols[name]
        assert c_kind(res, False) == kind(restype), name
        assert len(params) == len(argtypes), name
        for i, (p, a) in enumerate(zip(params, argtypes)):
            assert c_kind(p, True) == kind(a), (name, i, p, a)
    run_c(key, tmp_path, [], REDECLARED.get(key, ()))


@pytest.mark.parametrize('key', ALL)
def test_header_constants_are_the_python_ones(key, tmp_path):
    (abi,) = re.findall(r'^[ \t]*#[ \t]*define[ \t]+(ASTRO_\w*ABI_VERSION)\b', text_of(key), re.M)
    pairs = CONSTANTS.get(key, []) + [(abi, _lib.LIBS[key].abi)]
    mirrored = {expr for expr, _ in pairs}
    own = re.sub(r'#[ \t]*include[^\n]*', ' ', text_of(key))
    assert set(re.findall(r'\b(?:%s)\b' % FAMILIES, own)) <= mirrored
    got = run_c(key, tmp_path, ['printf("%%lld\\n", (long long)(%s));' % expr for expr, _ in pairs])
    assert got == [int(v) for _, v in pairs], [(e, v, g) for (e, v), g in zip(pairs, got) if int(v) != g]


def test_error_bits_are_the_keys_of_errors(tmp_path):
    names = re.findall(r'\b(ASTRO_ERR_[A-Z_]+)\s*=', text_of('hip'))
    got = run_c('hip', tmp_path, ['printf("%%d\\n", %s);' % n for n in names])
    assert len(names) == len(set(names)) and sorted(got) == sorted(_lib.ERRORS)


# ---------------------------------------------------------------------------
# dependencies and staleness

def reachable(path, headers, seen):
    """The project headers (basename -> path) that `path` reaches, by a walk of its own."""
    for line in open(path):
        m = re.match(r'\s*#\s*include\s*"([^"]+)"', line)
        if m and m.group(1) in headers and headers[m.group(1)] not in seen:
            seen.add(headers[m.group(1)])
            reachable(headers[m.group(1)], headers, seen)
    return seen


@pytest.mark.parametrize('key', ALL)
def test_dependencies_are_the_headers_the_source_reaches(key):
    headers = {}
    for d in (INCLUDE, CSRC):
        headers.update((f, os.path.join(d, f)) for f in os.listdir(d) if f.endswith('.h'))
    assert sorted(f for f in os.listdir(CSRC) if f.endswith('.h')) == CSRC_HEADERS
    assert len(headers) == len(os.listdir(INCLUDE)) + len(CSRC_HEADERS)   # no name twice
    row = _lib.LIBS[key]
    src = os.path.join(CSRC, row.source)
    deps = entry.dependencies(src)
    assert len(deps) == len(set(deps))
    assert set(deps) == {src} | reachable(src, headers, set())
    assert (entry.INCLUDE, entry.CSRC) == (INCLUDE, CSRC)
    assert os.path.exists(header_of(key)) and header_of(key) in deps
    assert headers['astro_common.h'] in deps
    if row.source in DEPENDENCIES:
        assert {os.path.basename(d) for d in deps} == DEPENDENCIES[row.source]


def test_a_header_reached_through_another_header_only():
    src = os.path.join(CSRC, _lib.LIBS['qtrain'].source)
    assert '"astro_qnet.h"' not in open(src).read() and os.path.join(INCLUDE, 'astro_qnet.h') in entry.dependencies(src)


def test_the_forward_is_stated_once():
    """The forward's helpers are astro_qfwd.h's: no Q-network source states them again."""
    for name in ('astro_qnet.hip', 'astro_qduel.hip', 'astro_qpool.hip'):
        text = open(os.path.join(CSRC, name)).read()
        assert not re.search(r'\bfloat\s+softsign\b|\bstruct\s+WaveLds\b|\bstruct\s+Explore\b', text), name


def test_a_newer_dependency_makes_the_library_stale(tmp_path):
    out, a, b = (str(tmp_path / n) for n in ('lib.so', 'a.hip', 'b.h'))
    for f in (a, b):
        open(f, 'w').close()
    assert entry.stale(out, [a, b])             # no library yet
    open(out, 'w').close()
    for f, t in ((a, 100), (b, 100), (out, 200)):
        os.utime(f, (t, t))
    assert not entry.stale(out, [a, b])
    os.utime(b, (200, 200))                     # as old as the library: not newer
    assert not entry.stale(out, [a, b])
    os.utime(b, (201, 201))
    assert entry.stale(out, [a, b]) and entry.stale(out, [b]) and not entry.stale(out, [a])
