"""CPU-only checks of the one table behind the five libraries (astro_amd._lib.LIBS):
__graft_entry__.build_lib's dependencies come from the sources' own #include
lines, its staleness rule, and _lib's module-level names are the table's objects."""
import os
import re

import pytest

import __graft_entry__ as entry
from astro_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('hip', 'qnet', 'qtrain', 'replay', 'actor')


def reachable(path, headers, seen):
    """The project headers (basename -> path) that `path` reaches, by a walk of its own."""
    for line in open(path):
        m = re.match(r'\s*#\s*include\s*"([^"]+)"', line)
        if m and m.group(1) in headers and headers[m.group(1)] not in seen:
            seen.add(headers[m.group(1)])
            reachable(headers[m.group(1)], headers, seen)
    return seen


def test_the_table_is_the_five_libraries():
    assert tuple(_lib.LIBS) == KEYS
    assert [L.key for L in _lib.LIBS.values()] == list(KEYS)
    assert len({L.file for L in _lib.LIBS.values()}) == len({L.source for L in _lib.LIBS.values()}) == 5


@pytest.mark.parametrize('key', KEYS)
def test_dependencies_are_the_headers_the_source_reaches(key):
    headers = {}
    for d in (os.path.join(ROOT, 'include'), os.path.join(ROOT, 'astro_amd', 'csrc')):
        headers.update((f, os.path.join(d, f)) for f in os.listdir(d) if f.endswith('.h'))
    assert len(headers) == len(os.listdir(os.path.join(ROOT, 'include'))) + 2   # no name twice; csrc has two headers
    src = os.path.join(ROOT, 'astro_amd', 'csrc', _lib.LIBS[key].source)
    deps = entry.dependencies(src)
    assert len(deps) == len(set(deps))
    assert set(deps) == {src} | reachable(src, headers, set())
    assert headers['astro_common.h'] in deps
    assert os.path.join(ROOT, 'include', 'astro_step.h' if key != 'replay' else 'astro_replay.h') in deps
    if key == 'qtrain':   # a header reached through another header only
        assert '"astro_qnet.h"' not in open(src).read() and headers['astro_qnet.h'] in deps


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


@pytest.mark.parametrize('key', KEYS)
def test_module_names_are_the_tables_objects(key):
    L = _lib.LIBS[key]
    prefix = '' if key == 'hip' else key.upper() + '_'
    assert getattr(_lib, prefix + 'LIB_PATH') is L.path
    assert getattr(_lib, prefix + 'ABI_VERSION') is L.abi
    assert getattr(_lib, '_' + prefix + 'SYMBOLS') is L.symbols
    assert L.path == os.environ.get(L.env) or L.path == os.path.join(ROOT, 'astro_amd', L.file)
    assert set(L.symbols) >= {L.version, L.error}
