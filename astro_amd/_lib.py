"""ctypes binding of libastro_hip.so (include/astro_step.h), of
libastro_qnet.so (include/astro_qnet.h), of libastro_qtrain.so
(include/astro_qtrain.h), of libastro_replay.so (include/astro_replay.h) and of
libastro_actor.so (include/astro_actor.h).

The shared library is built in-tree by ``__graft_entry__.build()``
(hipcc --offload-arch=gfx950).  There is no fallback: if the library is
missing or its ABI version differs, every entry point raises.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# (ASTRO_LIB: another build of the same library, e.g. an A/B variant from tools/build_var.sh)
LIB_PATH = os.environ.get('ASTRO_LIB') or os.path.join(HERE, 'libastro_hip.so')
ABI_VERSION = 21

STAT_NAMES = ('bullets_in', 'bullets_out', 'resets', 'collisions', 'timeouts',
              'overflows', 'planets', 'serial_resets')
NSTATS = 8
KERNELS = {'auto': 0, 'lane': 1, 'quad': 2, 'pair': 3}
MEM = {'default': 0, 'finegrained': 1, 'uncached': 2}   # include/astro_step.h ASTRO_MEM_*
ERRORS = {1: 'a helper wave never saw its step wave post (its finished games were not re-created)',
          2: "a step wave never saw its helper's header read"}


class AstroParams(ctypes.Structure):
    _fields_ = [
        ('gm', ctypes.c_double),
        ('dt', ctypes.c_double),
        ('db', ctypes.c_double),
        ('thrust', ctypes.c_double),
        ('r2_ss', ctypes.c_double),
        ('r2_sp', ctypes.c_double),
        ('r2_s0', ctypes.c_double),
        ('r2_p0', ctypes.c_double),
        ('gravity', ctypes.c_double),
        ('planet_mass', ctypes.c_double),
        ('spawn_off', ctypes.c_float),
        ('bullet_speed', ctypes.c_float),
        ('timeout_reward', ctypes.c_float),
        ('outer_pos', ctypes.c_float),
        ('inner_pos', ctypes.c_float),
        ('planet_orbit', ctypes.c_float),
        ('nships', ctypes.c_int32),
        ('solo', ctypes.c_int32),
        ('max_planets', ctypes.c_int32),
        ('p_pad', ctypes.c_int32),
        ('b_cap', ctypes.c_int32),
        ('timeout_tick', ctypes.c_int32),
        ('fire_bits', ctypes.c_void_p),
        ('kernel', ctypes.c_int32),
        ('planets_only', ctypes.c_int32),
        ('key_table', ctypes.c_void_p),
    ]


class AstroState(ctypes.Structure):
    _fields_ = [
        ('ships', ctypes.c_void_p),
        ('ships_b', ctypes.c_void_p),
        ('planets', ctypes.c_void_p),
        ('bullets', ctypes.c_void_p),
        ('hdr', ctypes.c_void_p),
        ('stream', ctypes.c_void_p),
        ('stream_ring', ctypes.c_void_p),
        ('n_env', ctypes.c_int32),
        ('state_f64', ctypes.c_int32),
        ('errors', ctypes.c_void_p),
    ]


class AstroPolicy(ctypes.Structure):
    _fields_ = [
        ('kind', ctypes.c_int32),
        ('bots', ctypes.c_int32),
        ('seed', ctypes.c_uint64),
        ('tick0', ctypes.c_int64),
        ('env_offset', ctypes.c_int64),
        ('script_r2', ctypes.c_double),
        ('script_threshold', ctypes.c_double),
        ('ship_thrust', ctypes.c_double),
        ('ship_rspeed', ctypes.c_double),
        ('bullet_speed', ctypes.c_double),
        ('ship_radius', ctypes.c_double),
    ]


class AstroGameTick(ctypes.Structure):
    """include/astro_step.h AstroGameTick: one game's tick (astro_game_step)."""
    _fields_ = [
        ('params', AstroParams),
        ('state', AstroState),
        ('stream', ctypes.c_void_p),
        ('hdr', ctypes.c_void_p),
        ('ships', ctypes.c_void_p),
        ('ships_b', ctypes.c_void_p),
        ('planets', ctypes.c_void_p),
        ('bullets', ctypes.c_void_p),
        ('control', ctypes.c_void_p),
        ('fire', ctypes.c_void_p),
        ('reward', ctypes.c_void_p),
        ('done', ctypes.c_void_p),
        ('errors', ctypes.c_void_p),
        ('control_dev', ctypes.c_void_p),
        ('fire_dev', ctypes.c_void_p),
        ('reward_dev', ctypes.c_void_p),
        ('done_dev', ctypes.c_void_p),
        ('in_', ctypes.c_void_p),
        ('out', ctypes.c_void_p),
        ('nplanets', ctypes.c_int32),
        ('nbullets', ctypes.c_int32),
        ('control0', ctypes.c_int32),
        ('control1', ctypes.c_int32),
        ('first_step', ctypes.c_int32),
        ('fire_now', ctypes.c_int32),
        ('timeout_now', ctypes.c_int32),
        ('out_nbullets', ctypes.c_int32),
        ('done_out', ctypes.c_int32),
        ('reward_out', ctypes.c_float * 2),
        ('flag', ctypes.c_void_p),
        ('flag_dev', ctypes.c_void_p),
        ('seq', ctypes.c_uint32),
        ('reserved', ctypes.c_int32),
    ]


POLICIES = {'control': 0, 'nothing': 1, 'random': 2, 'bots': 3}
BOTS = {'nothing': 0, 'script': 1, 'random': 2}

_SYMBOLS = {
    'astro_abi_version': (ctypes.c_int, []),
    'astro_last_error': (ctypes.c_char_p, []),
    'astro_step': (ctypes.c_int, [ctypes.POINTER(AstroParams), ctypes.POINTER(AstroState),
                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                  ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]),
    'astro_step_many': (ctypes.c_int, [ctypes.POINTER(AstroParams), ctypes.POINTER(AstroState),
                                       ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]),
    'astro_reset': (ctypes.c_int, [ctypes.POINTER(AstroParams), ctypes.POINTER(AstroState),
                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'astro_stream_init': (ctypes.c_int, [ctypes.POINTER(AstroState), ctypes.c_void_p,
                                         ctypes.c_void_p]),
    'astro_keytable_build': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                                            ctypes.c_void_p]),
    'astro_controls': (ctypes.c_int, [ctypes.POINTER(AstroParams), ctypes.POINTER(AstroState),
                                      ctypes.POINTER(AstroPolicy), ctypes.c_void_p, ctypes.c_void_p]),
    'astro_features': (ctypes.c_int, [ctypes.POINTER(AstroParams), ctypes.POINTER(AstroState),
                                      ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]),
    'astro_host_alloc': (ctypes.c_int, [ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p),
                                        ctypes.POINTER(ctypes.c_void_p)]),
    'astro_host_free': (ctypes.c_int, [ctypes.c_void_p]),
    'astro_dev_alloc': (ctypes.c_int, [ctypes.c_uint64, ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p)]),
    'astro_dev_free': (ctypes.c_int, [ctypes.c_void_p]),
    'astro_game_step': (ctypes.c_int, [ctypes.c_void_p]),
    'astro_rollout': (ctypes.c_int, [ctypes.POINTER(AstroParams), ctypes.POINTER(AstroState),
                                     ctypes.POINTER(AstroPolicy), ctypes.c_int32, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                     ctypes.c_void_p]),
}



class AstroQNet(ctypes.Structure):
    """include/astro_qnet.h AstroQNet: the packed Q-network of astro_qvalues."""
    _fields_ = [
        ('weights', ctypes.c_void_p),
        ('nships', ctypes.c_int32),
        ('nout', ctypes.c_int32),
    ]


# libastro_qnet.so: a library of its own (libastro_hip.so and _SYMBOLS stay what they are)
QNET_LIB_PATH = os.environ.get('ASTRO_QNET_LIB') or os.path.join(HERE, 'libastro_qnet.so')
QNET_ABI_VERSION = 1
QNET_HIDDEN = 32
_QNET_SYMBOLS = {
    'astro_qnet_abi_version': (ctypes.c_int, []),
    'astro_qnet_last_error': (ctypes.c_char_p, []),
    'astro_qvalues': (ctypes.c_int, [ctypes.POINTER(AstroParams), ctypes.POINTER(AstroState),
                                     ctypes.POINTER(AstroQNet), ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.POINTER(AstroPolicy), ctypes.c_double, ctypes.c_void_p]),
}

# libastro_qtrain.so: the training half, again a library of its own (include/astro_qtrain.h)
QTRAIN_LIB_PATH = os.environ.get('ASTRO_QTRAIN_LIB') or os.path.join(HERE, 'libastro_qtrain.so')
QTRAIN_ABI_VERSION = 1
_QTRAIN_SYMBOLS = {
    'astro_qtrain_abi_version': (ctypes.c_int, []),
    'astro_qtrain_last_error': (ctypes.c_char_p, []),
    'astro_qforward': (ctypes.c_int, [ctypes.POINTER(AstroQNet), ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'astro_qgrad_workspace_bytes': (ctypes.c_size_t, [ctypes.POINTER(AstroQNet), ctypes.c_int32]),
    'astro_qgrad': (ctypes.c_int, [ctypes.POINTER(AstroQNet), ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
}



class AstroReplay(ctypes.Structure):
    """include/astro_replay.h AstroReplay: the replay ring's arrays and shape."""
    _fields_ = [
        ('features', ctypes.c_void_p),
        ('action', ctypes.c_void_p),
        ('reward', ctypes.c_void_p),
        ('discount', ctypes.c_void_p),
        ('next', ctypes.c_void_p),
        ('loss', ctypes.c_void_p),
        ('wstart', ctypes.c_void_p),
        ('gpow', ctypes.c_void_p),
        ('gamma', ctypes.c_double),
        ('n_env', ctypes.c_int32),
        ('rows', ctypes.c_int32),
        ('nships', ctypes.c_int32),
        ('ticks', ctypes.c_int32),
        ('n_steps', ctypes.c_int32),
        ('reserved', ctypes.c_int32),
    ]


# libastro_replay.so: the experience replay, a library of its own (include/astro_replay.h)
REPLAY_LIB_PATH = os.environ.get('ASTRO_REPLAY_LIB') or os.path.join(HERE, 'libastro_replay.so')
REPLAY_ABI_VERSION = 1
_REPLAY_SYMBOLS = {
    'astro_replay_abi_version': (ctypes.c_int, []),
    'astro_replay_last_error': (ctypes.c_char_p, []),
    'astro_replay_push': (ctypes.c_int, [ctypes.POINTER(AstroReplay), ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p]),
    'astro_replay_sample_workspace_bytes': (ctypes.c_size_t, [ctypes.POINTER(AstroReplay)]),
    'astro_replay_sample': (ctypes.c_int, [ctypes.POINTER(AstroReplay), ctypes.c_int64, ctypes.c_int32, ctypes.c_uint64,
                                           ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_size_t, ctypes.c_void_p]),
    'astro_replay_gather': (ctypes.c_int, [ctypes.POINTER(AstroReplay), ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p]),
    'astro_replay_update': (ctypes.c_int, [ctypes.POINTER(AstroReplay), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                           ctypes.c_void_p]),
}



class AstroExplore(ctypes.Structure):
    """include/astro_actor.h AstroExplore: the sticky exploration's state and constants."""
    _fields_ = [
        ('policy', ctypes.c_void_p),
        ('stay_out', ctypes.c_uint64),
        ('stay_in', ctypes.c_uint64),
        ('seed', ctypes.c_uint64),
        ('env_offset', ctypes.c_int64),
        ('nrandom', ctypes.c_int32),
        ('reserved', ctypes.c_int32),
    ]


class AstroEpisodes(ctypes.Structure):
    """include/astro_actor.h AstroEpisodes: the per-game bookkeeping's arrays."""
    _fields_ = [
        ('length', ctypes.c_void_p),
        ('got', ctypes.c_void_p),
        ('winner', ctypes.c_void_p),
        ('ticks', ctypes.c_void_p),
        ('wins', ctypes.c_void_p),
        ('finished', ctypes.c_void_p),
        ('tick_sum', ctypes.c_void_p),
        ('n_env', ctypes.c_int32),
        ('nships', ctypes.c_int32),
        ('games', ctypes.c_int32),
        ('reserved', ctypes.c_int32),
    ]


# libastro_actor.so: exploration and episode bookkeeping, a library of its own (include/astro_actor.h)
ACTOR_LIB_PATH = os.environ.get('ASTRO_ACTOR_LIB') or os.path.join(HERE, 'libastro_actor.so')
ACTOR_ABI_VERSION = 1
_ACTOR_SYMBOLS = {
    'astro_actor_abi_version': (ctypes.c_int, []),
    'astro_actor_last_error': (ctypes.c_char_p, []),
    'astro_explore': (ctypes.c_int, [ctypes.POINTER(AstroParams), ctypes.POINTER(AstroState),
                                     ctypes.POINTER(AstroExplore), ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    'astro_episodes': (ctypes.c_int, [ctypes.POINTER(AstroEpisodes), ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_void_p]),
}

_lib = None
_qnet_lib = None
_qtrain_lib = None
_replay_lib = None
_actor_lib = None


class AstroError(RuntimeError):
    pass


def load(path=LIB_PATH):
    """Load (once) and type the library.  Raises if it is absent or stale."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise AstroError('%s is missing: build it with `python -c "import __graft_entry__ as g; '
                         'g.build()"` (hipcc --offload-arch=gfx950)' % path)
    # torch first: the library binds to the HIP runtime already in the process
    import torch  # noqa: F401
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    ab_any = os.environ.get('ASTRO_AB_ANY_ABI') == '1'
    for name, (res, args) in _SYMBOLS.items():
        if ab_any and not hasattr(lib, name):   # (an older A/B build: entry points it predates)
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    v = lib.astro_abi_version()
    # (ASTRO_AB_ANY_ABI=1: tools/ab.py timing an older build whose structs are a
    # prefix of these -- never for results)
    if v != ABI_VERSION and not (os.environ.get('ASTRO_AB_ANY_ABI') == '1' and 12 <= v <= ABI_VERSION):
        raise AstroError('libastro_hip.so ABI %d != expected %d (rebuild)' % (v, ABI_VERSION))
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().astro_last_error().decode(errors='replace')
        raise AstroError('%s failed (%d): %s' % (what, rc, msg))


def load_qnet(path=QNET_LIB_PATH):
    """Load (once) and type libastro_qnet.so.  Raises if it is absent or stale."""
    global _qnet_lib
    if _qnet_lib is not None:
        return _qnet_lib
    if not os.path.exists(path):
        raise AstroError('%s is missing: build it with `python -c "import __graft_entry__ as g; '
                         'g.build()"` (hipcc --offload-arch=gfx950)' % path)
    import torch  # noqa: F401
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    for name, (res, args) in _QNET_SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    v = lib.astro_qnet_abi_version()
    if v != QNET_ABI_VERSION:
        raise AstroError('libastro_qnet.so ABI %d != expected %d (rebuild)' % (v, QNET_ABI_VERSION))
    _qnet_lib = lib
    return lib


def check_qnet(rc, what):
    if rc != 0:
        msg = load_qnet().astro_qnet_last_error().decode(errors='replace')
        raise AstroError('%s failed (%d): %s' % (what, rc, msg))


def load_qtrain(path=QTRAIN_LIB_PATH):
    """Load (once) and type libastro_qtrain.so.  Raises if it is absent or stale."""
    global _qtrain_lib
    if _qtrain_lib is not None:
        return _qtrain_lib
    if not os.path.exists(path):
        raise AstroError('%s is missing: build it with `python -c "import __graft_entry__ as g; '
                         'g.build()"` (hipcc --offload-arch=gfx950)' % path)
    import torch  # noqa: F401
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    for name, (res, args) in _QTRAIN_SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    v = lib.astro_qtrain_abi_version()
    if v != QTRAIN_ABI_VERSION:
        raise AstroError('libastro_qtrain.so ABI %d != expected %d (rebuild)' % (v, QTRAIN_ABI_VERSION))
    _qtrain_lib = lib
    return lib


def check_qtrain(rc, what):
    if rc != 0:
        msg = load_qtrain().astro_qtrain_last_error().decode(errors='replace')
        raise AstroError('%s failed (%d): %s' % (what, rc, msg))


def load_replay(path=REPLAY_LIB_PATH):
    """Load (once) and type libastro_replay.so.  Raises if it is absent or stale."""
    global _replay_lib
    if _replay_lib is not None:
        return _replay_lib
    if not os.path.exists(path):
        raise AstroError('%s is missing: build it with `python -c "import __graft_entry__ as g; '
                         'g.build()"` (hipcc --offload-arch=gfx950)' % path)
    import torch  # noqa: F401
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    for name, (res, args) in _REPLAY_SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    v = lib.astro_replay_abi_version()
    if v != REPLAY_ABI_VERSION:
        raise AstroError('libastro_replay.so ABI %d != expected %d (rebuild)' % (v, REPLAY_ABI_VERSION))
    _replay_lib = lib
    return lib


def check_replay(rc, what):
    if rc != 0:
        msg = load_replay().astro_replay_last_error().decode(errors='replace')
        raise AstroError('%s failed (%d): %s' % (what, rc, msg))


def load_actor(path=ACTOR_LIB_PATH):
    """Load (once) and type libastro_actor.so.  Raises if it is absent or stale."""
    global _actor_lib
    if _actor_lib is not None:
        return _actor_lib
    if not os.path.exists(path):
        raise AstroError('%s is missing: build it with `python -c "import __graft_entry__ as g; '
                         'g.build()"` (hipcc --offload-arch=gfx950)' % path)
    import torch  # noqa: F401
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    for name, (res, args) in _ACTOR_SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    v = lib.astro_actor_abi_version()
    if v != ACTOR_ABI_VERSION:
        raise AstroError('libastro_actor.so ABI %d != expected %d (rebuild)' % (v, ACTOR_ABI_VERSION))
    _actor_lib = lib
    return lib


def check_actor(rc, what):
    if rc != 0:
        msg = load_actor().astro_actor_last_error().decode(errors='replace')
        raise AstroError('%s failed (%d): %s' % (what, rc, msg))
