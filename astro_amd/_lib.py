"""ctypes binding of the project's shared libraries, one row of ``LIBS`` each:

    key     library              header (include/)
    hip     libastro_hip.so      astro_step.h
    qnet    libastro_qnet.so     astro_qnet.h
    qtrain  libastro_qtrain.so   astro_qtrain.h
    replay  libastro_replay.so   astro_replay.h
    actor   libastro_actor.so    astro_actor.h
    qopt    libastro_qopt.so     astro_qopt.h
    qduel   libastro_qduel.so    astro_qduel.h
    qpool   libastro_qpool.so    astro_qpool.h
    trace   libastro_trace.so    astro_trace.h
    seats   libastro_seats.so    astro_seats.h
    fork    libastro_fork.so     astro_fork.h

The libraries are built in-tree by ``__graft_entry__.build()`` (hipcc
--offload-arch=gfx950).  There is no fallback: if a library is missing or its
ABI version differs, every entry point of it raises.  tests/test_libraries.py
checks every row against its header and its built library.

``LIBS`` is this module's own table: every row's struct mirrors and symbol
table live here.  A module that carries its binding itself registers its row
in ``MORE`` with ``register`` (astro_amd/search.py: libastro_search.so,
astro_search.h); ``row(key)`` finds a row of either and ``rows()`` lists both.
``LATER`` is a third table of the same kind, filled by ``register_later``
(astro_amd/es.py: libastro_es.so, astro_es.h): ``row(key)`` finds its rows too,
``all_rows()`` is ``rows()`` plus them, and ``build()`` compiles ``all_rows()``.
A key is taken once across the three tables.
"""
import collections
import ctypes
import os

# torch before any library is loaded: they bind to the HIP runtime already in the process
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

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
QNET_HIDDEN = 32
_QNET_SYMBOLS = {
    'astro_qnet_abi_version': (ctypes.c_int, []),
    'astro_qnet_last_error': (ctypes.c_char_p, []),
    'astro_qvalues': (ctypes.c_int, [ctypes.POINTER(AstroParams), ctypes.POINTER(AstroState),
                                     ctypes.POINTER(AstroQNet), ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.POINTER(AstroPolicy), ctypes.c_double, ctypes.c_void_p]),
}

# libastro_qtrain.so: the training half, again a library of its own (include/astro_qtrain.h)
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
_ACTOR_SYMBOLS = {
    'astro_actor_abi_version': (ctypes.c_int, []),
    'astro_actor_last_error': (ctypes.c_char_p, []),
    'astro_explore': (ctypes.c_int, [ctypes.POINTER(AstroParams), ctypes.POINTER(AstroState),
                                     ctypes.POINTER(AstroExplore), ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    'astro_episodes': (ctypes.c_int, [ctypes.POINTER(AstroEpisodes), ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_void_p]),
}


class AstroQOpt(ctypes.Structure):
    """include/astro_qopt.h AstroQOpt: the hyperparameters of one optimiser step."""
    _fields_ = [
        ('kind', ctypes.c_int32),
        ('nesterov', ctypes.c_int32),
        ('lr', ctypes.c_float),
        ('weight_decay', ctypes.c_float),
        ('max_norm', ctypes.c_float),
        ('momentum', ctypes.c_float),
        ('alpha', ctypes.c_float),
        ('one_minus_alpha', ctypes.c_float),
        ('beta1', ctypes.c_float),
        ('one_minus_beta1', ctypes.c_float),
        ('beta2', ctypes.c_float),
        ('one_minus_beta2', ctypes.c_float),
        ('step_size', ctypes.c_float),
        ('bc2', ctypes.c_float),
        ('eps', ctypes.c_float),
        ('tau', ctypes.c_float),
    ]


QOPT_KINDS = {'sgd': 0, 'rmsprop': 1, 'adagrad': 2, 'adam': 3}   # include/astro_qopt.h ASTRO_QOPT_*
QOPT_MAX_PARAMS = 1 << 20
QOPT_THREADS = 1024

# libastro_qopt.so: the optimiser step, a library of its own (include/astro_qopt.h)
_QOPT_SYMBOLS = {
    'astro_qopt_abi_version': (ctypes.c_int, []),
    'astro_qopt_last_error': (ctypes.c_char_p, []),
    'astro_qopt_step': (ctypes.c_int, [ctypes.POINTER(AstroQOpt), ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_void_p]),
}


# libastro_qduel.so: one Q-network per ship, a library of its own (include/astro_qduel.h)
_QDUEL_SYMBOLS = {
    'astro_qduel_abi_version': (ctypes.c_int, []),
    'astro_qduel_last_error': (ctypes.c_char_p, []),
    'astro_qvalues_ships': (ctypes.c_int, [ctypes.POINTER(AstroParams), ctypes.POINTER(AstroState),
                                           ctypes.POINTER(ctypes.POINTER(AstroQNet)), ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.POINTER(AstroPolicy), ctypes.c_double, ctypes.c_int32,
                                           ctypes.c_void_p]),
}


class AstroQSpan(ctypes.Structure):
    """include/astro_qpool.h AstroQSpan: ship ``ship`` of the envs [lo, hi) is played by nets[net]."""
    _fields_ = [
        ('ship', ctypes.c_int32),
        ('net', ctypes.c_int32),
        ('lo', ctypes.c_int32),
        ('hi', ctypes.c_int32),
    ]


QPOOL_MAX_NETS = 32     # include/astro_qpool.h ASTRO_QPOOL_MAX_NETS
QPOOL_MAX_SPANS = 64    # ASTRO_QPOOL_MAX_SPANS

# libastro_qpool.so: a pool of Q-networks over blocks of envs, a library of its own (include/astro_qpool.h)
_QPOOL_SYMBOLS = {
    'astro_qpool_abi_version': (ctypes.c_int, []),
    'astro_qpool_last_error': (ctypes.c_char_p, []),
    'astro_qvalues_pool': (ctypes.c_int, [ctypes.POINTER(AstroParams), ctypes.POINTER(AstroState),
                                          ctypes.POINTER(AstroQNet), ctypes.c_int32, ctypes.POINTER(AstroQSpan),
                                          ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.POINTER(AstroPolicy), ctypes.c_double, ctypes.c_int32,
                                          ctypes.c_void_p]),
}


class AstroTrace(ctypes.Structure):
    """include/astro_trace.h AstroTrace: the trace ring's arrays and shape."""
    _fields_ = [
        ('ids', ctypes.c_void_p),
        ('ships', ctypes.c_void_p),
        ('ships_b', ctypes.c_void_p),
        ('planets', ctypes.c_void_p),
        ('bullets', ctypes.c_void_p),
        ('hdr', ctypes.c_void_p),
        ('control', ctypes.c_void_p),
        ('q', ctypes.c_void_p),
        ('reward', ctypes.c_void_p),
        ('done', ctypes.c_void_p),
        ('m', ctypes.c_int32),
        ('ticks', ctypes.c_int32),
        ('nout', ctypes.c_int32),
        ('reserved', ctypes.c_int32),
    ]


TRACE_MAX_OUT = 6       # include/astro_trace.h ASTRO_TRACE_MAX_OUT

# libastro_trace.so: whole games of chosen envs recorded on the device, a library of its own (include/astro_trace.h)
_TRACE_SYMBOLS = {
    'astro_trace_abi_version': (ctypes.c_int, []),
    'astro_trace_last_error': (ctypes.c_char_p, []),
    'astro_trace_state': (ctypes.c_int, [ctypes.POINTER(AstroParams), ctypes.POINTER(AstroState),
                                         ctypes.POINTER(AstroTrace), ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p]),
    'astro_trace_result': (ctypes.c_int, [ctypes.POINTER(AstroTrace), ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]),
}


class AstroSeat(ctypes.Structure):
    """include/astro_seats.h AstroSeat: ship ``ship`` of the envs [lo, hi) is played by bot ``bot`` (a value of
    BOTS, or -1: skipped), a script bot with these two arguments."""
    _fields_ = [
        ('ship', ctypes.c_int32),
        ('bot', ctypes.c_int32),
        ('lo', ctypes.c_int32),
        ('hi', ctypes.c_int32),
        ('script_r2', ctypes.c_double),
        ('script_threshold', ctypes.c_double),
    ]


SEATS_MAX = 64          # include/astro_seats.h ASTRO_SEATS_MAX

# libastro_seats.so: scripted bots with their own arguments per ship and env block, a library of its own
# (include/astro_seats.h)
_SEATS_SYMBOLS = {
    'astro_seats_abi_version': (ctypes.c_int, []),
    'astro_seats_last_error': (ctypes.c_char_p, []),
    'astro_controls_seats': (ctypes.c_int, [ctypes.POINTER(AstroParams), ctypes.POINTER(AstroState),
                                            ctypes.POINTER(AstroPolicy), ctypes.POINTER(AstroSeat), ctypes.c_int32,
                                            ctypes.c_void_p, ctypes.c_void_p]),
}


FORK_GAME, FORK_STREAM = 1, 2    # include/astro_fork.h ASTRO_FORK_GAME / ASTRO_FORK_STREAM

# libastro_fork.so: env state copied between slots on the device, a library of its own (include/astro_fork.h)
_FORK_SYMBOLS = {
    'astro_fork_abi_version': (ctypes.c_int, []),
    'astro_fork_last_error': (ctypes.c_char_p, []),
    'astro_fork': (ctypes.c_int, [ctypes.POINTER(AstroParams), ctypes.POINTER(AstroState), ctypes.POINTER(AstroState),
                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]),
}


class AstroError(RuntimeError):
    pass


# One row per library: what __graft_entry__.build() compiles (csrc/<source> ->
# <file>) and what _load() checks.  env: the variable that names another build
# of the library (ASTRO_LIB: e.g. an A/B variant from tools/build_var.sh);
# handle: the module-level name that holds the loaded library.
Lib = collections.namedtuple('Lib', 'key file source env abi version error symbols path handle')


def _row(key, file, source, env, abi, prefix, symbols):
    return Lib(key, file, source, env, abi, prefix + 'abi_version', prefix + 'last_error', symbols,
               os.environ.get(env) or os.path.join(HERE, file), '_lib' if key == 'hip' else '_%s_lib' % key)


LIBS = collections.OrderedDict((r.key, r) for r in (
    _row('hip', 'libastro_hip.so', 'astro_kernels.hip', 'ASTRO_LIB', 21, 'astro_', _SYMBOLS),
    _row('qnet', 'libastro_qnet.so', 'astro_qnet.hip', 'ASTRO_QNET_LIB', 1, 'astro_qnet_', _QNET_SYMBOLS),
    _row('qtrain', 'libastro_qtrain.so', 'astro_qtrain.hip', 'ASTRO_QTRAIN_LIB', 1, 'astro_qtrain_', _QTRAIN_SYMBOLS),
    _row('replay', 'libastro_replay.so', 'astro_replay.hip', 'ASTRO_REPLAY_LIB', 1, 'astro_replay_', _REPLAY_SYMBOLS),
    _row('actor', 'libastro_actor.so', 'astro_actor.hip', 'ASTRO_ACTOR_LIB', 1, 'astro_actor_', _ACTOR_SYMBOLS),
    _row('qopt', 'libastro_qopt.so', 'astro_qopt.hip', 'ASTRO_QOPT_LIB', 1, 'astro_qopt_', _QOPT_SYMBOLS),
    _row('qduel', 'libastro_qduel.so', 'astro_qduel.hip', 'ASTRO_QDUEL_LIB', 1, 'astro_qduel_', _QDUEL_SYMBOLS),
    _row('qpool', 'libastro_qpool.so', 'astro_qpool.hip', 'ASTRO_QPOOL_LIB', 1, 'astro_qpool_', _QPOOL_SYMBOLS),
    _row('trace', 'libastro_trace.so', 'astro_trace.hip', 'ASTRO_TRACE_LIB', 1, 'astro_trace_', _TRACE_SYMBOLS),
    _row('seats', 'libastro_seats.so', 'astro_seats.hip', 'ASTRO_SEATS_LIB', 1, 'astro_seats_', _SEATS_SYMBOLS),
    _row('fork', 'libastro_fork.so', 'astro_fork.hip', 'ASTRO_FORK_LIB', 1, 'astro_fork_', _FORK_SYMBOLS),
))
LIB_PATH, ABI_VERSION = LIBS['hip'].path, LIBS['hip'].abi
QNET_LIB_PATH, QNET_ABI_VERSION = LIBS['qnet'].path, LIBS['qnet'].abi
QTRAIN_LIB_PATH, QTRAIN_ABI_VERSION = LIBS['qtrain'].path, LIBS['qtrain'].abi
REPLAY_LIB_PATH, REPLAY_ABI_VERSION = LIBS['replay'].path, LIBS['replay'].abi
ACTOR_LIB_PATH, ACTOR_ABI_VERSION = LIBS['actor'].path, LIBS['actor'].abi
QOPT_LIB_PATH, QOPT_ABI_VERSION = LIBS['qopt'].path, LIBS['qopt'].abi
QDUEL_LIB_PATH, QDUEL_ABI_VERSION = LIBS['qduel'].path, LIBS['qduel'].abi
QPOOL_LIB_PATH, QPOOL_ABI_VERSION = LIBS['qpool'].path, LIBS['qpool'].abi
TRACE_LIB_PATH, TRACE_ABI_VERSION = LIBS['trace'].path, LIBS['trace'].abi
SEATS_LIB_PATH, SEATS_ABI_VERSION = LIBS['seats'].path, LIBS['seats'].abi
FORK_LIB_PATH, FORK_ABI_VERSION = LIBS['fork'].path, LIBS['fork'].abi

# rows registered by the modules that hold their own binding (see the module docstring)
MORE = collections.OrderedDict()


# rows registered after ``rows()`` was fixed as LIBS + MORE: listed by ``all_rows()`` only
LATER = collections.OrderedDict()


def row(key):
    """The row of ``LIBS``, ``MORE`` or ``LATER`` with this key."""
    for table in (LIBS, MORE):
        if key in table:
            return table[key]
    return LATER[key]


def rows():
    """Every row, ``LIBS``' first."""
    return list(LIBS.values()) + list(MORE.values())


def all_rows():
    """Every row of the three tables: ``rows()``, then ``LATER``'s."""
    return rows() + list(LATER.values())


def _register(table, key, file, source, env, abi, prefix, symbols):
    if key in LIBS or key in MORE or key in LATER:
        raise ValueError('the library key %r is taken' % key)
    table[key] = _row(key, file, source, env, abi, prefix, symbols)
    globals()[table[key].handle] = None
    return _public(key)


def register(key, file, source, env, abi, prefix, symbols):
    """Add a row to ``MORE`` (once per key) and return its public (load, check) pair."""
    return _register(MORE, key, file, source, env, abi, prefix, symbols)


def register_later(key, file, source, env, abi, prefix, symbols):
    """Add a row to ``LATER`` (once per key across the three tables) and return its public (load, check) pair."""
    return _register(LATER, key, file, source, env, abi, prefix, symbols)


# the loaded libraries (tools/ab.py sets _lib back to None to load another build)
_lib = _qnet_lib = _qtrain_lib = _replay_lib = _actor_lib = None
_qopt_lib = _qduel_lib = _qpool_lib = _trace_lib = _seats_lib = _fork_lib = None


def _load(key, path):
    """The library of LIBS[key], loaded from `path` and typed on the first call.  Raises if
    it is absent or stale."""
    L = row(key)
    lib = globals()[L.handle]
    if lib is not None:
        return lib
    if not os.path.exists(path):
        raise AstroError('%s is missing: build it with `python -c "import __graft_entry__ as g; '
                         'g.build()"` (hipcc --offload-arch=gfx950)' % path)
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    # (ASTRO_AB_ANY_ABI=1: tools/ab.py timing an older build of the main library, which
    # lacks the entry points it predates and whose structs are a prefix of these -- never
    # for results)
    ab_any = key == 'hip' and os.environ.get('ASTRO_AB_ANY_ABI') == '1'
    for name, (res, args) in L.symbols.items():
        if ab_any and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    v = getattr(lib, L.version)()
    if v != L.abi and not (ab_any and 12 <= v <= L.abi):
        raise AstroError('%s ABI %d != expected %d (rebuild)' % (L.file, v, L.abi))
    globals()[L.handle] = lib
    return lib


def _check(key, rc, what):
    """Raise the library's last error for the entry point `what` that returned rc != 0."""
    msg = getattr(_load(key, row(key).path), row(key).error)().decode(errors='replace')
    raise AstroError('%s failed (%d): %s' % (what, rc, msg))


def _public(key):
    """The library's public pair; what a call per step pays is one lookup and one compare."""
    loaded, handle = globals(), row(key).handle

    def load(path=row(key).path):
        lib = loaded[handle]
        return lib if lib is not None else _load(key, path)

    def check(rc, what):
        if rc != 0:
            _check(key, rc, what)
    return load, check


load, check = _public('hip')
load_qnet, check_qnet = _public('qnet')
load_qtrain, check_qtrain = _public('qtrain')
load_replay, check_replay = _public('replay')
load_actor, check_actor = _public('actor')
load_qopt, check_qopt = _public('qopt')
load_qduel, check_qduel = _public('qduel')
load_qpool, check_qpool = _public('qpool')
load_trace, check_trace = _public('trace')
load_seats, check_seats = _public('seats')
load_fork, check_fork = _public('fork')


def stream_ptr(device):
    """torch's current stream on `device` as the void * the entry points take."""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
