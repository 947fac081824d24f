"""An antithetic evolution strategy for a packed Q-network (libastro_es.so,
include/astro_es.h): a gradient-free optimiser of the weights that follows the
outcome of games instead of a surrogate loss.

``perturb`` / ``score`` / ``gradient``   the checked device calls (astro_es_perturb,
                  astro_es_score, astro_es_gradient), one launch each
``noise_host`` / ``perturb_host`` / ``score_host`` / ``utilities_host`` /
``gradient_host`` the numpy mirrors, in the header's float32 / float64
                  operations and order: the kernels equal them bit for bit
``Population``    a centre network and 2 * pairs perturbed members, rows of one
                  tensor, each row a ``QNetwork`` of its own: a ``Pool`` or
                  ``Seats`` built once follows every ``perturb``
``ESTrainer``     the loop: perturb, play the members against an opponent on
                  blocks of one env (``league.Seats``, ``actor.Episodes``),
                  score, estimate the gradient, ``optim`` step

The noise of (seed, generation, pair, parameter) is a function of those four
alone (the header's THE NOISE): nothing of it is stored, and ``gradient``
regenerates what ``perturb`` used.  Member 2 j is ``theta + sigma * eps_j``,
member 2 j + 1 ``theta - sigma * eps_j``.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .replay import random_words


class AstroES(ctypes.Structure):
    """include/astro_es.h AstroES: one population's shape, step size and noise key."""
    _fields_ = [
        ('seed', ctypes.c_uint64),
        ('generation', ctypes.c_int64),
        ('nparams', ctypes.c_int32),
        ('pairs', ctypes.c_int32),
        ('sigma', ctypes.c_float),
        ('reserved', ctypes.c_int32),
    ]


ABI_VERSION = 1             # include/astro_es.h ASTRO_ES_ABI_VERSION
MAX_PAIRS = 512             # ASTRO_ES_MAX_PAIRS
MAX_MEMBERS = 1024          # ASTRO_ES_MAX_MEMBERS
MAX_PARAMS = 1 << 20        # ASTRO_ES_MAX_PARAMS
SHAPINGS = {'ranks': 0, 'raw': 1}   # ASTRO_ES_RANKS, ASTRO_ES_RAW
NOISE_MEAN = 131070         # of the sum of four 16-bit fields
NOISE_SCALE = np.float32(float.fromhex('0x1.bb67aep-16'))   # float32(sqrt(3 / (2^32 - 1)))
M64 = (1 << 64) - 1

SYMBOLS = {
    'astro_es_abi_version': (ctypes.c_int, []),
    'astro_es_last_error': (ctypes.c_char_p, []),
    'astro_es_perturb': (ctypes.c_int, [ctypes.POINTER(AstroES), ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                        ctypes.c_void_p, ctypes.c_void_p]),
    'astro_es_score': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                      ctypes.c_int32, ctypes.c_double, ctypes.c_double, ctypes.c_int32,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'astro_es_gradient': (ctypes.c_int, [ctypes.POINTER(AstroES), ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p]),
}

# The library's row.  _lib.LIBS and _lib.rows() are fixed tables; this row joins through _lib.LATER, which
# build() compiles (_lib.all_rows()) and _lib.row() finds.
load, check = _lib.register_later('es', 'libastro_es.so', 'astro_es.hip', 'ASTRO_ES_LIB', ABI_VERSION, 'astro_es_',
                                  SYMBOLS)
ROW = _lib.row('es')


# ---------------------------------------------------------------------------
# the numpy mirrors

def noise_host(seed, generation, first_pair, npairs, nparams):
    """eps of the pairs [first_pair, first_pair + npairs): float32 [npairs, nparams]."""
    j = np.arange(int(first_pair), int(first_pair) + int(npairs), dtype=np.uint64)[:, None]
    p = np.arange(int(nparams), dtype=np.uint64)[None, :]
    z = random_words((j << np.uint64(32)) | p, int(seed) & M64, int(generation) & M64)
    s = np.zeros(z.shape, np.int64)
    for shift in (0, 16, 32, 48):
        s += ((z >> np.uint64(shift)) & np.uint64(0xffff)).astype(np.int64)
    return (s - NOISE_MEAN).astype(np.float32) * NOISE_SCALE


def perturb_host(theta, sigma, seed, generation, first_pair, npairs):
    """astro_es_perturb's rows: float32 [2 * npairs, nparams]."""
    theta = np.asarray(theta, np.float32).ravel()
    d = np.float32(sigma) * noise_host(seed, generation, first_pair, npairs, theta.size)
    out = np.empty((2 * int(npairs), theta.size), np.float32)
    out[0::2] = theta[None, :] + d
    out[1::2] = theta[None, :] - d
    return out


def blocks(n_env, nmembers):
    """[(lo, hi)] of the members' env blocks: ``Pool.versus``'."""
    N, K = int(n_env), int(nmembers)
    return [(k * N // K, (k + 1) * N // K) for k in range(K)]


def score_host(winner, ticks, nmembers, ship=0, draw=0.0, survive=0.0, timeout_tick=1):
    """astro_es_score: (counts int32 [K, 3], lost_ticks int64 [K], fitness float32 [K])."""
    winner, ticks = np.asarray(winner), np.asarray(ticks)
    K, T = int(nmembers), int(timeout_tick)
    counts, lost, fit = np.zeros((K, 3), np.int32), np.zeros(K, np.int64), np.full(K, np.nan, np.float32)
    for k, (lo, hi) in enumerate(blocks(winner.shape[0], K)):
        w, t = winner[lo:hi].astype(np.int64).ravel(), ticks[lo:hi].astype(np.int64).ravel()
        won, none = w == int(ship), w == -1
        loss = ~won & ~none & (w != -2)
        W, L, D = int(won.sum()), int(loss.sum()), int(none.sum())
        lt = int(np.minimum(t[loss], T).sum())
        counts[k], lost[k] = (W, L, D), lt
        if W + L + D:
            a = float(W - L) + float(draw) * float(D)
            b = float(survive) * (float(lt) / float(T))
            fit[k] = np.float32((a + b) / float(W + L + D))
    return counts, lost, fit


def _shaping(shaping):
    if shaping not in SHAPINGS:
        raise ValueError('shaping must be one of %s, got %r' % (sorted(SHAPINGS), shaping))
    return SHAPINGS[shaping]


def utilities_host(fitness, shaping='ranks'):
    """astro_es_gradient's utilities: float32 [K]."""
    raw = _shaping(shaping) == SHAPINGS['raw']
    f = np.asarray(fitness, np.float32).ravel()
    K = f.size
    if K < 2 or K % 2:
        raise ValueError('fitness must hold 2 * pairs values, got %d' % K)
    if not np.isfinite(f).all():
        return np.zeros(K, np.float32)
    if raw:
        return f.copy()
    less = (f[None, :] < f[:, None]).sum(1)
    equal = (f[None, :] == f[:, None]).sum(1) - 1
    return (2 * less + equal).astype(np.float32) / np.float32(2 * (K - 1)) - np.float32(0.5)


def gradient_host(fitness, nparams, sigma, seed, generation, shaping='ranks'):
    """astro_es_gradient's gradient: float32 [nparams]."""
    u = utilities_host(fitness, shaping)
    pairs = u.size // 2
    du = u[0::2] - u[1::2]                       # float32
    a = np.zeros(int(nparams), np.float64)
    step = 64                                    # (the noise a few pairs at a time: it is never all in memory)
    for j0 in range(0, pairs, step):
        eps = noise_host(seed, generation, j0, min(step, pairs - j0), nparams).astype(np.float64)
        for i in range(eps.shape[0]):
            a = a + np.float64(du[j0 + i]) * eps[i]
    return (-a / ((2.0 * float(pairs)) * float(np.float32(sigma)))).astype(np.float32)


# ---------------------------------------------------------------------------
# the device calls

def _sigma_ok(sigma):
    with np.errstate(over='ignore'):
        s = np.float32(sigma)
    return bool(np.isfinite(s) and s > 0)


def _struct(nparams, pairs, sigma, seed, generation):
    nparams, pairs, sigma = int(nparams), int(pairs), float(sigma)
    if not 1 <= nparams <= MAX_PARAMS:
        raise ValueError('nparams must be in [1, %d], got %d' % (MAX_PARAMS, nparams))
    if not 1 <= pairs <= MAX_PAIRS:
        raise ValueError('pairs must be in [1, %d], got %d' % (MAX_PAIRS, pairs))
    if not _sigma_ok(sigma):
        raise ValueError('sigma must be finite and > 0 in float32, got %r' % sigma)
    g = int(generation)
    if not -(1 << 63) <= g < (1 << 63):
        raise ValueError('generation must fit an int64, got %d' % g)
    return AstroES(seed=int(seed) & M64, generation=g, nparams=nparams, pairs=pairs, sigma=sigma, reserved=0)


def _dev(t, dtype, shape, device, what):
    if (not torch.is_tensor(t) or t.dtype != dtype or t.device.type != 'cuda' or not t.is_contiguous()
            or (device is not None and t.device != device) or (shape is not None and tuple(t.shape) != tuple(shape))):
        raise ValueError('%s must be a contiguous %s %s tensor on %s'
                         % (what, str(dtype).replace('torch.', ''), 'x'.join(map(str, shape)) if shape else '',
                            device or 'a HIP device'))
    return t


def _ptr(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def perturb(theta, members, pairs, sigma, seed=0, generation=0, first_pair=0):
    """``members`` (float32 [2 * npairs, nparams]) becomes the + and - rows of
    the pairs [first_pair, first_pair + npairs) of a population of ``pairs``
    around ``theta`` (float32 [nparams], not written).  One launch on the
    current stream; returns ``members``."""
    if not torch.is_tensor(theta) or theta.dim() != 1:
        raise ValueError('theta must be a float32 [nparams] tensor')
    _dev(theta, torch.float32, None, None, 'theta')
    n = int(theta.shape[0])
    if not torch.is_tensor(members) or members.dim() != 2 or members.shape[0] % 2 or members.shape[1] != n:
        raise ValueError('members must be a float32 [2 * npairs, %d] tensor' % n)
    _dev(members, torch.float32, None, theta.device, 'members')
    npairs, first_pair = int(members.shape[0]) // 2, int(first_pair)
    c = _struct(n, pairs, sigma, seed, generation)
    if first_pair < 0 or first_pair + npairs > c.pairs:
        raise ValueError('the pairs [%d, %d) are not inside [0, %d)' % (first_pair, first_pair + npairs, c.pairs))
    check(load().astro_es_perturb(ctypes.byref(c), _ptr(theta), first_pair, npairs, _ptr(members),
                                  _lib.stream_ptr(theta.device)), 'astro_es_perturb')
    return members


def score(winner, ticks, nmembers, ship=0, draw=0.0, survive=0.0, timeout_tick=1, fitness=None, counts=None,
          lost_ticks=None):
    """``(fitness, counts, lost_ticks)`` of the members' env blocks from an
    ``actor.Episodes``' ``winner`` (int8 [N, G]) and ``ticks`` (int32 [N, G]).
    fitness: a float32 [K] tensor to fill, or None for a new one.  counts
    (int32 [K, 3]: W, L, D) and lost_ticks (int64 [K]): a tensor to fill, True
    for a new one, None (the default) not to compute it.  One launch."""
    if not torch.is_tensor(winner) or winner.dim() != 2:
        raise ValueError('winner must be an int8 [N, G] tensor')
    dev = winner.device
    _dev(winner, torch.int8, None, None, 'winner')
    _dev(ticks, torch.int32, tuple(winner.shape), dev, 'ticks')
    N, G, K = int(winner.shape[0]), int(winner.shape[1]), int(nmembers)
    if G < 1 or N * G > 2 ** 31 - 1:
        raise ValueError('winner must be [N, G] with G >= 1 and N * G within an int32, got %s' % (tuple(winner.shape),))
    if not 1 <= K <= MAX_MEMBERS:
        raise ValueError('nmembers must be in [1, %d], got %d' % (MAX_MEMBERS, K))
    if int(ship) not in (0, 1):
        raise ValueError('ship must be 0 or 1, got %r' % (ship,))
    if int(timeout_tick) < 1:
        raise ValueError('timeout_tick must be >= 1, got %r' % (timeout_tick,))
    if not (np.isfinite(draw) and np.isfinite(survive)):
        raise ValueError('draw and survive must be finite')
    fitness = torch.empty(K, dtype=torch.float32, device=dev) if fitness is None else \
        _dev(fitness, torch.float32, (K,), dev, 'fitness')
    if counts is not None:
        counts = torch.empty((K, 3), dtype=torch.int32, device=dev) if counts is True else \
            _dev(counts, torch.int32, (K, 3), dev, 'counts')
    if lost_ticks is not None:
        lost_ticks = torch.empty(K, dtype=torch.int64, device=dev) if lost_ticks is True else \
            _dev(lost_ticks, torch.int64, (K,), dev, 'lost_ticks')
    check(load().astro_es_score(_ptr(winner), _ptr(ticks), N, G, K, int(ship), float(draw), float(survive),
                                int(timeout_tick), _ptr(counts), _ptr(lost_ticks), fitness.data_ptr(),
                                _lib.stream_ptr(dev)), 'astro_es_score')
    return fitness, counts, lost_ticks


def gradient(fitness, nparams, sigma, seed=0, generation=0, shaping='ranks', utilities=None, out=None):
    """The gradient estimate (float32 [nparams]; ``out`` if given) from the
    fitness of 2 * pairs members (float32 [K], not written), for an optimiser
    that minimises.  utilities: a float32 [K] tensor to fill, True for a new
    one (the call then returns ``(grad, utilities)``), None not to store them.
    One launch."""
    mode = _shaping(shaping)
    if not torch.is_tensor(fitness) or fitness.dim() != 1 or fitness.shape[0] < 2 or fitness.shape[0] % 2:
        raise ValueError('fitness must be a float32 [2 * pairs] tensor')
    _dev(fitness, torch.float32, None, None, 'fitness')
    dev, K = fitness.device, int(fitness.shape[0])
    c = _struct(nparams, K // 2, sigma, seed, generation)
    out = torch.empty(c.nparams, dtype=torch.float32, device=dev) if out is None else \
        _dev(out, torch.float32, (c.nparams,), dev, 'out')
    if utilities is not None:
        utilities = torch.empty(K, dtype=torch.float32, device=dev) if utilities is True else \
            _dev(utilities, torch.float32, (K,), dev, 'utilities')
    check(load().astro_es_gradient(ctypes.byref(c), fitness.data_ptr(), mode, _ptr(utilities), out.data_ptr(),
                                   _lib.stream_ptr(dev)), 'astro_es_gradient')
    return out if utilities is None else (out, utilities)


# ---------------------------------------------------------------------------
# the population and the trainer

def _int(v, lo, what, hi=None):
    if isinstance(v, bool) or not isinstance(v, int) or v < lo or (hi is not None and v > hi):
        raise ValueError('%s must be an int %s, got %r' % (what, '>= %d' % lo if hi is None else 'in [%d, %d]' % (lo, hi), v))
    return v


class Population:
    """``net`` (a ``QNetwork``) is the centre: its packed buffer is ``theta``.
    ``members`` is one float32 [K, nparams] tensor, K = 2 * pairs <= 32 (a
    ``Pool``'s limit), and ``nets`` K ``QNetwork`` views of its rows.  The
    whole population has ``pairs * rounds`` pairs (at most 512), of which
    ``perturb(round)`` writes the pairs [round * pairs, (round + 1) * pairs)
    into ``members``.  ``generation`` is the noise's draw: whoever steps the
    centre adds one."""

    def __init__(self, net, pairs, sigma, seed=0, rounds=1):
        from .qnet import QNetwork
        if not isinstance(net, QNetwork):
            raise ValueError('net must be a QNetwork')
        _int(pairs, 1, 'pairs', _lib.QPOOL_MAX_NETS // 2)
        _int(rounds, 1, 'rounds')
        if pairs * rounds > MAX_PAIRS:
            raise ValueError('pairs * rounds must be at most %d, got %d' % (MAX_PAIRS, pairs * rounds))
        if isinstance(sigma, bool) or not isinstance(sigma, (int, float)) or not _sigma_ok(sigma):
            raise ValueError('sigma must be finite and > 0 in float32, got %r' % (sigma,))
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError('seed must be an int, got %r' % (seed,))
        self.net, self.pairs, self.rounds, self.sigma, self.seed = net, pairs, rounds, float(sigma), seed
        self.total_pairs, self.K = pairs * rounds, 2 * pairs
        self.generation = 0
        self.theta = net.weights
        self.nparams = int(self.theta.numel())
        self.members = torch.empty((self.K, self.nparams), dtype=torch.float32, device=self.theta.device)
        self.members.copy_(self.theta[None, :].expand(self.K, self.nparams))
        self.nets = [QNetwork.view(self.members[k], net.nships, net.nout) for k in range(self.K)]

    def perturb(self, round=0):
        """One launch: ``members`` becomes this generation's pairs of ``round``."""
        if not 0 <= int(round) < self.rounds:
            raise ValueError('round must be in [0, %d), got %r' % (self.rounds, round))
        return perturb(self.theta, self.members, self.total_pairs, self.sigma, self.seed, self.generation,
                       int(round) * self.pairs)


class ESTrainer:
    """Evolution strategies for ``net`` on a two-ship ``env`` (auto-reset).

    A population of ``pairs * rounds`` antithetic pairs (at most 512) is
    evaluated in ``rounds`` passes of ``2 * pairs`` members: member k plays ship
    0 of env block k (``Pool.versus``' blocks) and ``opponent`` ship 1
    everywhere -- a bot's name, a ``league.Script``, a ``QNetwork``, or a list
    of those, spread over each block's envs the same way for every member.  The
    ``league.Seats`` is built once: the members' networks are views of the rows
    that ``perturb`` rewrites.

    common_games: before each pass block 0's envs, the game and the futures,
    are copied onto every other block (one ``fork.Fork`` plan), so every member
    plays the same games and an antithetic pair differs by its weights alone.
    Needs ``n_env`` divisible by ``2 * pairs`` and refuses 'random', whose
    controls are keyed by env id and not by the state.

    fitness (``score``): per member ``((W - L) + draw * D + survive * lost_ticks
    / timeout_tick) / (W + L + D)`` over its block's ``games`` games per env.
    ``update`` turns the ``[2 * pairs * rounds]`` fitness tensor into a gradient
    (``gradient``, ``shaping`` 'ranks' or 'raw') and applies ``optimizer`` (an
    ``astro_amd.optim`` rule; default ``SGD(lr)``) to ``net``.

    ``generation()`` is ``perturb(r)``, ``evaluate(r)`` for every round, then
    ``update()``; it returns the mean fitness as a device scalar."""

    def __init__(self, env, net, opponent='script', pairs=16, rounds=1, sigma=0.05, optimizer=None, lr=1e-2, games=1,
                 shaping='ranks', draw=0.0, survive=0.0, common_games=True, seed=0):
        from . import optim
        from .league import BOT_NAMES, Script, Seats
        from .qnet import QNetwork
        if env.S != 2:
            raise ValueError('ESTrainer needs a two-ship env')
        if not isinstance(net, QNetwork) or net.nships != env.S:
            raise ValueError('net must be a QNetwork for %d ships' % env.S)
        _int(pairs, 1, 'pairs', _lib.QPOOL_MAX_NETS // 2)
        _int(rounds, 1, 'rounds')
        if pairs * rounds > MAX_PAIRS:
            raise ValueError('pairs * rounds must be at most %d, got %d' % (MAX_PAIRS, pairs * rounds))
        _int(games, 1, 'games')
        _shaping(shaping)
        for name, v in (('draw', draw), ('survive', survive), ('lr', lr)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not np.isfinite(v):
                raise ValueError('%s must be a finite number, got %r' % (name, v))
        rivals = list(opponent) if isinstance(opponent, (list, tuple)) else [opponent]
        if not rivals:
            raise ValueError('opponent must name at least one rival')
        for r in rivals:
            if not (isinstance(r, (Script, QNetwork)) or (isinstance(r, str) and r in BOT_NAMES)):
                raise ValueError("opponent must be a QNetwork, a Script, one of 'script', 'nothing', 'random', or a "
                                 "list of those: %r" % (r,))
        K, N = 2 * pairs, env.n_env
        if N < K * len(rivals):
            raise ValueError('%d members with %d rivals each need at least %d envs, got %d'
                             % (K, len(rivals), K * len(rivals), N))
        if common_games:
            if N % K:
                raise ValueError('common_games needs n_env (%d) divisible by 2 * pairs (%d)' % (N, K))
            if any(isinstance(r, str) and r == 'random' for r in rivals):
                raise ValueError("common_games refuses the opponent 'random': its controls are keyed by env id, so "
                                 "copies of one game would be played differently")
        if optimizer is not None and not isinstance(optimizer, optim.Optimizer):
            raise ValueError('optimizer must be an astro_amd.optim rule')
        self.env, self.net, self.opponent, self.rivals = env, net, opponent, tuple(rivals)
        self.pairs, self.rounds, self.games, self.shaping = pairs, rounds, games, shaping
        self.draw, self.survive, self.common_games, self.seed = float(draw), float(survive), bool(common_games), seed
        # (everything above read the arguments only; from here on the device is used)
        self.pop = Population(net, pairs, sigma, seed, rounds)
        self.optimizer = optim.SGD(float(lr)) if optimizer is None else optimizer
        R = len(self.rivals)
        bounds = blocks(N, K)
        spans = [(0, lo, hi, k) for k, (lo, hi) in enumerate(bounds)]
        if R == 1:
            spans.append((1, 0, N, K))
        else:
            for lo, hi in bounds:
                B = hi - lo
                spans += [(1, lo + r * B // R, lo + (r + 1) * B // R, K + r) for r in range(R)]
        self.seats = Seats(env, tuple(self.pop.nets) + self.rivals, spans)
        self.plan = None
        if self.common_games:
            from .fork import Fork
            B = N // K
            dst = np.arange(B, N)
            self.plan = Fork(env, env, dst % B, dst)
        dev = env.device
        self.fitness = torch.full((K * rounds,), float('nan'), dtype=torch.float32, device=dev)
        self.grad = torch.zeros(self.pop.nparams, dtype=torch.float32, device=dev)
        self.episodes = None       # the last evaluate's
        self.ngen = 0              # generations so far
        self.last = None

    def perturb(self, round=0):
        """``pop.perturb(round)``: the members become the round's pairs."""
        return self.pop.perturb(round)

    def evaluate(self, round=0):
        """The members as they are play ``games`` games per env (``play_q``'s
        loop on the seats, after the fork with ``common_games``), and their
        fitness goes to the round's slice of ``fitness``.  Returns the
        ``actor.Episodes``."""
        if not 0 <= int(round) < self.rounds:
            raise ValueError('round must be in [0, %d), got %r' % (self.rounds, round))
        env, K = self.env, self.pop.K
        if self.plan is not None:
            self.plan.apply()
        ep = env._play_q(self.seats, None, self.games, None, None, self.seed)
        score(ep.winner, ep.ticks, K, 0, self.draw, self.survive, env.schedule.timeout_tick,
              fitness=self.fitness[int(round) * K:(int(round) + 1) * K])
        self.episodes = ep
        return ep

    def update(self):
        """``gradient`` of the whole fitness tensor, then ``optimizer.apply(net,
        grad)``; the population's generation advances."""
        pop = self.pop
        gradient(self.fitness, pop.nparams, pop.sigma, pop.seed, pop.generation, self.shaping, out=self.grad)
        self.optimizer.apply(self.net, self.grad)
        pop.generation += 1
        self.ngen += 1

    def generation(self):
        """One generation; the mean fitness as a device scalar.  Synchronises
        only where ``play_q`` does."""
        for r in range(self.rounds):
            self.perturb(r)
            self.evaluate(r)
        self.last = self.fitness.mean()
        self.update()
        return self.last

    def run(self, n):
        """``n`` generations; returns the last mean fitness (or None)."""
        out = None
        for _ in range(int(n)):
            out = self.generation()
        return out

    def validate(self, eval_env, games=1, opponent=None, record=None):
        """``QTrainer.validate``'s: the centre network plays greedily --
        ``eval_env.play_q(net, opponent, games)`` as
        ``actor.Episodes.summary()``.  Synchronises."""
        return eval_env._play_q(self.net, opponent, games, None, None, 0, record).summary()
