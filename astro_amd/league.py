"""Which of two bots is better: the reference's util.p_better / find_better
(util.py:169-214) without scipy, and ``compare``, which plays two Q-networks
against each other on a ``BatchedEnv`` (``play_q`` with a network opponent:
one astro_qvalues_ships launch per tick, include/astro_qduel.h).

``Pool`` describes which network plays which ship of which block of envs (one
astro_qvalues_pool launch per tick, include/astro_qpool.h), and ``tournament``
plays every ordered pairing of a list of networks on one env that way.

``Script`` is a ScriptBot's arguments as a value, and ``Seats`` is ``Pool`` with
scripted players next to the networks: every scripted seat has its own bot and
arguments (one astro_controls_seats launch per tick, include/astro_seats.h).
``tournament`` and ``compare`` take scripted members through it, and ``mutate``
/ ``tune_script`` are the reference's ``ScriptBot.mutate`` / ``optimize``
(script.py:93-127) played in blocks of envs.
"""
import ctypes

from . import _lib


def _tail(n, k):
    """P(Binomial(n, 1/2) <= k) for 0 <= k <= n, from Python integers (the
    division rounds once)."""
    term = total = 1                    # C(n, 0)
    for j in range(1, k + 1):
        term = term * (n - j + 1) // j  # C(n, j), exact
        total += term
    return total / (1 << n)


def p_better(nwins, nlosses):
    """util.p_better: the posterior probability that the win rate exceeds 1/2
    under a Beta(1 + nwins, 1 + nlosses), ``1 - beta.cdf(0.5, 1 + nwins, 1 +
    nlosses)``.  For integer parameters the regularised incomplete beta
    function is a binomial tail, so this is P(Binomial(nwins + nlosses + 1,
    1/2) <= nwins): a sum of binomial coefficients over a power of two.  The
    smaller tail is computed and, for nwins > nlosses, taken from 1, so that
    ``p_better(w, l) + p_better(l, w) == 1`` holds in floating point too."""
    w, l = int(nwins), int(nlosses)
    if w != nwins or l != nlosses or w < 0 or l < 0:
        raise ValueError('nwins and nlosses must be integers >= 0')
    n = w + l + 1
    return _tail(n, w) if w <= l else 1.0 - _tail(n, l)


def find_better(games, max_trials, threshold):
    """util.find_better: the better of two bots from a (lazy) sequence of
    winners (0, 1 or None per game, ``play``'s first result).  0 or 1 as soon
    as ``p_better`` of that side exceeds ``threshold``; None as soon as the
    trials left of ``max_trials`` cannot take either side there, or when the
    sequence ends undecided.  The sequence is consumed no further than the
    game that decides."""
    nwins0 = nwins1 = 0
    for n, winner in enumerate(games):
        nwins0 += (winner == 0)
        nwins1 += (winner == 1)
        p0 = p_better(nwins0, nwins1)
        if threshold < p0:
            return 0
        if threshold < 1 - p0:
            return 1
        left = max_trials - n - 1
        if p_better(nwins0 + left, nwins1) < threshold and 1 - p_better(nwins0, nwins1 + left) < threshold:
            return None
    return None


def compare(env, net_a, net_b, games=1, seed=0):
    """``net_a`` against ``net_b`` on ``env`` (two ships, auto-reset): every
    env plays its next ``games`` games with a as ship 0 and b as ship 1, then
    ``games`` more with the seats swapped, both greedy (``env.play_q``; seed is
    passed on to it).  Returns ``dict(games=, wins_a=, wins_b=, none=,
    p_better=)``: the games counted (2 * n_env * games), each network's wins
    over both seats, the games without a winner, and ``p_better(wins_a,
    wins_b)``.  Either side may be a ``Script`` or a bot's name ('script',
    'nothing', 'random'): the games are then played on ``Seats.versus``.
    Synchronises."""
    from .qnet import QNetwork
    if isinstance(net_a, QNetwork) and isinstance(net_b, QNetwork):
        first = env._play_q(net_a, net_b, games, None, None, seed).winner
        second = env._play_q(net_b, net_a, games, None, None, seed).winner
    else:
        first = env._play_q(Seats.versus(env, net_a, [net_b]), None, games, None, None, seed).winner
        second = env._play_q(Seats.versus(env, net_b, [net_a]), None, games, None, None, seed).winner
    wins_a = int((first == 0).sum()) + int((second == 1).sum())
    wins_b = int((first == 1).sum()) + int((second == 0).sum())
    total = int(first.numel() + second.numel())
    return dict(games=total, wins_a=wins_a, wins_b=wins_b, none=total - wins_a - wins_b,
                p_better=p_better(wins_a, wins_b))


class Pool:
    """Which network plays which ship of which envs: a checked, immutable
    description that ``BatchedEnv.qvalues`` / ``qcontrols`` / ``rollout_q`` /
    ``play_q`` take wherever they take the per-ship form (one
    astro_qvalues_pool launch, include/astro_qpool.h).

    nets: a sequence of 1..32 ``QNetwork``s on the env's device, for the env's
    number of ships and with equal nout.  spans: a sequence of 1..64 ``(ship,
    lo, hi, k)``: ship ``ship`` of the envs [lo, hi) is played by ``nets[k]``,
    or by nobody when k is None (such a span, like an env no span names, is not
    evaluated: its entries keep what they held).  0 <= lo <= hi <= n_env; the
    spans of one ship must not overlap.  ValueError otherwise.  ``covered``:
    every ship of every env has a network (``rollout_q`` and ``play_q`` need
    that).  The networks' weight buffers are referenced, not copied: training
    a network or ``copy_from`` changes what the pool plays."""

    __slots__ = ('nets', 'spans', 'n_env', 'S', 'nout', 'device', 'covered', '_nets', '_spans')

    def __init__(self, env, nets, spans):
        from .qnet import QNetwork
        nets, S, N = tuple(nets), env.S, env.n_env
        if not 1 <= len(nets) <= _lib.QPOOL_MAX_NETS:
            raise ValueError('a pool takes 1..%d networks, got %d' % (_lib.QPOOL_MAX_NETS, len(nets)))
        if any(not isinstance(n, QNetwork) for n in nets):
            raise ValueError('every network of a pool is a QNetwork')
        for n in nets:
            if n.weights.device != env.hdr.device:
                raise ValueError('the network is on %s, the env on %s' % (n.weights.device, env.hdr.device))
            if n.nships != S:
                raise ValueError('a network for %d ships in an env of %d' % (n.nships, S))
            if n.nout != nets[0].nout:
                raise ValueError('the networks differ in nout (%d and %d)' % (nets[0].nout, n.nout))
        rows = []
        for sp in spans:
            try:
                ship, lo, hi, k = sp
                bad = any(isinstance(v, bool) or v != int(v) for v in (ship, lo, hi) + (() if k is None else (k,)))
            except (TypeError, ValueError):
                bad = True
            if bad:
                raise ValueError('a span is (ship, lo, hi, k) of integers, k an index into nets or None: %r' % (sp,))
            rows.append((int(ship), int(lo), int(hi), None if k is None else int(k)))
        if not 1 <= len(rows) <= _lib.QPOOL_MAX_SPANS:
            raise ValueError('a pool takes 1..%d spans, got %d' % (_lib.QPOOL_MAX_SPANS, len(rows)))
        for ship, lo, hi, k in rows:
            if not 0 <= ship < S:
                raise ValueError('a span of ship %d in an env of %d ships' % (ship, S))
            if k is not None and not 0 <= k < len(nets):
                raise ValueError('a span of network %d in a pool of %d' % (k, len(nets)))
            if not 0 <= lo <= hi <= N:
                raise ValueError('a span needs 0 <= lo <= hi <= n_env (%d), got [%d, %d)' % (N, lo, hi))
        covered = True
        for s in range(S):
            mine = sorted((lo, hi, k) for ship, lo, hi, k in rows if ship == s and lo < hi)
            if any(a[1] > b[0] for a, b in zip(mine, mine[1:])):
                raise ValueError('the spans of ship %d overlap' % s)
            at = 0
            for lo, hi, k in mine:
                covered = covered and lo == at and k is not None
                at = hi
            covered = covered and at == N
        self.nets, self.spans = nets, tuple(rows)
        self.n_env, self.S, self.nout, self.device = N, S, nets[0].nout, env.hdr.device
        self.covered = covered
        # the C side's arrays, built once: AstroQNet is (pointer, nships, nout), and a QNetwork keeps its buffer
        self._nets = (_lib.AstroQNet * len(nets))(*[_lib.AstroQNet(weights=n.c.weights, nships=n.nships, nout=n.nout)
                                                    for n in nets])
        self._spans = (_lib.AstroQSpan * len(rows))(*[_lib.AstroQSpan(ship=ship, net=-1 if k is None else k,
                                                                      lo=lo, hi=hi) for ship, lo, hi, k in rows])

    def __setattr__(self, name, value):
        if hasattr(self, '_spans'):
            raise AttributeError('a Pool is immutable')
        object.__setattr__(self, name, value)

    @classmethod
    def versus(cls, env, net, rivals):
        """``net`` as ship 0 of every env; ship 1's envs in ``len(rivals)``
        blocks as equal as possible, block j = [j N // K, (j + 1) N // K)
        playing ``rivals[j]``."""
        rivals = tuple(rivals)
        K, N = len(rivals), env.n_env
        if env.S != 2:
            raise ValueError('Pool.versus needs a two-ship env')
        if not 1 <= K <= _lib.QPOOL_MAX_NETS - 1:
            raise ValueError('Pool.versus takes 1..%d rivals, got %d' % (_lib.QPOOL_MAX_NETS - 1, K))
        return cls(env, (net,) + rivals, [(0, 0, N, 0)] + [(1, j * N // K, (j + 1) * N // K, 1 + j) for j in range(K)])

    @staticmethod
    def pairs(m):
        """The ordered pairs (a, b), a != b, of range(m) in lexicographic order."""
        return [(a, b) for a in range(m) for b in range(m) if a != b]

    @classmethod
    def pairings(cls, env, nets):
        """One block of envs per ordered pair (a, b), a != b, of ``nets`` in
        lexicographic order: block j of P = M (M - 1) is [j N // P, (j + 1) N
        // P), ship 0 played by ``nets[a]`` and ship 1 by ``nets[b]``.  Needs a
        two-ship env, M >= 2, 2 P <= 64 spans (M <= 6) and N >= P."""
        nets = tuple(nets)
        pairs, N = cls.pairs(len(nets)), env.n_env
        P = len(pairs)
        if env.S != 2:
            raise ValueError('Pool.pairings needs a two-ship env')
        if P < 2 or 2 * P > _lib.QPOOL_MAX_SPANS:
            raise ValueError('Pool.pairings takes 2..6 networks (two spans per ordered pair, at most %d), got %d'
                             % (_lib.QPOOL_MAX_SPANS, len(nets)))
        if N < P:
            raise ValueError('Pool.pairings of %d networks needs at least %d envs, got %d' % (len(nets), P, N))
        spans = []
        for j, (a, b) in enumerate(pairs):
            lo, hi = j * N // P, (j + 1) * N // P
            spans += [(0, lo, hi, a), (1, lo, hi, b)]
        return cls(env, nets, spans)


def tournament(env, nets, games=1, seed=0):
    """Every network of ``nets`` against every other on ``env`` (two ships,
    auto-reset) in one ``play_q`` loop on ``Pool.pairings(env, nets)``: the envs
    of block (a, b) play their next ``games`` games with ``nets[a]`` as ship 0
    and ``nets[b]`` as ship 1, all greedy.  Returns ``dict(games=, wins=, none=,
    p_better=)`` of M x M nested lists: ``wins[a][b]`` a's wins over b over both
    seats, ``games[a][b]`` the games the two played (symmetric, as is
    ``none[a][b]``, those without a winner), ``p_better[a][b] =
    p_better(wins[a][b], wins[b][a])``; the diagonal is 0 / 0.5.  The counts
    are taken on the device and read once at the end.  A member may be a
    ``Script`` or a bot's name ('script', 'nothing', 'random'): the loop then
    runs on ``Seats.pairings``; a list of networks only takes ``Pool.pairings``
    as before."""
    import torch
    from .qnet import QNetwork
    nets = tuple(nets)
    scripted = any(not isinstance(n, QNetwork) for n in nets)
    pool = Seats.pairings(env, nets) if scripted else Pool.pairings(env, nets)
    winner = env._play_q(pool, None, games, None, None, seed).winner      # int8 [N, G]: -1 none, 0, 1
    M, N, pairs = len(nets), env.n_env, Pool.pairs(len(nets))
    P = len(pairs)
    block = torch.tensor([j for j in range(P) for _ in range((j + 1) * N // P - j * N // P)], dtype=torch.int64,
                         device=winner.device)
    slot = block[:, None] * 3 + (winner.to(torch.int64) + 1)            # per block: none, ship 0 won, ship 1 won
    counts = torch.zeros(3 * P, dtype=torch.int64, device=winner.device)
    counts.scatter_add_(0, slot.reshape(-1), torch.ones(slot.numel(), dtype=torch.int64, device=winner.device))
    counts = counts.cpu().view(P, 3).tolist()
    wins = [[0] * M for _ in range(M)]
    none = [[0] * M for _ in range(M)]
    played = [[0] * M for _ in range(M)]
    for (a, b), (n_none, n0, n1) in zip(pairs, counts):
        wins[a][b] += n0
        wins[b][a] += n1
        for x, y in ((a, b), (b, a)):
            none[x][y] += n_none
            played[x][y] += n_none + n0 + n1
    return dict(games=played, wins=wins, none=none,
                p_better=[[p_better(wins[a][b], wins[b][a]) for b in range(M)] for a in range(M)])


# ---------------------------------------------------------------------------
# scripted players

BOT_NAMES = ('script', 'nothing', 'random')


def _number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool) and v == v and abs(v) != float('inf')


class Script:
    """A ScriptBot's arguments (script.py:17-21) as an immutable value: a
    player of ``Seats``, an ``opponent`` of ``QTrainer``.  ``args`` is the
    reference's dict.  ValueError unless both are finite numbers."""

    __slots__ = ('avoid_distance', 'avoid_threshold')

    def __init__(self, avoid_distance=0.1, avoid_threshold=0.45):
        if not (_number(avoid_distance) and _number(avoid_threshold)):
            raise ValueError('avoid_distance and avoid_threshold are finite numbers, got %r and %r'
                             % (avoid_distance, avoid_threshold))
        object.__setattr__(self, 'avoid_distance', float(avoid_distance))
        object.__setattr__(self, 'avoid_threshold', float(avoid_threshold))

    def __setattr__(self, name, value):
        raise AttributeError('a Script is immutable')

    @property
    def args(self):
        return dict(avoid_distance=self.avoid_distance, avoid_threshold=self.avoid_threshold)

    def __eq__(self, other):
        return type(other) is Script and self.args == other.args

    def __hash__(self):
        return hash((self.avoid_distance, self.avoid_threshold))

    def __repr__(self):
        return 'Script(avoid_distance=%r, avoid_threshold=%r)' % (self.avoid_distance, self.avoid_threshold)


class Seats:
    """Who plays which ship of which envs, networks and scripted bots alike: a
    checked, immutable description that ``BatchedEnv.qvalues`` / ``qcontrols``
    / ``rollout_q`` / ``play_q`` take wherever they take a ``Pool``, and
    ``BatchedEnv.seat_controls`` for its scripted part alone.

    players: a sequence of ``QNetwork``s, ``Script``s and the names 'script'
    (a ``Script`` with the default arguments), 'nothing' and 'random'.  spans:
    ``(ship, lo, hi, k)`` as in ``Pool``, k an index into players or None, with
    ``Pool``'s rules and errors.  The network players' spans become ``pool`` (a
    ``Pool`` of those networks in their order of appearance, with ``Pool``'s
    limits; None without a network; the spans without a player go there too
    when there is one) and the scripted players' an AstroSeat array (at most
    64; one astro_controls_seats launch, include/astro_seats.h): every seat
    carries its own bot and its own ScriptBot arguments.  ``covered``: every
    ship of every env has a player.  ``nout``: the networks', or None."""

    __slots__ = ('players', 'spans', 'pool', 'covered', 'nout', 'n_env', 'S', 'device', '_seats')

    def __init__(self, env, players, spans):
        from .qnet import QNetwork
        players, S, N = tuple(players), env.S, env.n_env
        if not players:
            raise ValueError('Seats needs at least one player')
        norm = []
        for pl in players:
            if isinstance(pl, str) and pl in BOT_NAMES:
                pl = Script() if pl == 'script' else pl
            elif not isinstance(pl, (QNetwork, Script)):
                raise ValueError("a player is a QNetwork, a Script or one of 'script', 'nothing', 'random': %r" % (pl,))
            norm.append(pl)
        players = tuple(norm)
        rows = []
        for sp in spans:
            try:
                ship, lo, hi, k = sp
                bad = any(isinstance(v, bool) or v != int(v) for v in (ship, lo, hi) + (() if k is None else (k,)))
            except (TypeError, ValueError):
                bad = True
            if bad:
                raise ValueError('a span is (ship, lo, hi, k) of integers, k an index into players or None: %r' % (sp,))
            rows.append((int(ship), int(lo), int(hi), None if k is None else int(k)))
        if not rows:
            raise ValueError('Seats needs at least one span')
        for ship, lo, hi, k in rows:
            if not 0 <= ship < S:
                raise ValueError('a span of ship %d in an env of %d ships' % (ship, S))
            if k is not None and not 0 <= k < len(players):
                raise ValueError('a span of player %d among %d players' % (k, len(players)))
            if not 0 <= lo <= hi <= N:
                raise ValueError('a span needs 0 <= lo <= hi <= n_env (%d), got [%d, %d)' % (N, lo, hi))
        covered = True
        for s in range(S):
            mine = sorted((lo, hi, k is None) for ship, lo, hi, k in rows if ship == s and lo < hi)
            if any(a[1] > b[0] for a, b in zip(mine, mine[1:])):
                raise ValueError('the spans of ship %d overlap' % s)
            at = 0
            for lo, hi, empty in mine:
                covered = covered and lo == at and not empty
                at = hi
            covered = covered and at == N
        # the networks, in their order of appearance among the players, as a Pool of their spans
        nets, index = [], {}
        for pl in players:
            if isinstance(pl, QNetwork) and id(pl) not in index:
                index[id(pl)] = len(nets)
                nets.append(pl)
        net_rows, seat_rows = [], []
        for ship, lo, hi, k in rows:
            pl = None if k is None else players[k]
            if isinstance(pl, QNetwork):
                net_rows.append((ship, lo, hi, index[id(pl)]))
            elif pl is None and nets:
                net_rows.append((ship, lo, hi, None))
            else:
                seat_rows.append((ship, lo, hi, pl))
        if len(seat_rows) > _lib.SEATS_MAX:
            raise ValueError('Seats takes at most %d scripted seats, got %d' % (_lib.SEATS_MAX, len(seat_rows)))
        pool = Pool(env, nets, net_rows) if nets and net_rows else None
        c = env.config
        seats = []
        for ship, lo, hi, pl in seat_rows:
            a = pl if isinstance(pl, Script) else Script()
            seats.append(_lib.AstroSeat(
                ship=ship, bot=-1 if pl is None else _lib.BOTS['script' if isinstance(pl, Script) else pl], lo=lo, hi=hi,
                script_r2=(c.planet_radius + c.ship_radius + a.avoid_distance) ** 2,
                script_threshold=a.avoid_threshold))
        set_ = object.__setattr__
        set_(self, 'players', players)
        set_(self, 'spans', tuple(rows))
        set_(self, 'pool', pool)
        set_(self, 'covered', covered)
        set_(self, 'nout', None if pool is None else pool.nout)
        set_(self, 'n_env', N)
        set_(self, 'S', S)
        set_(self, 'device', env.hdr.device)
        set_(self, '_seats', (_lib.AstroSeat * len(seats))(*seats) if seats else None)

    def __setattr__(self, name, value):
        raise AttributeError('a Seats is immutable')

    @classmethod
    def versus(cls, env, player, rivals):
        """``player`` as ship 0 of every env; ship 1's envs in ``len(rivals)``
        blocks as equal as possible, block j = [j N // K, (j + 1) N // K)
        playing ``rivals[j]`` (``Pool.versus``' blocks)."""
        rivals = tuple(rivals)
        K, N = len(rivals), env.n_env
        if env.S != 2:
            raise ValueError('Seats.versus needs a two-ship env')
        if K < 1:
            raise ValueError('Seats.versus takes at least one rival')
        return cls(env, (player,) + rivals, [(0, 0, N, 0)] + [(1, j * N // K, (j + 1) * N // K, 1 + j) for j in range(K)])

    @classmethod
    def pairings(cls, env, players):
        """``Pool.pairings`` for players of any kind: one block of envs per
        ordered pair (a, b), a != b, in lexicographic order, block j of P = M
        (M - 1) being [j N // P, (j + 1) N // P), ship 0 played by
        ``players[a]`` and ship 1 by ``players[b]``.  Needs a two-ship env, M
        >= 2 and N >= P; the networks' spans and the scripted seats have their
        own limits (``Pool``'s, 64)."""
        players = tuple(players)
        pairs, N = Pool.pairs(len(players)), env.n_env
        P = len(pairs)
        if env.S != 2:
            raise ValueError('Seats.pairings needs a two-ship env')
        if P < 2:
            raise ValueError('Seats.pairings takes at least 2 players, got %d' % len(players))
        if N < P:
            raise ValueError('Seats.pairings of %d players needs at least %d envs, got %d' % (len(players), P, N))
        spans = []
        for j, (a, b) in enumerate(pairs):
            lo, hi = j * N // P, (j + 1) * N // P
            spans += [(0, lo, hi, a), (1, lo, hi, b)]
        return cls(env, players, spans)


def mutate(args, scale, random):
    """ScriptBot.mutate (script.py:93-108): a copy of ``args`` with ``scale *
    random.normal()`` added to 'avoid_distance', then to 'avoid_threshold'
    (``random``: a numpy RandomState)."""
    args = dict(args)
    args['avoid_distance'] += scale * random.normal()
    args['avoid_threshold'] += scale * random.normal()
    return args


class _More(Exception):
    """find_better asked for a game that has not been played yet."""


def _so_far(winners, count):
    """``winners``, counting in count[0] the games taken; then _More."""
    for w in winners:
        count[0] += 1
        yield w
    raise _More()


def tune_script(env, max_trials, threshold, max_mutations, scale, args=None, seed=None, candidates=1):
    """ScriptBot.optimize (script.py:110-127), the random-walk 1-vs-1
    tournament behind ScriptBot.DEFAULT_ARGS, on a two-ship ``env``.

    ``random = RandomState(env.config.seed if seed is None else seed)``; ``best``
    starts at ``args`` (default ScriptBot.DEFAULT_ARGS).  Each of
    ``max_mutations`` rounds draws ``candidates`` mutations ``mutate(best, scale,
    random)`` in order, one per block of envs (block j = [j N // K, (j + 1) N //
    K)): ``best`` plays ship 0 of every env and candidate j ship 1 of block j
    (a ``Seats``), as in the reference.  A pass re-creates every env
    (``env.reset()``: the next game of its stream) and plays one game per env
    (``play_q``); block j's winners, ordered by (pass, env), are what
    ``find_better(..., max_trials, threshold)`` is given, and passes stop once it
    has an answer for every block (at the latest after ``max_trials`` games of
    a block).  ``best`` becomes the lowest-numbered candidate judged better
    (verdict 1).  ``candidates=1`` is the reference's sequential walk.

    Returns ``(best_args, history)``: per round ``dict(candidates=[args, ...],
    wins=[[best's, candidate's, none], ...], games=[...], verdicts=[0 | 1 |
    None, ...], passes=, best=args after the round)`` with the counts over the
    games ``find_better`` was given.  Deterministic: the env's streams and
    ``random`` decide everything.  Synchronises."""
    import numpy as np
    for name, v in (('max_trials', max_trials), ('max_mutations', max_mutations), ('candidates', candidates)):
        if isinstance(v, bool) or not isinstance(v, int) or v < (0 if name == 'max_mutations' else 1):
            raise ValueError('%s must be an int >= %d, got %r' % (name, 0 if name == 'max_mutations' else 1, v))
    if not (_number(threshold) and 0.5 <= threshold < 1.0):
        raise ValueError('threshold must be in [0.5, 1), got %r' % (threshold,))
    if not _number(scale):
        raise ValueError('scale must be a finite number, got %r' % (scale,))
    if env.S != 2:
        raise ValueError('tune_script needs a two-ship env')
    K, N = candidates, env.n_env
    if N < K:
        raise ValueError('tune_script with %d candidates needs at least %d envs, got %d' % (K, K, N))
    if K > _lib.SEATS_MAX - 1:
        raise ValueError('tune_script takes at most %d candidates, got %d' % (_lib.SEATS_MAX - 1, K))
    best = Script(**(args or {})).args
    random = np.random.RandomState(env.config.seed if seed is None else seed)
    bounds = [(j * N // K, (j + 1) * N // K) for j in range(K)]
    history = []
    for _ in range(max_mutations):
        cands = [mutate(best, scale, random) for _ in range(K)]
        seats = Seats.versus(env, Script(**best), [Script(**c) for c in cands])
        played = [[] for _ in range(K)]
        verdicts, final, games, passes = [None] * K, [False] * K, [0] * K, 0
        while not all(final):
            env.reset()
            winner = env._play_q(seats, None, 1, None, None, 0).winner[:, 0].cpu().tolist()
            passes += 1
            for j, (lo, hi) in enumerate(bounds):
                if final[j]:
                    continue
                played[j] = (played[j] + [None if w < 0 else w for w in winner[lo:hi]])[:max_trials]
                count = [0]
                try:
                    verdicts[j] = find_better(_so_far(played[j], count), max_trials, threshold)
                    final[j] = True
                except _More:   # (undecided after max_trials games: p_better exactly at the threshold)
                    final[j] = len(played[j]) >= max_trials
                games[j] = count[0]   # the games find_better took: up to the one that decided
        wins = []
        for j in range(K):
            used = played[j][:games[j]]
            wins.append([used.count(0), used.count(1), used.count(None)])
        better = [j for j in range(K) if verdicts[j] == 1]
        if better:
            best = cands[better[0]]
        history.append(dict(candidates=cands, wins=wins, games=games, verdicts=verdicts, passes=passes, best=dict(best)))
    return best, history
