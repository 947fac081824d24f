"""Which of two bots is better: the reference's util.p_better / find_better
(util.py:169-214) without scipy, and ``compare``, which plays two Q-networks
against each other on a ``BatchedEnv`` (``play_q`` with a network opponent:
one astro_qvalues_ships launch per tick, include/astro_qduel.h).
"""


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
    wins_b)``.  Synchronises."""
    first = env._play_q(net_a, net_b, games, None, None, seed).winner
    second = env._play_q(net_b, net_a, games, None, None, seed).winner
    wins_a = int((first == 0).sum()) + int((second == 1).sum())
    wins_b = int((first == 1).sum()) + int((second == 0).sum())
    total = int(first.numel() + second.numel())
    return dict(games=total, wins_a=wins_a, wins_b=wins_b, none=total - wins_a - wins_b,
                p_better=p_better(wins_a, wins_b))
