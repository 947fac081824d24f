"""The evolution strategy on the device (libastro_es.so, include/astro_es.h):
``es.perturb``, ``es.score`` and ``es.gradient`` against their numpy mirrors,
bit for bit, on synthetic arrays -- every output inside a guard band that must
keep its bytes, every input unchanged -- and then ``Population`` and
``ESTrainer`` on real envs: the members are what ``perturb_host`` says, every
block is played by its member, the fork gives every block the same games, the
fitness is ``score_host`` of the episodes, and a generation is
``gradient_host`` plus ``optim.step_host``.  Nothing here claims that anything
learns."""
import numpy as np
import pytest
import torch

from astro_amd import BatchedEnv, DEFAULT_CONFIG, es, league, optim, qnet
from tests import qtrain_util as qt

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARD = 64
SHORT = DEFAULT_CONFIG._replace(max_time=3.0)            # 150 ticks at most
SIGMA = 0.1                                              # inexact in float32
ARRAYS = ('ships', 'ships_b', 'planets', 'bullets', 'hdr', 'stream', 'stream_ring')


def bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def guarded(shape, dtype, fill):
    """(the whole buffer, the view of `shape` in its middle): GUARD elements on either side."""
    n = int(np.prod(shape))
    big = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return big, big[GUARD:GUARD + n].view(shape)


def band_kept(big, fill):
    b = big.cpu()
    return bool((b[:GUARD] == fill).all() and (b[-GUARD:] == fill).all())


# ---------------------------------------------------------------------------
# perturb

@pytest.mark.parametrize('nparams', [1, 63, 64, 65, 257, 4934])
def test_perturb_equals_the_mirror(nparams):
    rng = np.random.RandomState(nparams)
    theta_h = rng.normal(size=nparams).astype(np.float32)
    theta = torch.from_numpy(theta_h).to(DEV)
    pairs = 21
    checked = 0
    for npairs in (0, 1, 3, 16):
        for first in sorted({0, 5, pairs - npairs}):
            for gen, seed in ((0, 11), (1, 11), (2 ** 40, 11), (1, 2 ** 63 + 5)):
                big, members = guarded((2 * npairs, nparams), torch.float32, 7.5)
                assert es.perturb(theta, members, pairs, SIGMA, seed, gen, first) is members
                want = es.perturb_host(theta_h, SIGMA, seed, gen, first, npairs)
                assert same(members, want), (npairs, first, gen, seed)
                assert band_kept(big, 7.5), (npairs, first, gen, seed)
                checked += want.size
    assert same(theta, theta_h) and checked > 0
    # the rows are antithetic around theta and differ from it
    m = es.perturb(theta, torch.empty((2, nparams), dtype=torch.float32, device=DEV), pairs, SIGMA, 11, 0, 20).cpu().numpy()
    d = np.float32(SIGMA) * es.noise_host(11, 0, 20, 1, nparams)[0]
    assert np.array_equal(m[0], theta_h + d) and np.array_equal(m[1], theta_h - d)


def test_perturb_errors():
    theta = torch.zeros(10, dtype=torch.float32, device=DEV)
    ok = torch.zeros((4, 10), dtype=torch.float32, device=DEV)
    for args, word in (((theta, ok[:3], 4, SIGMA), 'members'), ((theta, ok[:, :9], 4, SIGMA), 'members'),
                       ((theta, ok.double(), 4, SIGMA), 'members'), ((theta, ok.cpu(), 4, SIGMA), 'members'),
                       ((theta.double(), ok, 4, SIGMA), 'theta'), ((theta, ok.t().contiguous().t(), 4, SIGMA), 'members'),
                       ((theta, ok, 0, SIGMA), 'pairs'), ((theta, ok, 513, SIGMA), 'pairs'), ((theta, ok, 4, 0.0), 'sigma'),
                       ((theta, ok, 1, SIGMA), 'inside'), ((theta, ok, 4, SIGMA, 0, 0, 3), 'inside'),
                       ((theta, ok, 4, SIGMA, 0, 0, -1), 'inside')):
        with pytest.raises(ValueError, match=word):
            es.perturb(*args)
    both = torch.zeros(50, dtype=torch.float32, device=DEV)
    with pytest.raises(Exception, match='overlaps'):          # the library's own check
        es.perturb(both[5:15], both[10:50].view(4, 10), 4, SIGMA)
    assert float(both.abs().sum()) == 0.0


# ---------------------------------------------------------------------------
# score

def episodes(N, G, seed, timeout):
    """winner with all four codes (and a foreign one), ticks on both sides of the timeout."""
    rng = np.random.RandomState(seed)
    winner = rng.choice(np.array([0, 1, -1, -2, 0, 1], np.int8), size=(N, G))
    ticks = rng.randint(1, 2 * timeout, size=(N, G)).astype(np.int32)
    ticks[rng.rand(N, G) < 0.2] = timeout
    return winner, ticks


@pytest.mark.parametrize('N,K,G', [(1, 1, 1), (7, 2, 3), (77, 6, 1), (64, 32, 2), (5, 8, 1), (3000, 3, 2)])
def test_score_equals_the_mirror(N, K, G):
    timeout = 150
    seen = set()
    for ship in (0, 1):
        for draw, survive in ((0.0, 0.0), (0.3, 0.7)):
            wh, th = episodes(N, G, 100 * N + K + ship, timeout)
            seen |= set(wh.ravel().tolist())
            w, t = torch.from_numpy(wh).to(DEV), torch.from_numpy(th).to(DEV)
            bf, fit = guarded((K,), torch.float32, -9.0)
            bc, cnt = guarded((K, 3), torch.int32, -77)
            bl, lost = guarded((K,), torch.int64, -55)
            got = es.score(w, t, K, ship, draw, survive, timeout, fitness=fit, counts=cnt, lost_ticks=lost)
            assert got[0] is fit and got[1] is cnt and got[2] is lost
            c_h, l_h, f_h = es.score_host(wh, th, K, ship, draw, survive, timeout)
            assert np.array_equal(cnt.cpu().numpy(), c_h) and np.array_equal(lost.cpu().numpy(), l_h)
            assert same(fit, f_h), (ship, draw, fit.cpu(), f_h)
            assert band_kept(bf, -9.0) and band_kept(bc, -77) and band_kept(bl, -55)
            assert same(w, wh) and same(t, th)
            assert int(c_h.sum()) == int((wh != -2).sum())
            if N < K:
                assert np.isnan(f_h).any()                  # empty blocks occur
            # the optional outputs left out: the same fitness
            f2, c2, l2 = es.score(w, t, K, ship, draw, survive, timeout)
            assert c2 is None and l2 is None and same(f2, f_h)
            f3, c3, l3 = es.score(w, t, K, ship, draw, survive, timeout, counts=True)
            assert l3 is None and np.array_equal(c3.cpu().numpy(), c_h) and same(f3, f_h)
    if N * G >= 20:
        assert seen == {0, 1, -1, -2}


def test_score_foreign_codes_and_long_games():
    """Any winner code but ship, -1 and -2 is a loss; ticks far above the timeout count as the timeout."""
    wh = np.array([[5, -3, 0, -2, -1, 1, 127, -128]], np.int8).T.copy()
    th = np.array([[2 ** 31 - 1, 3, 9, 9, 9, 2 ** 30, 1, 149]], np.int32).T.copy()
    f, c, l = es.score(torch.from_numpy(wh).to(DEV), torch.from_numpy(th).to(DEV), 1, 0, 0.0, 1.0, 150, counts=True,
                       lost_ticks=True)
    c_h, l_h, f_h = es.score_host(wh, th, 1, 0, 0.0, 1.0, 150)
    assert c_h.tolist() == [[1, 5, 1]] and l_h.tolist() == [150 + 3 + 150 + 1 + 149]
    assert np.array_equal(c.cpu().numpy(), c_h) and np.array_equal(l.cpu().numpy(), l_h) and same(f, f_h)


# ---------------------------------------------------------------------------
# gradient

def fitness_cases(K, seed):
    rng = np.random.RandomState(seed)
    plain = rng.normal(size=K).astype(np.float32)
    ties = rng.randint(-2, 3, size=K).astype(np.float32) / np.float32(4)
    equal = np.full(K, 0.375, np.float32)
    nan, inf = plain.copy(), plain.copy()
    nan[K // 3] = np.nan
    inf[K - 1] = -np.inf
    return dict(plain=plain, ties=ties, equal=equal, nan=nan, inf=inf)


@pytest.mark.parametrize('shaping', ['ranks', 'raw'])
@pytest.mark.parametrize('pairs', [1, 3, 16, 512])
def test_gradient_equals_the_mirror(pairs, shaping):
    K = 2 * pairs
    nparams = 257 if pairs == 512 else 4934
    for name, f_h in fitness_cases(K, pairs).items():
        gen, seed = (2 ** 40 + 3, 5) if name == 'ties' else (pairs, 2 ** 64 - 3)
        f = torch.from_numpy(f_h).to(DEV)
        bg, grad = guarded((nparams,), torch.float32, 3.25)
        bu, util = guarded((K,), torch.float32, -3.25)
        got = es.gradient(f, nparams, SIGMA, seed, gen, shaping, utilities=util, out=grad)
        assert got[0] is grad and got[1] is util
        u_h = es.utilities_host(f_h, shaping)
        g_h = es.gradient_host(f_h, nparams, SIGMA, seed, gen, shaping)
        assert same(util, u_h), (name, 'utilities')
        assert same(grad, g_h), (name, 'gradient')
        assert band_kept(bg, 3.25) and band_kept(bu, -3.25) and same(f, f_h)
        if name in ('nan', 'inf') or (name == 'equal' and shaping == 'ranks'):
            assert not g_h.any() and not u_h.any()
        elif name == 'plain':
            assert np.count_nonzero(g_h) > 0.99 * nparams
        # without the utilities: the same gradient
        assert same(es.gradient(f, nparams, SIGMA, seed, gen, shaping), g_h), name
    if shaping == 'ranks':
        assert len(set(es.utilities_host(fitness_cases(K, pairs)['ties']).tolist())) <= 5


def test_gradient_odd_sizes_and_errors():
    f_h = np.array([0.5, -1.0, 2.0, 2.0, -3.0, 0.0], np.float32)
    f = torch.from_numpy(f_h).to(DEV)
    for n in (1, 63, 64, 65, 256, 257):
        assert same(es.gradient(f, n, SIGMA, 1, 2), es.gradient_host(f_h, n, SIGMA, 1, 2)), n
    for args, kw, word in (((f[:5], 10, SIGMA), {}, 'pairs'), ((f.double(), 10, SIGMA), {}, 'fitness'),
                           ((f, 0, SIGMA), {}, 'nparams'), ((f, 10, -1.0), {}, 'sigma'),
                           ((f, 10, SIGMA), dict(out=torch.zeros(9, device=DEV)), 'out'),
                           ((f, 10, SIGMA), dict(utilities=torch.zeros(5, device=DEV)), 'utilities'),
                           ((f, 10, SIGMA), dict(shaping='best'), 'shaping')):
        with pytest.raises(ValueError, match=word):
            es.gradient(*args, **kw)


# ---------------------------------------------------------------------------
# on real envs

N_ENV, PAIRS = 64, 2
K = 2 * PAIRS
B = N_ENV // K


def make(n=N_ENV, age=40):
    env = BatchedEnv(SHORT, n, device=DEV, auto_reset=True, b_cap=32)
    env.reset()
    if age:
        env.rollout(age, 'random', tick0=1 << 20)
    return env


def net_of(factor=1.0):
    return qnet.QNetwork.from_module(qt.weights_of('duo', factor=factor), DEV)


def raw(env):
    torch.cuda.synchronize()
    out = {k: bits(getattr(env, k)) for k in ARRAYS}
    for k in ('ships', 'planets'):
        out[k] = out[k].transpose(1, 0, 2)
    out['ships_b'] = out['ships_b'].transpose(1, 0)
    return out


def trainer(env, net, **kw):
    a = dict(opponent='script', pairs=PAIRS, sigma=SIGMA, games=1, seed=3)
    a.update(kw)
    return es.ESTrainer(env, net, **a)


def test_members_are_the_mirrors_and_each_block_plays_its_member():
    env, net = make(), net_of()
    theta_h = net.weights.cpu().numpy().copy()
    tr = trainer(env, net)
    pop = tr.pop
    assert pop.K == K and pop.members.shape == (K, theta_h.size) and pop.theta is net.weights
    assert same(pop.members, np.tile(theta_h, (K, 1)))         # before the first perturb: the centre
    assert tr.perturb(0) is pop.members
    assert same(pop.members, es.perturb_host(theta_h, SIGMA, 3, 0, 0, PAIRS)) and same(net.weights, theta_h)
    for k, member in enumerate(pop.nets):
        assert member.weights.data_ptr() == pop.members[k].data_ptr() and (member.nships, member.nout) == (2, 6)
    c = env.qcontrols(tr.seats).cpu().numpy()
    differ = 0
    for k, (lo, hi) in enumerate(es.blocks(N_ENV, K)):
        alone = env.qcontrols((pop.nets[k], None)).cpu().numpy()
        assert np.array_equal(c[lo:hi, 0], alone[lo:hi, 0]), k
        differ += int((alone[:, 0] != env.qcontrols((net, None)).cpu().numpy()[:, 0]).sum())
    assert np.array_equal(c[:, 1], env.controls('script').cpu().numpy()[:, 1])
    assert differ > 0                                          # the members do not all play the centre's game
    # a later generation is other noise
    pop.generation = 1
    tr.perturb(0)
    assert same(pop.members, es.perturb_host(theta_h, SIGMA, 3, 1, 0, PAIRS))
    with pytest.raises(ValueError, match='row'):
        qnet.QNetwork.view(pop.members[0][:10], 2, 6)


def test_common_games_equal_blocks_and_the_fitness_is_the_mirror():
    env, net = make(), net_of()
    tr = trainer(env, net, draw=0.25, survive=0.5)
    # right after the fork: every state array of block j is block 0's
    tr.plan.apply()
    r = raw(env)
    nb = (r['hdr'][:, 1] >> 16) & 0xffff
    for j in range(1, K):
        for name in ARRAYS:
            if name != 'bullets':
                assert np.array_equal(r[name][j * B:(j + 1) * B], r[name][:B]), (j, name)
        for i in range(B):
            assert np.array_equal(r['bullets'][j * B + i, :nb[i]], r['bullets'][i, :nb[i]]), (j, i)
    assert len({r['stream'][i, 3] for i in range(B)}) > 1       # ... and block 0's envs are not one game
    # four copies of theta: every block plays the same games to the same ends
    assert same(tr.pop.members, np.tile(net.weights.cpu().numpy(), (K, 1)))
    ep = tr.evaluate(0)
    w, t = ep.winner.cpu().numpy(), ep.ticks.cpu().numpy()
    assert (w > -2).all() and w.shape == (N_ENV, 1)
    for j in range(1, K):
        assert np.array_equal(w[j * B:(j + 1) * B], w[:B]) and np.array_equal(t[j * B:(j + 1) * B], t[:B]), j
    T = env.schedule.timeout_tick
    _, _, f_h = es.score_host(w, t, K, 0, 0.25, 0.5, T)
    assert same(tr.fitness, f_h) and len(set(bits(f_h).tolist())) == 1
    # perturbed members: the blocks part ways, and the fitness is still the mirror of the episodes
    tr.perturb(0)
    ep = tr.evaluate(0)
    w, t = ep.winner.cpu().numpy(), ep.ticks.cpu().numpy()
    _, _, f_h = es.score_host(w, t, K, 0, 0.25, 0.5, T)
    assert same(tr.fitness, f_h) and np.isfinite(f_h).all()
    assert any(not np.array_equal(t[j * B:(j + 1) * B], t[:B]) for j in range(1, K))


def test_one_generation_is_the_mirrors():
    env, net = make(), net_of()
    theta_h = net.weights.cpu().numpy().copy()
    tr = trainer(env, net, lr=0.5, shaping='ranks')
    mean = tr.generation()
    f_h = tr.fitness.cpu().numpy()
    assert np.isfinite(f_h).all() and same(mean, np.float32(tr.fitness.mean().cpu().numpy()))
    assert same(tr.pop.members, es.perturb_host(theta_h, SIGMA, 3, 0, 0, PAIRS))
    g_h = es.gradient_host(f_h, theta_h.size, SIGMA, 3, 0, 'ranks')
    assert same(tr.grad, g_h)
    w_h, _, _, _, skipped = optim.step_host('sgd', tr.optimizer.hyper(1), theta_h, g_h, ())
    assert not skipped and same(net.weights, w_h)
    assert tr.pop.generation == 1 and tr.ngen == 1 and tr.optimizer.t == 1
    if len(set(f_h.tolist())) > 1:
        assert not same(net.weights, theta_h)
    s = tr.validate(env, 1, 'script')
    assert s['games'] == N_ENV


def test_three_generations_with_adam_repeat_bit_for_bit():
    runs = []
    for _ in range(2):
        env, net = make(), net_of()
        tr = trainer(env, net, optimizer=optim.Adam(lr=1e-2), shaping='raw', opponent=['script', 'nothing'])
        means = [tr.generation() for _ in range(3)]
        runs.append((bits(net.weights), bits(torch.stack(means)), bits(tr.fitness), bits(tr.optimizer.state)))
        assert tr.pop.generation == 3
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def test_two_rounds_fill_both_halves():
    env, net = make(), net_of()
    theta_h = net.weights.cpu().numpy().copy()
    tr = trainer(env, net, rounds=2, common_games=False, opponent=league.Script(0.2, 0.4))
    assert tr.fitness.shape == (2 * K,) and bool(tr.fitness.isnan().all()) and tr.plan is None
    seen = []
    for r in range(2):
        tr.perturb(r)
        assert same(tr.pop.members, es.perturb_host(theta_h, SIGMA, 3, 0, r * PAIRS, PAIRS))      # pairs 0-1, then 2-3
        ep = tr.evaluate(r)
        _, _, f_h = es.score_host(ep.winner.cpu().numpy(), ep.ticks.cpu().numpy(), K, 0, 0.0, 0.0,
                                  env.schedule.timeout_tick)
        seen.append(f_h)
        assert same(tr.fitness[r * K:(r + 1) * K], f_h)
        if r == 0:
            assert bool(tr.fitness[K:].isnan().all())
    assert same(tr.fitness, np.concatenate(seen))
    tr.update()
    g_h = es.gradient_host(np.concatenate(seen), theta_h.size, SIGMA, 3, 0, 'ranks')
    assert same(tr.grad, g_h)
    with pytest.raises(ValueError, match='round'):
        tr.evaluate(2)
