"""The optimiser library on the device (include/astro_qopt.h, astro_amd/optim.py)
against its numpy mirror bit for bit, and what is built on it: QNetwork.step /
clone / td_targets(online=) and QTrainer's options against the loop written out."""
import types

import numpy as np
import pytest
import torch

from astro_amd import BatchedEnv, _lib, actor, optim, qnet, replay, train
from tests import golden_io as gio
from tests import qopt_util as qo
from tests import qtrain_util as qt

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SIZES = (1, 63, 1024, 1025, 4609, 4934)   # one element, a partial wave, one pass, one into the second, both networks


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _flat(w):
    """What ``apply`` needs of a network: its weight tensor."""
    return types.SimpleNamespace(weights=_dev(w))


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def _same(t, a):
    return _bits(t) == np.ascontiguousarray(a).tobytes()


@pytest.mark.parametrize('name,kind,kw', qo.CONFIGS, ids=[c[0] for c in qo.CONFIGS])
def test_step_equals_the_host_bit_for_bit(name, kind, kw):
    rng = np.random.default_rng(sum(map(ord, name)))
    for n in SIZES:
        grads = qo.normal_grads(rng, 25, n)
        w = qo.start_weights(rng, n)
        state = tuple(np.zeros(n, np.float32) for _ in range(qo.nstate(kind, kw)))
        net, opt = _flat(w), qo.make(kind, kw)
        for t in range(1, 26):
            g = _dev(grads[t - 1])
            opt.apply(net, g)
            w, state, _, norm, skipped = optim.step_host(kind, opt.hyper(t), w, grads[t - 1], state)
            assert not skipped and opt.t == t
            assert _same(net.weights, w), (n, t)
            assert opt.state.shape == (len(state), n) and all(_same(opt.state[i], s) for i, s in enumerate(state)), (n, t)
            assert _same(opt.norm, np.float32([norm])), (n, t)
            assert _same(g, grads[t - 1])
        assert int(opt.skipped) == 0 and np.isfinite(w).all()


def test_clip_and_guard():
    rng = np.random.default_rng(5)
    n = 1025
    for name, kind, kw in qo.CONFIGS:
        g = qo.normal_grads(rng, 1, n)[0]
        w0 = qo.start_weights(rng, n)
        norm = float(optim.norm_host(g))

        def run(max_norm, grad=g):
            net, opt = _flat(w0), qo.make(kind, kw, max_norm=max_norm)
            opt.apply(net, _dev(grad))
            return net, opt

        plain, popt = run(None)
        loose, lopt = run(norm * 1.01)
        assert _bits(loose.weights) == _bits(plain.weights) and _bits(lopt.state) == _bits(popt.state)
        tight, topt = run(norm / 3)
        hw, hs, _, hn, _ = optim.step_host(kind, topt.hyper(1), w0, g, [np.zeros(n, np.float32)] * topt.nstate)
        assert _same(tight.weights, hw) and all(_same(topt.state[i], s) for i, s in enumerate(hs))
        assert _same(topt.norm, np.float32([hn])) and _bits(tight.weights) != _bits(plain.weights)
        # a zero gradient: norm 0, coef 1, only what the rule says moves
        zero, zopt = run(1.0, np.zeros(n, np.float32))
        hw, hs, _, hn, _ = optim.step_host(kind, zopt.hyper(1), w0, np.zeros(n, np.float32),
                                           [np.zeros(n, np.float32)] * zopt.nstate)
        assert _same(zero.weights, hw) and all(_same(zopt.state[i], s) for i, s in enumerate(hs)) and float(zopt.norm) == 0
        if not kw.get('weight_decay'):
            assert _same(zero.weights, w0)
        # one NaN, one inf at the last index: nothing moves but skipped, and the next finite step proceeds
        net, opt, target = _flat(w0), qo.make(kind, kw, max_norm=1.0), _flat(w0 + np.float32(1))
        opt.apply(net, _dev(g), target=target, tau=0.5)
        w1, s1, t1 = _bits(net.weights), _bits(opt.state), _bits(target.weights)
        for k, (poison, at) in enumerate(((np.nan, 7), (np.inf, n - 1))):
            gp = g.copy()
            gp[at] = poison
            opt.apply(net, _dev(gp), target=target, tau=0.5)
            assert (_bits(net.weights), _bits(opt.state), _bits(target.weights)) == (w1, s1, t1), (name, poison)
            assert int(opt.skipped) == k + 1 and not np.isfinite(float(opt.norm))
        opt.apply(net, _dev(g), target=target, tau=0.5)
        assert _bits(net.weights) != w1 and _bits(target.weights) != t1 and int(opt.skipped) == 2
        assert np.isfinite(net.weights.cpu().numpy()).all() and float(opt.norm) == np.float32(norm)


def test_target_network():
    rng = np.random.default_rng(6)
    n = 4934
    grads = qo.normal_grads(rng, 12, n)
    for name, kind, kw in (qo.CONFIGS[4], qo.CONFIGS[1], qo.CONFIGS[6]):
        w = qo.start_weights(rng, n)
        tw = qo.start_weights(rng, n)
        state = tuple(np.zeros(n, np.float32) for _ in range(qo.nstate(kind, kw)))
        net, target, opt = _flat(w), _flat(tw), qo.make(kind, kw)
        for t in range(1, 11):       # tau = 0.01 over 10 steps
            opt.apply(net, _dev(grads[t - 1]), target=target, tau=0.01)
            w, state, tw, _, _ = optim.step_host(kind, opt.hyper(t), w, grads[t - 1], state, target=tw, tau=0.01)
            assert _same(net.weights, w) and _same(target.weights, tw), (name, t)
        assert _bits(target.weights) != _bits(net.weights)
        before = _bits(target.weights)
        opt.apply(net, _dev(grads[10]))                       # without target nothing else moves
        w, state, _, _, _ = optim.step_host(kind, opt.hyper(11), w, grads[10], state)
        assert _bits(target.weights) == before and _same(net.weights, w)
        opt.apply(net, _dev(grads[11]), target=target)        # tau = 1: an exact copy of the new weights
        w, state, tw, _, _ = optim.step_host(kind, opt.hyper(12), w, grads[11], state, target=tw, tau=1.0)
        assert _bits(target.weights) == _bits(net.weights) and _same(net.weights, w) and _same(target.weights, tw)
        with pytest.raises(_lib.AstroError, match='target is weights'):
            opt.apply(net, _dev(grads[0]), target=net)
        with pytest.raises(_lib.AstroError, match='tau'):
            opt.apply(net, _dev(grads[0]), target=target, tau=0.0)
        assert opt.t == 12 and _same(net.weights, w)          # a rejected call changed nothing


def test_step_is_reproducible_and_ignores_nothing_it_should_read():
    rng = np.random.default_rng(7)
    n = 4934
    g, g2 = qo.normal_grads(rng, 2, n)
    w0 = qo.start_weights(rng, n)
    for name, kind, kw in qo.SIX:
        def two_steps(prefill=None):
            net, opt = _flat(w0), qo.make(kind, kw)
            opt._bind(net)
            if prefill is not None:
                opt.state.fill_(prefill)
            opt.apply(net, _dev(g))
            opt.apply(net, _dev(g2))
            return net, opt
        a, aopt = two_steps()
        b, bopt = two_steps()
        assert _bits(a.weights) == _bits(b.weights) and _bits(aopt.state) == _bits(bopt.state)
        c, _ = two_steps(prefill=0.5)
        assert _bits(c.weights) != _bits(a.weights), name      # the state is read
        # reset(): the zero-state result again, from the same weights
        sd = aopt.state_dict()
        aopt.reset()
        assert aopt.t == 0 and not aopt.state.any()
        a.weights.copy_(_dev(w0))
        aopt.apply(a, _dev(g))
        aopt.apply(a, _dev(g2))
        assert _bits(a.weights) == _bits(b.weights) and _bits(aopt.state) == _bits(bopt.state)
        # state_dict / load_state_dict: a third step from the restored state equals b's third step
        aopt.reset()
        aopt.load_state_dict(sd)
        assert aopt.t == 2 and _bits(aopt.state) == _bits(bopt.state)
        aopt.apply(a, _dev(g))
        bopt.apply(b, _dev(g))
        assert _bits(a.weights) == _bits(b.weights)
        with pytest.raises(ValueError, match='another QNetwork'):
            aopt.apply(b, _dev(g))


def _env(N, ticks=30):
    env = BatchedEnv(gio.configs()['short'], N, device=DEV, b_cap=32)
    env.reset()
    env.rollout(ticks, 'random', seed=4)
    return env


def _duo():
    return qnet.QNetwork.from_module(qt.weights_of('duo'), DEV)


def test_qnetwork_step_is_grad_then_apply():
    env = _env(64)
    f = env.features()
    rng = np.random.default_rng(8)
    a, y = _dev(rng.integers(0, 6, 64).astype(np.int8)), _dev(rng.uniform(-1, 1, 64).astype(np.float32))
    net, twin, old = _duo(), _duo(), _duo()
    clone = net.clone()
    assert clone.weights.data_ptr() != net.weights.data_ptr() and _bits(clone.weights) == _bits(net.weights)
    assert (clone.nships, clone.nout, clone.c.weights) == (2, 6, clone.weights.data_ptr())
    opt, topt = optim.Adam(max_norm=10.0), optim.Adam(max_norm=10.0)
    for _ in range(3):
        loss = net.step(f, a, y, opt, target_net=clone, tau=0.5)
        tloss, grad = twin.grad(f, a, y)
        topt.apply(twin, grad)
        assert _bits(loss) == _bits(tloss) and _bits(net.weights) == _bits(twin.weights)
    start = _bits(old.weights)
    assert _bits(net.weights) != start and _bits(clone.weights) not in (start, _bits(net.weights))
    assert opt.t == 3 and int(opt.skipped) == 0 and float(opt.norm) > 0
    # the acting kernel reads the stepped buffer: a fresh network of the new weights gives the same values
    fresh = qnet.QNetwork(net.weights.cpu().numpy(), 2, 6, DEV)
    assert _bits(env.qvalues(net)) == _bits(env.qvalues(fresh)) != _bits(env.qvalues(old))
    # copy_from, on the device
    assert clone.copy_from(net) is clone and _bits(clone.weights) == _bits(net.weights)
    assert clone.weights.data_ptr() != net.weights.data_ptr()
    # sgd_step is what it was: grad, then torch's add_
    _, g0 = old.grad(f, a, y)
    want = old.weights.clone().add_(g0, alpha=-1e-2)
    old.sgd_step(f, a, y, lr=1e-2)
    assert _bits(old.weights) == _bits(want) != start


def test_double_targets():
    N = 70
    env = _env(N)
    nf = env.features()
    rng = np.random.default_rng(9)
    reward = _dev(rng.uniform(-1, 1, N).astype(np.float32))
    discount = _dev(rng.uniform(0.5, 1, N).astype(np.float32))
    terminal = _dev((rng.random(N) < 0.3).astype(np.uint8))
    w = qt.weights_of('duo')
    other = {k: v.copy() for k, v in w.items()}
    other['v0.weight'], other['v0.bias'] = np.roll(w['v0.weight'], 1, axis=0), np.roll(w['v0.bias'], 1)
    tied = {k: v.copy() for k, v in w.items()}
    tied['v0.weight'][:] = w['v0.weight'][3]
    tied['v0.bias'][:] = w['v0.bias'][3]
    net = qnet.QNetwork.from_module(w, DEV)
    term, r, d = terminal.cpu().numpy() != 0, reward.cpu().numpy(), discount.cpu().numpy()
    qs = net.forward(nf).cpu().numpy()
    assert term.any() and not term.all()
    for online_w, what in ((other, 'other'), (tied, 'tied'), (w, 'self')):
        online = qnet.QNetwork.from_module(online_w, DEV)
        qon = online.forward(nf).cpu().numpy()
        pick = np.argmax(qon, 1)
        if what == 'other':
            assert (pick != np.argmax(qs, 1)).any()                    # the two networks prefer other actions
        if what == 'tied':
            assert (qon == qon[:, :1]).all() and (pick == 0).all()     # ties go to the first index
        want = np.where(term, r, d * qs[np.arange(N), pick])
        got = net.td_targets(reward, discount, nf, terminal, online=online)
        assert got.dtype == torch.float32 and _same(got, want.astype(np.float32)), what
    # Q_self[argmax Q_self] is the maximum: double with itself is the plain target, which is what it was
    plain = net.td_targets(reward, discount, nf, terminal)
    assert _bits(plain) == _bits(got)
    assert _bits(plain) == _bits(torch.where(terminal.to(torch.bool), reward, discount * net.qmax(nf)))
    assert _same(plain[terminal != 0], r[term])
    with pytest.raises(ValueError, match='another shape'):
        net.td_targets(reward, discount, nf, terminal, online=qnet.QNetwork.from_module(qt.weights_of('duo', nout=3), DEV))


# ---------------------------------------------------------------------------
# the trainer's options

SEED = 5


def _pieces():
    N = 64
    env = BatchedEnv(gio.configs()['short'], N, device=DEV, b_cap=32)
    env.reset()
    net = _duo()
    buf = replay.ReplayBuffer(N, env.p_pad + env.b_cap, 2, 12, n_steps=4, device=DEV)
    eg = actor.EpsilonGreedy(env, t_in=0.2, t_out=0.1, seed=3)
    return env, net, buf, eg


def _result(net, target, opt, buf, eg):
    return (_bits(net.weights), None if target is None else _bits(target.weights),
            None if opt is None or opt.state is None else _bits(opt.state), _bits(buf.loss), _bits(eg.policy))


def _trainer_run(make_opt, **kw):
    env, net, buf, eg = _pieces()
    opt = make_opt()
    tr = train.QTrainer(env, net, buf, eg, n_samples=32, seed=SEED, optimizer=opt, **kw)
    script_ok = differs = 0
    for t in range(20):
        script = env.controls('script', SEED, t)[:, 1].clone()
        greedy = env.qcontrols(net, tick0=t)[:, 1].clone()      # (no explore: its state is the trainer's to advance)
        tr.tick()
        script_ok += int(torch.equal(buf.action[t % 12][:, 1], script))
        differs += int(not torch.equal(script, greedy))
    env.check_errors()
    return _result(net, tr.target, opt, buf, eg), tr, script_ok, differs


def _written_out(make_opt, sync_every=None, tau=1.0, double=False, opponent=None):
    """The trainer's loop from the pieces, as the README writes it."""
    env, net, buf, eg = _pieces()
    opt = make_opt()
    target = net.clone() if (sync_every or tau != 1.0) else None
    nstep = 0
    for t in range(20):
        env.features(out=buf.head())
        control = env.qcontrols(net, tick0=t, explore=eg)
        if opponent is not None:
            control[:, 1] = env.controls(opponent, SEED, t)[:, 1]
        _, reward, done = env.step(control)
        buf.push(control, reward, done)
        if buf.eligible_lower_bound() < 32:
            continue
        ids = buf.sample(32, seed=SEED, draw=t)
        f, a, r, d, nf, term = buf.gather(ids)
        valuer = net if target is None else target
        y = valuer.td_targets(r, d, nf, term, online=net) if double else valuer.td_targets(r, d, nf, term)
        if opt is None:
            loss = net.sgd_step(f, a, y, lr=1e-2)
        else:
            loss, grad = net.grad(f, a, y)
            follow = target if (sync_every is None or (nstep + 1) % sync_every == 0) else None
            opt.apply(net, grad, target=follow, tau=tau)
        buf.update_loss(ids, loss)
        nstep += 1
    return _result(net, target, opt, buf, eg), nstep


@pytest.mark.parametrize('case', ['adam_sync3_double_script', 'adam_polyak', 'defaults'])
def test_qtrainer_options_are_the_loop_written_out(case):
    if case == 'adam_sync3_double_script':
        kw, loop = dict(target_sync=3, double=True, opponent='script'), dict(sync_every=3, double=True, opponent='script')
        make_opt = optim.Adam
    elif case == 'adam_polyak':
        kw, loop, make_opt = dict(target_sync=0.05), dict(tau=0.05), optim.Adam
    else:
        kw, loop, make_opt = {}, {}, lambda: None
    one, tr, script_ok, differs = _trainer_run(make_opt, **kw)
    two, _, _, _ = _trainer_run(make_opt, **kw)
    assert one == two                                             # reproducible bit for bit
    out, nstep = _written_out(make_opt, **loop)
    assert out == one and nstep == tr.nstep == 16
    start = _bits(_duo().weights)
    assert one[0] != start and np.isfinite(np.frombuffer(one[0], np.float32)).all()
    if case == 'defaults':
        assert tr.target is None and tr.optimizer is None and one[1] is None and one[2] is None
        assert script_ok < 20                                     # the network plays ship 1
        return
    assert tr.optimizer.t == 16 and int(tr.optimizer.skipped) == 0
    assert one[1] not in (start, one[0])                          # the target moved, and is not the online network
    if case == 'adam_sync3_double_script':
        assert script_ok == 20 and differs > 0                    # ship 1 is ScriptBot on every tick, not the network
        assert tr.sync_every == 3 and tr.tau == 1.0
    else:
        assert tr.sync_every is None and tr.tau == 0.05


def test_qtrainer_rejects_what_it_cannot_do():
    env, net, buf, eg = _pieces()
    with pytest.raises(ValueError, match='needs an optimizer'):
        train.QTrainer(env, net, buf, eg, target_sync=3)
    for bad in (0, 1.0, True, 'x'):
        with pytest.raises(ValueError, match='target_sync'):
            train.QTrainer(env, net, buf, eg, optimizer=optim.Adam(), target_sync=bad)
    with pytest.raises(ValueError, match='opponent'):
        train.QTrainer(env, net, buf, eg, opponent='human')


@pytest.mark.parametrize('kind,kw', qo.FIT_RULES, ids=['sgd', 'momentum', 'rmsprop', 'adagrad', 'adam'])
def test_each_rule_fits_a_fixed_batch(kind, kw):
    """The CPU test's batch and settings with net.step: the mean loss falls."""
    x, action, target = qo.fixed_batch()
    f, a, y = _dev(x), _dev(action), _dev(target)
    net = qnet.QNetwork(qo.fit_weights(), 2, 6, DEV)
    opt = qo.make(kind, kw)
    first = float(net.step(f, a, y, opt).mean())
    for _ in range(qo.FIT_STEPS - 1):
        net.step(f, a, y, opt)
    last = float(net.grad(f, a, y)[0].mean())
    print(kind, kw, first, last)
    assert opt.t == qo.FIT_STEPS and int(opt.skipped) == 0
    assert np.isfinite(last) and last < first
