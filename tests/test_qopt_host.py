"""CPU-only checks of the optimiser library's host side: libastro_qopt.so's
argument checks and astro_amd/optim.py's numpy mirror against torch.optim in
float64."""
import ctypes

import numpy as np
import pytest

import __graft_entry__ as entry
from astro_amd import _lib, optim, qnet
from tests import qopt_util as qo
from tests import test_libraries as libraries

U = 2.0 ** -24


def test_header_compiles_as_c_and_matches_the_ctypes_layout(tmp_path):
    """AstroQOpt (64 bytes), the ABI number, the kinds and limits: the qopt row's layout and constants cases."""
    libraries.test_struct_layouts_are_the_ctypes_mirrors('qopt', tmp_path)
    libraries.test_header_constants_are_the_python_ones('qopt', tmp_path)


def _opt(**kw):
    """A valid ADAM struct with the given fields overwritten."""
    h = optim.hyper('adam')
    c = _lib.AstroQOpt(kind=h['kind'], nesterov=h['nesterov'], **{k: float(h[k]) for k in optim._F})
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_bad_arguments_without_gpu():
    """Every bad argument has its own negative code and a message, and is
    rejected before the device is touched (the pointers are not memory)."""
    entry.build()
    lib = _lib.load_qopt()
    P = ctypes.c_void_p

    def step(opt=None, n=4934, grad=P(0x1000), w=P(0x2000), s1=P(0x3000), s2=P(0x4000), target=P(0x5000),
             norm=P(0x6000), skipped=P(0x7000), null=False):
        opt = _opt() if opt is None else opt
        rc = lib.astro_qopt_step(None if null else ctypes.byref(opt), n, grad, w, s1, s2, target, norm, skipped, None)
        return rc, lib.astro_qopt_last_error().decode()

    nan, inf = float('nan'), float('inf')
    cases = [
        (dict(null=True), -100, 'opt is NULL'),
        (dict(opt=_opt(kind=4)), -101, 'kind'), (dict(opt=_opt(kind=-1)), -101, 'kind'),
        (dict(n=0), -102, 'nparams'), (dict(n=-5), -102, 'nparams'), (dict(n=(1 << 20) + 1), -102, 'nparams'),
        (dict(opt=_opt(tau=0.0)), -103, 'tau'), (dict(opt=_opt(tau=1.5)), -103, 'tau'),
        (dict(opt=_opt(tau=-0.1)), -103, 'tau'), (dict(opt=_opt(tau=nan)), -103, 'tau'),
        (dict(opt=_opt(lr=nan)), -104, 'finite'), (dict(opt=_opt(eps=inf)), -104, 'finite'),
        (dict(opt=_opt(lr=-1.0)), -104, '>= 0'), (dict(opt=_opt(momentum=-0.5)), -104, '>= 0'),
        (dict(opt=_opt(bc2=0.0)), -104, 'bc2'), (dict(opt=_opt(bc2=1.5)), -104, 'bc2'),
        (dict(grad=None), -110, 'grad is NULL'), (dict(w=None), -111, 'weights is NULL'),
        (dict(s1=None), -112, 'state1'), (dict(opt=_opt(kind=1), s1=None), -112, 'state1'),
        (dict(opt=_opt(kind=2), s1=None), -112, 'state1'), (dict(opt=_opt(kind=0, momentum=0.9), s1=None), -112, 'state1'),
        (dict(s2=None), -113, 'state2'),
        (dict(target=P(0x2000)), -114, 'target is weights'),
        (dict(grad=P(0x1002)), -119, 'aligned'), (dict(w=P(0x2001)), -119, 'aligned'),
        (dict(s1=P(0x3002)), -119, 'aligned'), (dict(s2=P(0x4003)), -119, 'aligned'),
        (dict(target=P(0x5002)), -119, 'aligned'), (dict(norm=P(0x6002)), -119, 'aligned'),
        (dict(skipped=P(0x7001)), -119, 'aligned'),
    ]
    codes = set()
    for kw, code, word in cases:
        rc, msg = step(**kw)
        assert rc == code and word in msg, (kw, rc, msg)
        codes.add(rc)
    assert sorted(codes) == [-119, -114, -113, -112, -111, -110, -104, -103, -102, -101, -100]
    # the documented order: each case breaks the rule of its code and every later one
    bad_ptr = dict(grad=None, w=None, s1=None, s2=None)
    assert step(opt=_opt(kind=9, tau=2.0, lr=nan), n=0, **bad_ptr)[0] == -101
    assert step(opt=_opt(tau=2.0, lr=nan), n=0, **bad_ptr)[0] == -102
    assert step(opt=_opt(tau=2.0, lr=nan), **bad_ptr)[0] == -103
    assert step(opt=_opt(lr=nan), **bad_ptr)[0] == -104
    assert step(**bad_ptr)[0] == -110
    assert step(w=None, s1=None, s2=None)[0] == -111
    assert step(s1=None, s2=None, target=P(0x2000))[0] == -112
    assert step(s2=None, target=P(0x2000))[0] == -113
    assert step(target=P(0x2000), grad=P(0x1002))[0] == -114
    # the bounds themselves pass the scalar checks and stop at the next rule; what a kind does not need may be NULL
    assert step(n=1, grad=None)[0] == -110 and step(n=1 << 20, grad=None)[0] == -110
    assert step(opt=_opt(tau=1.0), grad=None)[0] == -110
    assert step(opt=_opt(kind=0), s1=None, s2=None, target=None, norm=None, skipped=None, grad=P(0x1002))[0] == -119
    assert step(opt=_opt(kind=1), s2=None, grad=P(0x1002))[0] == -119


# ---------------------------------------------------------------------------
# the mirror against torch.optim in float64

def _compare(name, kind, kw, max_norm=None, steps=30, n=4934):
    """Teacher-forced: every step starts both sides from the mirror's float32
    weights and state.  Returns the worst error / (2^-24 M) per output."""
    rng = np.random.default_rng(sum(map(ord, name)))
    grads = qo.wide_grads(rng, steps, n)
    opt = qo.make(kind, kw, max_norm=max_norm)
    w = qo.start_weights(rng, n)
    state = tuple(np.zeros(n, np.float32) for _ in range(qo.nstate(kind, kw)))
    worst = {}
    for t in range(1, steps + 1):
        h = opt.hyper(t)
        g = grads[t - 1]
        w2, state2, _, norm, skipped = optim.step_host(kind, h, w, g, state)
        assert not skipped and w2.dtype == np.float32
        tw, tstate = qo.torch_step(kind, kw, t, w, g, state, max_norm)
        m_w, r_w, ms = qo.bound(kind, h, w, g, state, norm)
        assert r_w <= 12 and all(r <= 12 for _, r in ms) and len(ms) == len(state2) == len(tstate)
        for what, got, want, m, r in [('w', w2, tw, m_w, r_w)] + [
                ('state%d' % i, state2[i], tstate[i], ms[i][0], ms[i][1]) for i in range(len(ms))]:
            err = np.abs(got.astype(np.float64) - want)
            assert (err <= r * U * m).all(), (name, what, t, float((err / (U * m + 1e-300)).max()), r)
            ratio = float((err[m > 0] / (U * m[m > 0])).max())
            worst[what] = max(worst.get(what, 0.0), ratio)
        w, state = w2, state2
    assert np.isfinite(w).all()
    return worst


@pytest.mark.parametrize('name,kind,kw', qo.SIX, ids=[c[0] for c in qo.SIX])
def test_step_host_equals_torch_optim_within_the_rounding_bound(name, kind, kw):
    worst = _compare(name, kind, kw)
    print(name, {k: round(v, 2) for k, v in worst.items()})
    assert max(worst.values()) > 0.05          # float32 against float64: the comparison is not vacuous


@pytest.mark.parametrize('name,kind,kw', qo.SIX, ids=[c[0] for c in qo.SIX])
def test_clipped_step_host_equals_clip_grad_norm_then_torch_optim(name, kind, kw):
    worst = _compare(name, kind, kw, max_norm=5.0)      # the drawn gradients' norms are about a hundred
    print(name, {k: round(v, 2) for k, v in worst.items()})


def test_clip_and_guard_on_the_host():
    rng = np.random.default_rng(3)
    n = 1025
    for name, kind, kw in qo.CONFIGS:
        g = qo.normal_grads(rng, 1, n)[0]
        w = qo.start_weights(rng, n)
        state = tuple((rng.random(n) * 0.1).astype(np.float32) for _ in range(qo.nstate(kind, kw)))
        target = qo.start_weights(rng, n)
        plain = optim.step_host(kind, qo.make(kind, kw).hyper(3), w, g, state, target=target, tau=0.25)
        norm = plain[3]
        assert norm == optim.norm_host(g) and abs(norm - np.sqrt((g.astype(np.float64) ** 2).sum())) <= 1e-12 * norm
        # a norm below max_norm: coef = 1 and the same bits
        loose = optim.step_host(kind, qo.make(kind, kw, max_norm=float(norm) * 1.01).hyper(3), w, g, state,
                                target=target, tau=0.25)
        assert optim.clip_coef(norm, float(norm) * 1.01) == 1
        for a, b in zip([plain[0], *plain[1], plain[2]], [loose[0], *loose[1], loose[2]]):
            assert a.tobytes() == b.tobytes()
        tight = optim.step_host(kind, qo.make(kind, kw, max_norm=float(norm) / 3).hyper(3), w, g, state)
        assert tight[0].tobytes() != plain[0].tobytes()
        # all zeros: coef = 1, norm 0
        zero = optim.step_host(kind, qo.make(kind, kw, max_norm=1.0).hyper(3), w, np.zeros(n, np.float32), state)
        assert zero[3] == 0 and not zero[4] and optim.clip_coef(0.0, 1.0) == 1
        # a NaN, an inf: skipped, nothing changed
        for poison, at in ((np.nan, 7), (np.inf, n - 1), (-np.inf, 0)):
            gp = g.copy()
            gp[at] = poison
            w2, s2, t2, nrm, skipped = optim.step_host(kind, qo.make(kind, kw, max_norm=1.0).hyper(3), w, gp, state,
                                                       target=target, tau=0.25)
            assert skipped and not np.isfinite(nrm)
            assert w2.tobytes() == w.tobytes() and t2.tobytes() == target.tobytes()
            assert all(a.tobytes() == b.tobytes() for a, b in zip(s2, state))
    # tau = 1 is an exact copy, tau < 1 the three-rounding blend
    out = optim.step_host('sgd', optim.hyper('sgd'), w, g, (), target=target, tau=1.0)
    assert out[2].tobytes() == out[0].tobytes()
    out = optim.step_host('sgd', optim.hyper('sgd'), w, g, (), target=target, tau=0.25)
    assert out[2].tobytes() == (target + np.float32(0.25) * (out[0] - target)).tobytes()


def test_adam_scalars():
    lr, b1, b2 = np.float32(1e-3), np.float32(0.9), np.float32(0.999)
    ss, bc = optim.adam_scalars(1e-3, 0.9, 0.999, 1)
    assert ss.dtype == bc.dtype == np.float32
    assert ss == np.float32(float(lr) / (1.0 - float(b1))) and bc == np.float32(np.sqrt(1.0 - float(b2)))
    for t in (10 ** 6, 10 ** 9):
        ss, bc = optim.adam_scalars(1e-3, 0.9, 0.999, t)
        assert ss == lr and bc == 1
    seq = [optim.adam_scalars(1e-3, 0.9, 0.999, t) for t in range(1, 20000)]
    ss, bc = np.array([s for s, _ in seq]), np.array([b for _, b in seq])
    assert (np.diff(ss) <= 0).all() and (np.diff(bc) >= 0).all() and ss[0] > ss[-1] and bc[0] < bc[-1] == 1
    with pytest.raises(ValueError):
        optim.adam_scalars(1e-3, 0.9, 0.999, 0)
    # the complements: float64 of the float32 value, rounded once
    h = optim.hyper('adam')
    assert h['one_minus_beta1'] == np.float32(1.0 - float(b1)) != np.float32(1.0 - 0.9)
    assert h['one_minus_beta2'] == np.float32(1.0 - float(b2)) and h['one_minus_alpha'] == np.float32(1.0 - float(np.float32(0.99)))
    assert all(isinstance(h[k], np.float32) for k in optim._F) and set(h) == {f for f, _ in _lib.AstroQOpt._fields_}
    o = optim.Adam()
    assert o.hyper() == optim.hyper('adam', lr=1e-3) and o.t == 0 and o.state is None


def test_python_surface():
    import astro_amd
    from astro_amd import train
    for name in ('SGD', 'RMSprop', 'Adagrad', 'Adam'):
        assert getattr(astro_amd, name) is getattr(optim, name)
    assert (optim.RMSprop().h['lr'], optim.RMSprop().h['eps']) == (np.float32(1e-2), np.float32(1e-3))
    assert optim.Adagrad().h['eps'] == np.float32(1e-10) and optim.Adam().h['lr'] == np.float32(1e-3)
    assert optim.SGD(0.1).nstate == 0 and optim.SGD(0.1, momentum=0.5).nstate == 1
    with pytest.raises(ValueError):
        optim.SGD(0.1, nesterov=True)
    with pytest.raises(ValueError):
        optim.Adam(max_norm=0.0)
    names = train.QTrainer.__init__.__code__.co_varnames
    assert names[:9] == ('self', 'env', 'net', 'buf', 'explore', 'n_samples', 'n_ministeps', 'lr', 'seed')
    assert names[9:13] == ('optimizer', 'target_sync', 'double', 'opponent')
    assert 'online' in qnet.QNetwork.td_targets.__code__.co_varnames
    for name in ('clone', 'copy_from', 'step', 'sgd_step'):
        assert callable(getattr(qnet.QNetwork, name))


@pytest.mark.parametrize('kind,kw', qo.FIT_RULES, ids=['sgd', 'momentum', 'rmsprop', 'adagrad', 'adam'])
def test_each_rule_fits_a_fixed_batch(kind, kw):
    """grad64 and step_host for 50 steps on the fixed batch: the mean loss falls."""
    x, action, target = qo.fixed_batch()
    opt = qo.make(kind, kw)
    w = qo.fit_weights()
    state = tuple(np.zeros(w.size, np.float32) for _ in range(qo.nstate(kind, kw)))
    first = None
    for t in range(1, qo.FIT_STEPS + 1):
        loss, g = qnet.grad64(qnet.unpack(w, 2, 6), x, action, target)
        first = loss.mean() if first is None else first
        w, state, _, _, skipped = optim.step_host(kind, opt.hyper(t), w, qnet.pack(g), state)
        assert not skipped
    last = qnet.grad64(qnet.unpack(w, 2, 6), x, action, target)[0].mean()
    print(kind, kw, first, last)
    assert np.isfinite(last) and last < first
