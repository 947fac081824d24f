"""Shared by tests/test_qopt_host.py and tests/test_gpu_qopt.py: the optimiser
configurations, the gradients, the fixed batch both fit tests train on, and the
derived bound of the float32 mirror against torch.optim in float64."""
import functools

import numpy as np

from astro_amd import optim, qnet
from oracle import batched, features
from tests import golden_io as gio
from tests import qtrain_util as qt

# (name, kind, arguments): the issue's six configurations, then SGD without momentum
CONFIGS = [
    ('sgd_momentum', 'sgd', dict(lr=1e-2, momentum=0.9)),
    ('sgd_nesterov_decay', 'sgd', dict(lr=1e-2, momentum=0.9, nesterov=True, weight_decay=1e-4)),
    ('rmsprop', 'rmsprop', dict(lr=1e-2, alpha=0.99, eps=1e-3)),
    ('adagrad', 'adagrad', dict(lr=1e-2, eps=1e-10)),
    ('adam', 'adam', dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)),
    ('adam_decay', 'adam', dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)),
    ('sgd_plain', 'sgd', dict(lr=1e-2)),
]
SIX = CONFIGS[:6]
CLASSES = {'sgd': optim.SGD, 'rmsprop': optim.RMSprop, 'adagrad': optim.Adagrad, 'adam': optim.Adam}
NSTATE = {'sgd': 1, 'rmsprop': 1, 'adagrad': 1, 'adam': 2}


def nstate(kind, kw):
    return 0 if kind == 'sgd' and not kw.get('momentum') else NSTATE[kind]


def make(kind, kw, **more):
    return CLASSES[kind](**dict(kw, **more))


def wide_grads(rng, steps, n):
    """randn * 10^U(-6, 1) with 5 % exact zeros, float32 [steps, n]."""
    g = rng.standard_normal((steps, n)) * 10.0 ** rng.uniform(-6, 1, size=(steps, n))
    g[rng.random((steps, n)) < 0.05] = 0.0
    return g.astype(np.float32)


def normal_grads(rng, steps, n):
    """Magnitudes 0 (5 %) or in [1e-6, 10], random signs: no intermediate of a
    step is subnormal.  float32 [steps, n]."""
    g = 10.0 ** rng.uniform(-6, 1, size=(steps, n)) * rng.choice([-1.0, 1.0], size=(steps, n))
    g[rng.random((steps, n)) < 0.05] = 0.0
    g = g.astype(np.float32)
    assert ((g == 0) | ((np.abs(g) >= np.float32(1e-6)) & (np.abs(g) <= 10))).all()
    return g


def start_weights(rng, n):
    return (rng.standard_normal(n) * 0.3).astype(np.float32)


# ---------------------------------------------------------------------------
# the bound: R * 2^-24 * M per element.  M is the header's formula in float64
# on magnitudes (|operand| for every operand, + for every -); R counts the
# float32 roundings on the longest chain to the output, every host scalar that
# is rounded once (coef, 1 - alpha, 1 - beta, step_size, bc2) counting as one.
# A chain that runs through g * g meets g's roundings in both operands, so they
# count twice there (d(g^2)/g^2 = 2 dg/g); through sqrt(v) the count so far
# halves, rounded up (d(sqrt v)/sqrt v = dv/v / 2).  Where chains join (a sum,
# a quotient) the longest counts.  R is at most 11 for every kind.

def _half(r):
    return (r + 1) // 2


def bound(kind, h, w, g, state, norm):
    """-> (M_w, R_w, [(M_s, R_s) per state array]) for one step from float32 w, g, state."""
    f = lambda x: float(x)  # noqa: E731
    W, G = np.abs(w.astype(np.float64)), np.abs(g.astype(np.float64))
    S = [np.abs(s.astype(np.float64)) for s in state]
    rg = 0
    if h['max_norm'] > 0:
        G = min(1.0, f(h['max_norm']) / (float(norm) + 1e-6)) * G
        rg = 2                                  # coef, coef * g
    if h['weight_decay'] != 0:
        G = G + f(h['weight_decay']) * W
        rg = max(rg, 1) + 1                     # wd * w, the add
    lr, eps = f(h['lr']), f(h['eps'])
    if kind == 'sgd':
        mu = f(h['momentum'])
        if mu == 0:
            return W + lr * G, rg + 2, []
        B = mu * S[0] + G
        rb = max(1, rg) + 1                     # mu * b, the add
        D, rd = (G + mu * B, rb + 2) if h['nesterov'] else (B, rb)
        return W + lr * D, rd + 2, [(B, rb)]
    if kind in ('rmsprop', 'adagrad'):
        if kind == 'rmsprop':
            V = f(h['alpha']) * S[0] + f(h['one_minus_alpha']) * (G * G)
            rv = 2 * rg + 3                     # g * g, (1 - alpha) * it, the add
        else:
            V = S[0] + G * G
            rv = 2 * rg + 2
        with np.errstate(divide='ignore', invalid='ignore'):
            Q = np.where(G == 0, 0.0, G / (np.sqrt(V) + eps))
        return W + lr * Q, max(rg, _half(rv) + 2) + 3, [(V, rv)]    # sqrt, + eps | /, lr *, the subtraction
    M = f(h['beta1']) * S[0] + f(h['one_minus_beta1']) * G
    rm = max(1, rg) + 2
    V = f(h['beta2']) * S[1] + f(h['one_minus_beta2']) * (G * G)
    rv = 2 * rg + 3
    with np.errstate(divide='ignore', invalid='ignore'):
        Q = np.where(M == 0, 0.0, M / (np.sqrt(V) / f(h['bc2']) + eps))
    # sqrt, / bc2, + eps | /, step_size *, the subtraction
    return W + f(h['step_size']) * Q, max(rm, _half(rv) + 3) + 3, [(M, rm), (V, rv)]


def torch_step(kind, kw, t, w, g, state, max_norm=None):
    """One step of torch.optim's rule in float64 from the float32 w, g, state
    (the step counter set to t - 1), after clip_grad_norm_ if max_norm."""
    import torch
    f = lambda x: float(np.float32(x))  # noqa: E731
    p = torch.nn.Parameter(torch.from_numpy(w.astype(np.float64)))
    p.grad = torch.from_numpy(g.astype(np.float64))
    T = lambda a: torch.from_numpy(a.astype(np.float64))  # noqa: E731
    step = torch.tensor(float(t - 1), dtype=torch.float64)
    wd = f(kw.get('weight_decay', 0.0))
    if kind == 'sgd':
        o = torch.optim.SGD([p], lr=f(kw['lr']), momentum=f(kw.get('momentum', 0.0)),
                            nesterov=bool(kw.get('nesterov', False)), weight_decay=wd)
        if state:
            o.state[p]['momentum_buffer'] = T(state[0])
        names = ['momentum_buffer'] if state else []
    elif kind == 'rmsprop':
        o = torch.optim.RMSprop([p], lr=f(kw['lr']), alpha=f(kw['alpha']), eps=f(kw['eps']), weight_decay=wd)
        o.state[p].update(step=step, square_avg=T(state[0]))
        names = ['square_avg']
    elif kind == 'adagrad':
        o = torch.optim.Adagrad([p], lr=f(kw['lr']), eps=f(kw['eps']), weight_decay=wd)
        o.state[p].update(step=step, sum=T(state[0]))
        names = ['sum']
    else:
        o = torch.optim.Adam([p], lr=f(kw['lr']), betas=(f(kw['betas'][0]), f(kw['betas'][1])), eps=f(kw['eps']),
                             weight_decay=wd)
        o.state[p].update(step=step, exp_avg=T(state[0]), exp_avg_sq=T(state[1]))
        names = ['exp_avg', 'exp_avg_sq']
    if max_norm is not None:
        torch.nn.utils.clip_grad_norm_([p], f(max_norm))
    o.step()
    return p.detach().numpy(), [o.state[p][k].numpy() for k in names]


# ---------------------------------------------------------------------------
# the fixed batch of the two fit tests

FIT_STEPS = 50
FIT_RULES = [('sgd', dict(lr=1e-2)), ('sgd', dict(lr=1e-2, momentum=0.9)), ('rmsprop', {}), ('adagrad', {}),
             ('adam', {})]


@functools.lru_cache(maxsize=None)
def fixed_batch():
    """(features float32 [64, 24, 15], action int8 [64], target float32 [64]):
    the features of 64 two-ship games the oracle stepped 40 ticks under random
    controls, with fixed random actions and targets."""
    cfg = gio.configs()['short']
    P = batched.make_params(cfg)
    rng = np.random.RandomState(17)
    B = batched.create(np.arange(100, 164, dtype=np.uint32), P, p_pad=8, b_cap=16)
    for _ in range(40):
        B, _, done = batched.step(B, rng.randint(0, 6, size=(64, 2)).astype(np.int8), P, store='f32')
        fin = np.nonzero(done)[0]
        if fin.size:
            B.put(fin, batched.create(rng.randint(1, 1 << 30, size=fin.size).astype(np.uint32), P, p_pad=8, b_cap=16))
    x = np.ascontiguousarray(features.batched(B, 2, 24))
    assert (x[:, 0, 0] >= 0).all() and (x[:, :, 0] == 1).any()      # every sample is live; there are bullets
    return x, rng.randint(0, 6, size=64).astype(np.int8), rng.uniform(-1, 1, size=64).astype(np.float32)


def fit_weights():
    return qnet.pack(qt.weights_of('duo'))
