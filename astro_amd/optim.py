"""torch.optim's SGD, RMSprop, Adagrad and Adam for a ``qnet.QNetwork``: the
candidates of the reference's trainer (astro/rl.py:172-176; Rprop is left
out), stepping the packed weight buffer in place in one launch
(csrc/astro_qopt.hip, include/astro_qopt.h) -- with the gradient-norm clipping
of ``torch.nn.utils.clip_grad_norm_``, a guard that skips a step whose gradient
is not finite, and the update of a target network, all in that launch.

* ``SGD`` / ``RMSprop`` / ``Adagrad`` / ``Adam`` own their state tensors, the
  step count ``t`` and the device scalars ``norm`` and ``skipped``;
  ``opt.apply(net, grad)`` is the launch.  ``QNetwork.step`` is ``grad`` then
  ``apply``.
* ``step_host`` is the same step in numpy float32, in the operation order the
  header states: the kernel equals it bit for bit (the tests' truth, as
  ``actor.explore_host`` is for the exploration).
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib

KINDS = _lib.QOPT_KINDS
THREADS = _lib.QOPT_THREADS
_F = [name for name, ctype in _lib.AstroQOpt._fields_ if ctype is ctypes.c_float]


def f32(x):
    return np.float32(x)


def adam_scalars(lr, beta1, beta2, t):
    """Adam's two per-step scalars for step t = 1, 2, ...: (step_size = lr /
    (1 - beta1^t), bc2 = sqrt(1 - beta2^t)), each computed in float64 from the
    float32 hyperparameters and rounded once to float32."""
    lr, beta1, beta2, t = float(f32(lr)), float(f32(beta1)), float(f32(beta2)), int(t)
    if t < 1:
        raise ValueError('t counts the steps from 1, got %d' % t)
    return f32(lr / (1.0 - beta1 ** t)), f32(math.sqrt(1.0 - beta2 ** t))


def hyper(kind, t=1, lr=1e-2, momentum=0.0, nesterov=False, weight_decay=0.0, max_norm=None, alpha=0.99,
          betas=(0.9, 0.999), eps=1e-8, tau=1.0):
    """The fields of AstroQOpt for step ``t`` as a dict: ``kind`` and
    ``nesterov`` ints, everything else its float32 value.  The complements 1 -
    alpha, 1 - beta1, 1 - beta2 are computed in float64 from the float32
    hyperparameter and rounded once."""
    if kind not in KINDS:
        raise ValueError('kind must be one of %s' % sorted(KINDS))
    h = dict(kind=KINDS[kind], nesterov=int(bool(nesterov)), lr=f32(lr), weight_decay=f32(weight_decay),
             max_norm=f32(0.0 if max_norm is None else max_norm), momentum=f32(momentum), alpha=f32(alpha),
             beta1=f32(betas[0]), beta2=f32(betas[1]), eps=f32(eps), tau=f32(tau))
    for name in ('alpha', 'beta1', 'beta2'):
        h['one_minus_' + name] = f32(1.0 - float(h[name]))
    h['step_size'], h['bc2'] = adam_scalars(h['lr'], h['beta1'], h['beta2'], t)
    if max_norm is not None and not float(h['max_norm']) > 0.0:
        raise ValueError('max_norm must be positive (None: no clipping)')
    return h


def norm_host(grad):
    """The gradient's norm as the kernel adds it up, float64: thread t of 1024
    adds the squares of grad[t], grad[t + 1024], ... in that order, then the
    partials are folded in halves (512, 256, ..., 1)."""
    g = np.asarray(grad, dtype=np.float32).astype(np.float64).ravel()
    sq = np.zeros(-(-g.size // THREADS) * THREADS, np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        sq[:g.size] = g * g
        s = np.zeros(THREADS, np.float64)
        for row in sq.reshape(-1, THREADS):
            s = s + row
        h = THREADS // 2
        while h >= 1:
            s = s[:h] + s[h:2 * h]
            h //= 2
        return np.sqrt(s[0])


def clip_coef(norm, max_norm):
    """float32(min(1, max_norm / (norm + 1e-6))) in float64 (clip_grad_norm_)."""
    return f32(min(1.0, float(f32(max_norm)) / (float(norm) + 1e-6)))


def step_host(kind, hyper, w, grad, state, t=None, target=None, tau=None):
    """One optimiser step in numpy float32, in include/astro_qopt.h's order of
    operations.  hyper: the dict of ``hyper`` (or ``opt.hyper(t)``); with ``t``
    given, Adam's two scalars are recomputed for that step; with ``tau`` given it
    replaces the dict's.  w, grad: float32 [n]; state: a sequence of the kind's
    state arrays (SGD: (b,) or () without momentum; RMSprop, Adagrad: (v,); Adam:
    (m, v)); target: float32 [n] or None.  Nothing is changed in place.  Returns
    (w, state tuple, target, norm float64, skipped bool)."""
    h = dict(hyper)
    if KINDS[kind] != h['kind']:
        raise ValueError('hyper is of another kind')
    if t is not None:
        h['step_size'], h['bc2'] = adam_scalars(h['lr'], h['beta1'], h['beta2'], t)
    tau = h['tau'] if tau is None else f32(tau)
    w = np.array(w, dtype=np.float32)
    g = np.array(grad, dtype=np.float32)
    state = tuple(np.array(s, dtype=np.float32) for s in state)
    target = None if target is None else np.array(target, dtype=np.float32)
    norm = norm_host(g)
    if not np.isfinite(norm):
        return w, state, target, norm, True
    with np.errstate(all='ignore'):
        if h['max_norm'] > 0:
            g = clip_coef(norm, h['max_norm']) * g
        if h['weight_decay'] != 0:
            g = g + h['weight_decay'] * w
        if kind == 'sgd':
            if h['momentum'] != 0:
                b = h['momentum'] * state[0] + g
                state = (b,)
                g = g + h['momentum'] * b if h['nesterov'] else b
            w = w - h['lr'] * g
        elif kind == 'rmsprop':
            v = h['alpha'] * state[0] + h['one_minus_alpha'] * (g * g)
            state = (v,)
            w = w - h['lr'] * (g / (np.sqrt(v) + h['eps']))
        elif kind == 'adagrad':
            v = state[0] + g * g
            state = (v,)
            w = w - h['lr'] * (g / (np.sqrt(v) + h['eps']))
        else:
            m = h['beta1'] * state[0] + h['one_minus_beta1'] * g
            v = h['beta2'] * state[1] + h['one_minus_beta2'] * (g * g)
            state = (m, v)
            w = w - h['step_size'] * (m / (np.sqrt(v) / h['bc2'] + h['eps']))
        if target is not None:
            target = w.copy() if tau == 1 else target + tau * (w - target)
    assert w.dtype == np.float32 and all(s.dtype == np.float32 for s in state)
    return w, state, target, norm, False


class Optimizer:
    """What the four rules share.  Bound to a ``QNetwork`` on the first
    ``apply``; ``state`` is a float32 [nstate, nparams] tensor of zeros until
    then stepped; ``t`` counts the calls of ``apply`` -- the host's count: a
    step the device skipped (``skipped``, a device int32 [1], counts those)
    still advances it, because reading ``skipped`` would synchronise.  ``norm``
    (device float32 [1]) is the last gradient's norm before clipping."""

    kind = None
    nstate = 0

    def __init__(self, **kw):
        self._kw = kw
        self.h = hyper(self.kind, **kw)        # every hyperparameter as its float32 value
        self.t = 0
        self.net = self.state = self.norm = self.skipped = None

    def hyper(self, t=None, tau=1.0):
        """AstroQOpt's fields for step t (default: the next one)."""
        h = dict(self.h)
        h['step_size'], h['bc2'] = adam_scalars(h['lr'], h['beta1'], h['beta2'], self.t + 1 if t is None else t)
        h['tau'] = f32(tau)
        return h

    def _bind(self, net):
        if self.net is None:
            dev = net.weights.device
            self.net = net
            self.state = torch.zeros((self.nstate, net.weights.numel()), dtype=torch.float32, device=dev)
            self.norm = torch.zeros(1, dtype=torch.float32, device=dev)
            self.skipped = torch.zeros(1, dtype=torch.int32, device=dev)
        elif net is not self.net:
            raise ValueError('this optimizer is bound to another QNetwork (its state is that network\'s)')

    def apply(self, net, grad, target=None, tau=1.0):
        """One step on ``net.weights`` in place from ``grad`` (float32
        [nparams], not written), one launch on the current stream.  target: a
        ``QNetwork`` (or its weight tensor) that follows: target += tau *
        (weights - target), an exact copy with tau = 1."""
        self._bind(net)
        w = net.weights
        if (not torch.is_tensor(grad) or tuple(grad.shape) != (w.numel(),) or grad.dtype != torch.float32
                or grad.device != w.device or not grad.is_contiguous()):
            raise ValueError('grad must be a contiguous float32 [%d] tensor on %s' % (w.numel(), w.device))
        tw = None
        if target is not None:
            tw = target if torch.is_tensor(target) else target.weights
            if (tuple(tw.shape) != tuple(w.shape) or tw.dtype != torch.float32 or tw.device != w.device
                    or not tw.is_contiguous()):
                raise ValueError('target must be a QNetwork of the same shape on %s' % w.device)
        h = self.hyper(self.t + 1, tau)
        c = _lib.AstroQOpt(kind=h['kind'], nesterov=h['nesterov'], **{k: float(h[k]) for k in _F})
        lib = _lib.load_qopt()
        _lib.check_qopt(lib.astro_qopt_step(
            ctypes.byref(c), w.numel(), grad.data_ptr(), w.data_ptr(),
            self.state[0].data_ptr() if self.nstate > 0 else None,
            self.state[1].data_ptr() if self.nstate > 1 else None,
            None if tw is None else tw.data_ptr(), self.norm.data_ptr(), self.skipped.data_ptr(),
            _lib.stream_ptr(w.device)), 'astro_qopt_step')
        self.t += 1

    def reset(self):
        """Zero state, t = 0, skipped = 0 (the binding stays)."""
        self.t = 0
        if self.state is not None:
            self.state.zero_()
            self.norm.zero_()
            self.skipped.zero_()

    def state_dict(self):
        """{'kind', 't', 'hyper' (the constructor's arguments), 'state' (a copy
        of the state tensor, or None before the first apply), 'skipped'}."""
        return dict(kind=self.kind, t=self.t, hyper=dict(self._kw),
                    state=None if self.state is None else self.state.clone(),
                    skipped=None if self.skipped is None else self.skipped.clone())

    def load_state_dict(self, d):
        """Restore ``state_dict()``'s state and t (the hyperparameters stay
        this instance's).  The instance must be bound if the dict holds state."""
        if d['kind'] != self.kind:
            raise ValueError('state of %s, this is %s' % (d['kind'], self.kind))
        if d['state'] is not None:
            if self.state is None:
                raise ValueError('bind the optimizer first (one apply, or _bind(net))')
            self.state.copy_(d['state'])
            self.skipped.copy_(d['skipped'])
        elif self.state is not None:
            self.state.zero_()
            self.skipped.zero_()
        self.t = int(d['t'])


class SGD(Optimizer):
    """torch.optim.SGD(lr, momentum, nesterov=, weight_decay=) without
    dampening.  With momentum 0 there is no state.  Not bit for bit
    ``QNetwork.sgd_step``: torch's ``add_(alpha=)`` may fuse the multiply-add,
    this kernel rounds the product first."""
    kind = 'sgd'

    def __init__(self, lr, momentum=0.0, nesterov=False, weight_decay=0.0, max_norm=None):
        if nesterov and not momentum > 0:
            raise ValueError('nesterov needs a momentum')
        self.nstate = 1 if momentum != 0 else 0
        super().__init__(lr=lr, momentum=momentum, nesterov=nesterov, weight_decay=weight_decay, max_norm=max_norm)


class RMSprop(Optimizer):
    """torch.optim.RMSprop(lr, alpha, eps, weight_decay=), not centered, no
    momentum; the defaults are the reference's commented settings (rl.py:175)."""
    kind, nstate = 'rmsprop', 1

    def __init__(self, lr=1e-2, alpha=0.99, eps=1e-3, weight_decay=0.0, max_norm=None):
        super().__init__(lr=lr, alpha=alpha, eps=eps, weight_decay=weight_decay, max_norm=max_norm)


class Adagrad(Optimizer):
    """torch.optim.Adagrad(lr, eps=, weight_decay=) without lr_decay."""
    kind, nstate = 'adagrad', 1

    def __init__(self, lr=1e-2, eps=1e-10, weight_decay=0.0, max_norm=None):
        super().__init__(lr=lr, eps=eps, weight_decay=weight_decay, max_norm=max_norm)


class Adam(Optimizer):
    """torch.optim.Adam(lr, betas, eps, weight_decay=) (L2 decay, no amsgrad);
    the reference's first candidate at lr 1e-3 (rl.py:172)."""
    kind, nstate = 'adam', 2

    def __init__(self, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=None):
        super().__init__(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, max_norm=max_norm)
