"""The Q-network policy of astro/rl.py: ``ValueNetwork`` (rl.py:32-165) and
``QBot`` (rl.py:195-209), with the forward pass of a whole ``BatchedEnv``
fused into one HIP kernel (csrc/astro_qnet.hip, include/astro_qnet.h).

* ``ValueNetwork(solo, nout)`` is a torch module with the reference's
  parameter names (a reference ``state_dict`` loads unchanged).  Train it with
  torch autograd on ``BatchedEnv.features()``.
* ``QNetwork.from_module(module, device)`` packs its weights into the device
  buffer ``BatchedEnv.qvalues`` / ``qcontrols`` / ``rollout_q`` take: the
  kernel reads the env state directly, so acting needs no feature tensor.
* ``QNetwork.forward`` / ``qmax`` / ``td_targets`` / ``grad`` / ``sgd_step``
  train the packed buffer in place on the device (csrc/astro_qtrain.hip,
  include/astro_qtrain.h): rl.QNetworkTrainer.step without a torch module.
  ``step`` does the same with an ``astro_amd.optim`` rule, ``clone`` /
  ``copy_from`` make a target network, ``td_targets(online=)`` Double-DQN targets.
* ``forward64`` is the same forward pass in numpy float64 (the tests' truth),
  ``grad64`` its backward pass;
  ``QBot`` is the reference's evaluation bot for the single-game
  ``astro_amd.core.play``, on the host.
"""
import ctypes

import numpy as np
import torch

from . import _lib

HIDDEN = _lib.QNET_HIDDEN     # rl.py:140: nh, d = 32, 2
DEPTH = 2
# state_dict order = the order of AstroQNet.weights
LAYERS = ('f0', 'f.0', 'f.1', 'v.0', 'v.1', 'v0')


def nfeatures(solo):
    return 10 if solo else 15   # rl.py:139: type + 5 per ship + 4


def get_features(state):
    """rl.ValueNetwork.get_features (rl.py:43-72): float32 [planets + bullets,
    1 + 5 * ships + 4]; column 0 is 0 for a planet and 1 for a bullet, then
    every ship's (x, dx, norm_angle(b) / pi), then the object's (x, dx)."""
    sh, pl, bl = state.ships, state.planets, state.bullets
    npl, S = pl.x.shape[0], sh.x.shape[0]
    f = np.zeros((npl + bl.x.shape[0], 1 + 4 + 5 * S), dtype=np.float32)
    f[npl:, 0] = 1
    bearing = (((sh.b[:, np.newaxis] + np.pi) % (2 * np.pi)) - np.pi) / np.pi   # util.py:125-132
    f[:, 1:1 + 5 * S] = np.concatenate((sh.x, sh.dx, bearing), axis=1).flatten()
    f[:npl, 1 + 5 * S:] = np.concatenate((pl.x, pl.dx), axis=1)
    f[npl:, 1 + 5 * S:] = np.concatenate((bl.x, bl.dx), axis=1)
    return f


def swap_ego(features):
    """The other ship's ego view of two-ship features (array or tensor
    [..., 15]): the two ships' five columns exchanged (core.roll_ships)."""
    idx = list(range(0, 1)) + list(range(6, 11)) + list(range(1, 6)) + list(range(11, 15))
    return features[..., idx]


class ValueNetwork(torch.nn.Module):
    """rl.ValueNetwork (rl.py:137-155): f0 (nf -> 32), f.0, f.1 on every
    object row with softsign between, a max over the rows whose type column
    is >= 0 (to_batch pads with -1), v.0, v.1 with softsign after each, v0
    and tanh.  features: [..., rows, nf]; returns [..., nout]."""

    def __init__(self, solo, nout=6):
        super().__init__()
        nf, nh = nfeatures(solo), HIDDEN
        self.solo, self.nout = bool(solo), int(nout)
        self.f0 = torch.nn.Linear(nf, nh)
        self.f = torch.nn.ModuleList([torch.nn.Linear(nh, nh) for _ in range(DEPTH)])
        self.v = torch.nn.ModuleList([torch.nn.Linear(nh, nh) for _ in range(DEPTH)])
        self.v0 = torch.nn.Linear(nh, nout)

    @staticmethod
    def masked_max(x, features):
        pad = (features[..., 0] < 0)[..., None]
        return torch.max(torch.where(pad, x - 1e9, x), -2)[0]   # rl.py:126-128

    def forward(self, features):
        act = torch.nn.functional.softsign
        h = self.f0(features)
        for layer in self.f:
            h = layer(act(h))
        v = self.masked_max(h, features)
        for layer in self.v:
            v = act(layer(v))
        return torch.tanh(self.v0(v))

    def evaluate(self, state):
        """Q values of one State (the bot's ego view), float32 [nout]."""
        with torch.no_grad():
            p = next(self.parameters())
            x = torch.from_numpy(get_features(state)).to(device=p.device, dtype=p.dtype)
            return self(x)


def _arrays(weights):
    """state_dict / module / dict of arrays -> {name: float array}."""
    if isinstance(weights, torch.nn.Module):
        weights = weights.state_dict()
    return {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in weights.items()}


def shapes(nships, nout):
    """[(state_dict name, shape)] in the order of AstroQNet.weights."""
    nf, nh = 5 + 5 * nships, HIDDEN
    dims = [(nh, nf)] + [(nh, nh)] * (2 * DEPTH) + [(nout, nh)]
    out = []
    for name, (o, i) in zip(LAYERS, dims):
        out += [(name + '.weight', (o, i)), (name + '.bias', (o,))]
    return out


def pack(weights):
    """A module or state_dict as the flat float32 array AstroQNet.weights
    points to (state_dict order, torch's [out][in] rows)."""
    w = _arrays(weights)
    nout, nf = w['v0.weight'].shape[0], w['f0.weight'].shape[1]
    if nf not in (10, 15) or not 1 <= nout <= 6:
        raise ValueError('not a ValueNetwork: %d features, %d outputs' % (nf, nout))
    parts = []
    for name, shape in shapes((nf - 5) // 5, nout):
        a = w[name]
        if tuple(a.shape) != shape:
            raise ValueError('%s is %s, expected %s' % (name, tuple(a.shape), shape))
        parts.append(np.ascontiguousarray(a, dtype=np.float32).ravel())
    return np.concatenate(parts)


def unpack(flat, nships, nout=6):
    """The inverse of ``pack``: {state_dict name: float32 array}."""
    flat = np.asarray(flat, dtype=np.float32)
    out, k = {}, 0
    for name, shape in shapes(nships, nout):
        n = int(np.prod(shape))
        out[name] = flat[k:k + n].reshape(shape).copy()
        k += n
    if k != flat.size:
        raise ValueError('%d floats, expected %d' % (flat.size, k))
    return out


def forward64(weights, features):
    """ValueNetwork.forward in numpy float64.  features: [rows, nf] of one
    state or [B, rows, nf] with to_batch's -1 padding."""
    w = {k: v.astype(np.float64) for k, v in _arrays(weights).items()}
    x = np.asarray(features, dtype=np.float64)
    softsign = lambda a: a / (1.0 + np.abs(a))  # noqa: E731
    lin = lambda a, k: a @ w[k + '.weight'].T + w[k + '.bias']  # noqa: E731
    h = lin(x, 'f0')
    for k in ('f.0', 'f.1'):
        h = lin(softsign(h), k)
    v = np.where((x[..., 0] < 0)[..., None], -np.inf, h).max(-2)
    for k in ('v.0', 'v.1'):
        v = softsign(lin(v, k))
    return np.tanh(lin(v, 'v0'))


def grad64(weights, features, action, target):
    """rl.QNetworkTrainer.step's loss and gradient (rl.py:184-188) in numpy
    float64: y = Q(features)[action], loss = (target - y)^2, L = mean(loss).
    features [n, rows, nf] with to_batch's padding (column 0 < 0, anywhere
    among the rows; a padding row's other columns are ignored).  The pool's
    gradient goes to the first maximal live row (np.argmax).  A sample whose
    action is outside [0, nout) has loss NaN and adds nothing, but counts in
    the mean.  Returns (loss [n], {state_dict name: dL/dw})."""
    w = {k: v.astype(np.float64) for k, v in _arrays(weights).items()}
    x = np.asarray(features, dtype=np.float64)
    n, nout = x.shape[0], w['v0.weight'].shape[0]
    live = ~(x[..., 0] < 0)
    x = np.where(live[..., None], x, 0.0)
    action = np.asarray(action).astype(np.int64).reshape(n)
    target = np.asarray(target, dtype=np.float64).reshape(n)

    def fwd(a, k):   # softsign(linear): (value, reciprocal of 1 + |z|)
        z = a @ w[k + '.weight'].T + w[k + '.bias']
        r = 1.0 / (1.0 + np.abs(z))
        return z * r, r

    a0, r0 = fwd(x, 'f0')
    a1, r1 = fwd(a0, 'f.0')
    z2 = a1 @ w['f.1.weight'].T + w['f.1.bias']
    arg = np.where(live[..., None], z2, -np.inf).argmax(1)            # [n, 32]: the first maximal live row
    p = np.take_along_axis(z2, arg[:, None, :], 1)[:, 0, :]
    av0, rv0 = fwd(p, 'v.0')
    av1, rv1 = fwd(av0, 'v.1')
    q = np.tanh(av1 @ w['v0.weight'].T + w['v0.bias'])
    ok = (action >= 0) & (action < nout)
    a = np.where(ok, action, 0)
    y = q[np.arange(n), a]
    loss = np.where(ok, (target - y) ** 2, np.nan)

    g = {}

    def bwd(k, dz, inp):   # a linear layer's parameter gradients; returns the input's gradient
        g[k + '.weight'] = dz.reshape(-1, dz.shape[-1]).T @ inp.reshape(-1, inp.shape[-1])
        g[k + '.bias'] = dz.reshape(-1, dz.shape[-1]).sum(0)
        return dz @ w[k + '.weight']

    dz = np.zeros((n, nout))
    dz[np.arange(n), a] = np.where(ok, 2.0 * (y - target) / max(n, 1) * (1.0 - y * y), 0.0)
    dz = bwd('v0', dz, av1) * rv1 ** 2
    dz = bwd('v.1', dz, av0) * rv0 ** 2
    dp = bwd('v.0', dz, p)
    dz = np.zeros_like(z2)
    np.put_along_axis(dz, arg[:, None, :], dp[:, None, :], 1)
    dz = bwd('f.1', dz, a1) * r1 ** 2
    dz = bwd('f.0', dz, a0) * r0 ** 2
    bwd('f0', dz, x)
    return loss, {k: g[k] for k, _ in shapes((x.shape[-1] - 5) // 5, nout)}


def _td_targets(reward, discount, qmax, terminal):
    """rl.QBotTrainer._step's targets (rl.py:281-291) from max_a Q(new_state_f)."""
    return torch.where(terminal.to(torch.bool), reward, discount * qmax)


class QNetwork:
    """A ValueNetwork's weights packed on a device, as astro_qvalues reads
    them (``BatchedEnv.qvalues(net)``).  ``sgd_step`` trains the buffer in
    place, so the acting kernel sees the new weights at once; ``update``
    copies a torch module's weights in.  ``grad`` and ``sgd_step`` share one
    cached workspace per QNetwork: issue them on one stream (or order the
    streams yourself); calls on two streams at once would race on it."""

    def __init__(self, flat, nships, nout, device):
        flat = np.ascontiguousarray(flat, dtype=np.float32)
        if flat.size != sum(int(np.prod(s)) for _, s in shapes(nships, nout)):
            raise ValueError('packed weights do not fit nships %d, nout %d' % (nships, nout))
        self.nships, self.nout = int(nships), int(nout)
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise ValueError('QNetwork lives on a HIP device (got %s)' % self.device)
        self.weights = torch.from_numpy(flat).to(self.device)
        self.c = _lib.AstroQNet(weights=self.weights.data_ptr(), nships=self.nships, nout=self.nout)
        self._workspace = None    # astro_qgrad's scratch, grown when needed

    @classmethod
    def from_module(cls, module, device='cuda'):
        w = _arrays(module)
        return cls(pack(w), (w['f0.weight'].shape[1] - 5) // 5, w['v0.weight'].shape[0], device)

    @classmethod
    def from_npz(cls, path, device='cuda', prefix=''):
        """From an .npz of state_dict arrays (names optionally prefixed)."""
        z = np.load(path, allow_pickle=False) if isinstance(path, str) else path
        names = [n for n, _ in shapes(2, 1)]
        return cls.from_module({n: z[prefix + n] for n in names}, device)

    def update(self, module):
        """Copy a module's current weights into the device buffer (same shapes)."""
        self.weights.copy_(torch.from_numpy(pack(module)))

    def byref(self):
        return ctypes.byref(self.c)

    def state_dict(self):
        """{state_dict name: view into the flat device buffer}: what
        ``module.load_state_dict`` takes to write the network back into a
        torch or reference module."""
        out, k = {}, 0
        for name, shape in shapes(self.nships, self.nout):
            size = int(np.prod(shape))
            out[name] = self.weights[k:k + size].view(shape)
            k += size
        return out

    # ------------------------------------------------ training (astro_qtrain.h)

    def _features(self, features):
        nf = 5 + 5 * self.nships
        if (not torch.is_tensor(features) or features.dim() != 3 or features.shape[2] != nf
                or features.shape[1] < 1 or features.dtype != torch.float32
                or features.device != self.weights.device or not features.is_contiguous()):
            raise ValueError('features must be a contiguous float32 [n, rows, %d] tensor on %s'
                             % (nf, self.weights.device))
        return int(features.shape[0]), int(features.shape[1])

    def _out(self, out, shape, what):
        if out is None:
            return torch.empty(shape, dtype=torch.float32, device=self.weights.device)
        if (not torch.is_tensor(out) or tuple(out.shape) != tuple(shape) or out.dtype != torch.float32
                or out.device != self.weights.device or not out.is_contiguous()):
            raise ValueError('%s must be a contiguous float32 %s tensor on %s'
                             % (what, list(shape), self.weights.device))
        return out

    def _vector(self, v, n, what):
        """An [n] input on the device, of any stride (the callers convert, which also packs it)."""
        if not torch.is_tensor(v) or tuple(v.shape) != (n,) or v.device != self.weights.device:
            raise ValueError('%s must be a [%d] tensor on %s' % (what, n, self.weights.device))
        return v

    def _qforward(self, features, q, qmax):
        n, rows = self._features(features)
        if n == 0:      # (an empty tensor has no address)
            return
        lib = _lib.load_qtrain()
        stream = _lib.stream_ptr(self.weights.device)
        _lib.check_qtrain(lib.astro_qforward(self.byref(), features.data_ptr(), n, rows,
                                             None if q is None else q.data_ptr(),
                                             None if qmax is None else qmax.data_ptr(), stream), 'astro_qforward')

    def forward(self, features, out=None):
        """rl.ValueNetwork.forward on a to_batch feature tensor
        (``BatchedEnv.features()``): float32 [n, nout]."""
        n, _ = self._features(features)
        q = self._out(out, (n, self.nout), 'out')
        self._qforward(features, q, None)
        return q

    def qmax(self, features, out=None):
        """The maximum of ``forward(features)`` over the outputs: float32 [n]."""
        n, _ = self._features(features)
        m = self._out(out, (n,), 'out')
        self._qforward(features, None, m)
        return m

    def td_targets(self, reward, discount, next_features, terminal, online=None):
        """rl.QBotTrainer._step's targets (rl.py:281-291): ``reward`` where
        ``terminal``, ``discount * max_a Q(next_features)`` elsewhere (a
        terminal sample's next_features may hold anything).  reward, terminal:
        [n] tensors on the device; discount: a number or an [n] tensor.

        online: another ``QNetwork`` of the same shape -- Double-DQN targets:
        this network's value of the action the online network prefers,
        ``discount * Q_self(next)[argmax_a Q_online(next)]``, the first maximal
        output as ``np.argmax`` takes it (two ``forward`` calls and a few
        elementwise launches on [n, nout] values)."""
        n, _ = self._features(next_features)
        reward = self._vector(reward, n, 'reward').to(torch.float32)
        terminal = self._vector(terminal, n, 'terminal')
        if online is None:
            return _td_targets(reward, discount, self.qmax(next_features), terminal)
        if (online.nships, online.nout) != (self.nships, self.nout):
            raise ValueError('the online network has another shape')
        qo = online.forward(next_features)
        # np.argmax: the first index that attains the maximum, the first NaN if there is one
        best = (qo == qo.max(1, keepdim=True).values) | qo.isnan()
        index = torch.arange(self.nout, device=qo.device).expand_as(qo)
        first = torch.where(best, index, self.nout - 1).min(1, keepdim=True).values
        return _td_targets(reward, discount, self.forward(next_features).gather(1, first)[:, 0], terminal)

    def grad(self, features, action, target, loss_out=None, grad_out=None):
        """rl.QNetworkTrainer.step's loss and gradient (rl.py:184-188): y =
        Q(features)[action], loss = (target - y)^2, L = mean(loss).  action:
        an integer [n] tensor, target: float32 [n].  Returns (loss [n], dL/dw
        [nparams] in the layout of ``weights``); deterministic bit for bit.
        Stream-ordered on the current stream; see the class on the shared
        workspace."""
        n, rows = self._features(features)
        action = self._vector(action, n, 'action')
        if action.dtype.is_floating_point or action.dtype == torch.bool:
            raise ValueError('action must be an integer tensor')
        if action.dtype != torch.int8:
            # widened first (an unsigned dtype cannot hold the -1 bound), then clamped so that a
            # value outside int8 stays out of range instead of wrapping into it
            action = action.to(torch.int64).clamp(-1, 127).to(torch.int8)
        action = action.contiguous()
        target = self._vector(target, n, 'target')
        if target.dtype != torch.float32:
            raise ValueError('target must be a float32 tensor')
        target = target.contiguous()
        loss = self._out(loss_out, (n,), 'loss_out')
        grad = self._out(grad_out, (self.weights.numel(),), 'grad_out')
        lib = _lib.load_qtrain()
        need = int(lib.astro_qgrad_workspace_bytes(self.byref(), n))
        ws = self._workspace
        if ws is None or ws.numel() * 4 < need:
            ws = self._workspace = torch.empty(max(1, (need + 3) // 4), dtype=torch.float32,
                                               device=self.weights.device)
        stream = _lib.stream_ptr(self.weights.device)
        _lib.check_qtrain(lib.astro_qgrad(self.byref(), features.data_ptr(), n, rows, action.data_ptr(),
                                          target.data_ptr(), loss.data_ptr(), grad.data_ptr(), ws.data_ptr(),
                                          ws.numel() * 4, stream), 'astro_qgrad')
        return loss, grad

    def sgd_step(self, features, action, target, lr=1e-2):
        """rl.QNetworkTrainer.step (rl.py:176-192, SGD with lr 1e-2) on the
        packed buffer, in place.  Returns the per-sample loss [n]."""
        loss, grad = self.grad(features, action, target)
        self.weights.add_(grad, alpha=-lr)
        return loss

    def step(self, features, action, target, opt, target_net=None, tau=1.0):
        """``grad`` then ``opt.apply(self, grad, target_net, tau)``: one
        optimisation step with an ``astro_amd.optim`` rule on the packed buffer,
        in place.  target_net: a ``clone()`` that follows the new weights
        (``optim.Optimizer.apply``).  Returns the per-sample loss [n].
        ``step`` with ``optim.SGD(lr)`` and ``sgd_step`` need not agree bit for
        bit: torch's ``add_(alpha=)`` may fuse the multiply-add, the optimiser
        kernel never does."""
        loss, grad = self.grad(features, action, target)
        opt.apply(self, grad, target_net, tau)
        return loss

    def clone(self):
        """A new QNetwork with storage of its own and equal weights (a target
        network), copied on the device."""
        other = QNetwork.__new__(QNetwork)
        other.nships, other.nout, other.device = self.nships, self.nout, self.device
        other.weights = self.weights.clone()
        other.c = _lib.AstroQNet(weights=other.weights.data_ptr(), nships=other.nships, nout=other.nout)
        other._workspace = None
        return other

    @classmethod
    def view(cls, row, nships, nout):
        """A QNetwork whose ``weights`` IS ``row`` (a contiguous float32
        [nparams] device tensor, e.g. a row of a population's member matrix):
        made like ``clone()`` without the copy, so whatever writes the row
        changes what this network plays."""
        n = sum(int(np.prod(s)) for _, s in shapes(nships, nout))
        if (not torch.is_tensor(row) or tuple(row.shape) != (n,) or row.dtype != torch.float32
                or row.device.type != 'cuda' or not row.is_contiguous()):
            raise ValueError('row must be a contiguous float32 [%d] tensor on a HIP device' % n)
        other = cls.__new__(cls)
        other.nships, other.nout, other.device = int(nships), int(nout), row.device
        other.weights = row
        other.c = _lib.AstroQNet(weights=row.data_ptr(), nships=other.nships, nout=other.nout)
        other._workspace = None
        return other

    def copy_from(self, other):
        """Copy another QNetwork's weights in, on the device (no host trip)."""
        if (other.nships, other.nout) != (self.nships, self.nout):
            raise ValueError('the other network has another shape')
        self.weights.copy_(other.weights)
        return self


class QBot:
    """rl.QBot (rl.py:195-209): the greedy evaluation bot for the single-game
    ``astro_amd.core.play`` -- argmax of the network's Q values on the ego
    view it is called with, the values kept in ``data``.  Host side."""

    def __init__(self, network):
        self.q = network
        self._last_q = None

    def __call__(self, state):
        self._last_q = self.q.evaluate(state).cpu().numpy()
        return np.argmax(self._last_q)

    def reward(self, state, reward):
        pass

    @property
    def data(self):
        return dict(q=self._last_q)
