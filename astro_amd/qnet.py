"""The Q-network policy of astro/rl.py: ``ValueNetwork`` (rl.py:32-165) and
``QBot`` (rl.py:195-209), with the forward pass of a whole ``BatchedEnv``
fused into one HIP kernel (csrc/astro_qnet.hip, include/astro_qnet.h).

* ``ValueNetwork(solo, nout)`` is a torch module with the reference's
  parameter names (a reference ``state_dict`` loads unchanged).  Train it with
  torch autograd on ``BatchedEnv.features()``.
* ``QNetwork.from_module(module, device)`` packs its weights into the device
  buffer ``BatchedEnv.qvalues`` / ``qcontrols`` / ``rollout_q`` take: the
  kernel reads the env state directly, so acting needs no feature tensor.
* ``forward64`` is the same forward pass in numpy float64 (the tests' truth);
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


class QNetwork:
    """A ValueNetwork's weights packed on a device, as astro_qvalues reads
    them (``BatchedEnv.qvalues(net)``).  A snapshot: pack again after training."""

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
