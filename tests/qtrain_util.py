"""Shared by tests/test_qtrain_host.py and tests/test_gpu_qtrain.py: feature
batches with designed live-row counts and no near-tie in the max pool, and
the float64 / torch float32 references of astro_qforward and astro_qgrad
with the tolerances derived from them."""
import numpy as np

from tests import qnet_util as qu

GAP = 1e-5          # smallest float64 top-2 gap of the pool a sample may have
MAX_DROPPED = 0.01  # share of generated samples the gap rule may drop


def weights_of(kind, nout=6, factor=1.0):
    """The fixture's network (torch-default weights x3) with the first
    ``nout`` rows of v0, times ``factor``."""
    fx, _, _ = qu.fixture()
    w = {k: np.array(v, dtype=np.float32) for k, v in fx[kind]['weights'].items()}
    w['v0.weight'], w['v0.bias'] = w['v0.weight'][:nout].copy(), w['v0.bias'][:nout].copy()
    return qu.scaled(w, factor) if factor != 1.0 else w


def nf_of(kind):
    return 10 if kind == 'solo' else 15


def raw_batch(kind, counts, rows, rng, holes=False):
    """float32 [len(counts), rows, nf]: counts[i] live rows (type 0 or 1,
    the rest uniform in [-1.2, 1.2]) and -1 padding after them, as to_batch
    writes it.  holes: every sample with room gets one padding row BETWEEN
    its live rows, and every padding row holds NaN outside column 0."""
    counts = np.asarray(counts, dtype=np.int64)
    n, nf = counts.size, nf_of(kind)
    assert counts.min() >= 1 and counts.max() + (1 if holes else 0) <= rows
    x = rng.uniform(-1.2, 1.2, size=(n, rows, nf)).astype(np.float32)
    x[:, :, 0] = rng.randint(0, 2, size=(n, rows))
    live = np.arange(rows)[None, :] < counts[:, None]
    if holes:
        at = np.where(counts > 1, rng.randint(1, np.maximum(counts, 2)), rows)   # the hole's row (none: one live row)
        live = np.arange(rows)[None, :] < (counts + (counts > 1))[:, None]
        live &= np.arange(rows)[None, :] != at[:, None]
        assert (live.sum(1) == counts).all()
    x[~live] = np.nan if holes else -1.0
    x[~live, 0] = -1.0
    return x


def pool_gap(weights, x):
    """The smallest float64 top-2 gap, over the 32 pooled units, of f.1's
    output among each sample's live rows: [n], inf for one live row."""
    w = {k: np.asarray(v, dtype=np.float64) for k, v in weights.items()}
    x = np.asarray(x, dtype=np.float64)
    live = ~(x[..., 0] < 0)
    h = np.where(live[..., None], x, 0.0) @ w['f0.weight'].T + w['f0.bias']
    for k in ('f.0', 'f.1'):
        h = (h / (1.0 + np.abs(h))) @ w[k + '.weight'].T + w[k + '.bias']
    h = np.sort(np.where(live[..., None], h, -np.inf), axis=1)
    if h.shape[1] < 2:
        return np.full(h.shape[0], np.inf)
    gap = h[:, -1, :] - h[:, -2, :]          # inf where the second is -inf
    return np.where(np.isnan(gap), np.inf, gap).min(-1)


def batch(kind, weights, counts, rows, rng, n=None, holes=False, block=8192):
    """raw_batch without the samples whose pool has a near tie (gap < GAP in
    float64), before any implementation sees it; at most MAX_DROPPED of the
    generated samples may go (asserted).  n: keep the first n of what is left.
    Returns (features, counts of the kept samples)."""
    x = raw_batch(kind, counts, rows, rng, holes)
    gap = np.concatenate([pool_gap(weights, x[a:a + block]) for a in range(0, x.shape[0], block)])
    keep = gap >= GAP
    dropped = int((~keep).sum())
    assert dropped <= MAX_DROPPED * x.shape[0], (dropped, x.shape[0])
    x, counts = x[keep], np.asarray(counts)[keep]
    if n is not None:
        assert x.shape[0] >= n, (x.shape[0], n)
        x, counts = x[:n], counts[:n]
    return np.ascontiguousarray(x), counts


def torch_module(weights, dtype):
    import torch
    from astro_amd import qnet
    w = {k: np.asarray(v) for k, v in weights.items()}
    m = qnet.ValueNetwork(w['f0.weight'].shape[1] == 10, w['v0.weight'].shape[0]).to(dtype)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in w.items()})
    return m


def torch_grad(weights, x, action, target, dtype, block=8192):
    """torch CPU autograd of rl.QNetworkTrainer.step's loss (rl.py:184-188) in
    ``dtype``: (q [n, nout], loss [n], {name: grad}).  Samples with an action
    outside [0, nout) are left out of the sum but counted in the mean, their
    loss is NaN.  Padding rows' columns other than column 0 are zeroed first
    (torch would multiply their NaN by 0)."""
    import torch
    m = torch_module(weights, dtype)
    x = np.asarray(x)
    x = np.where((x[..., :1] < 0) & (np.arange(x.shape[-1]) > 0), 0.0, x).astype(np.float32)
    n, nout = x.shape[0], m.nout
    action = np.asarray(action).astype(np.int64)
    ok = (action >= 0) & (action < nout)
    qs, losses = [], []
    for a in range(0, n, block):
        xb = torch.from_numpy(x[a:a + block]).to(dtype)
        q = m(xb)
        okb = torch.from_numpy(ok[a:a + block])
        ab = torch.from_numpy(np.where(ok, action, 0)[a:a + block])
        y = q.gather(1, ab.view(-1, 1)).view(-1)
        loss = (torch.from_numpy(np.asarray(target)[a:a + block]).to(dtype) - y) ** 2
        if n <= block and ok.all():
            loss.mean().backward()     # the trainer's own expression
        else:
            (loss[okb].sum() / n).backward()
        qs.append(q.detach().numpy())
        losses.append(torch.where(okb, loss.detach(), torch.full_like(loss, float('nan'))).numpy())
    g = {k: (p.grad.numpy() if p.grad is not None else np.zeros(tuple(p.shape))) for k, p in m.named_parameters()}
    return np.concatenate(qs), np.concatenate(losses), g


def grad64(weights, x, action, target, block=8192):
    """qnet.grad64 in blocks of samples (each block's mean rescaled to the batch's)."""
    from astro_amd import qnet
    n = np.asarray(x).shape[0]
    losses, total = [], None
    for a in range(0, n, block):
        loss, g = qnet.grad64(weights, x[a:a + block], action[a:a + block], target[a:a + block])
        losses.append(loss)
        scale = loss.shape[0] / n
        total = {k: v * scale for k, v in g.items()} if total is None else {k: total[k] + v * scale for k, v in g.items()}
    return np.concatenate(losses), total


class Reference:
    """The float64 truth of one batch and the tolerances the float32 torch
    path sets: forward tol = 4 max |q32 - q64|; per parameter tensor tol = 4
    max(max |g32 - g64|, 2^-24 max |g64|); loss tol = 4 max |loss32 - loss64|."""

    def __init__(self, weights, x, action, target):
        from astro_amd import qnet
        self.nships = (np.asarray(x).shape[-1] - 5) // 5
        self.nout = np.asarray(weights['v0.weight']).shape[0]
        self.loss64, self.g64 = grad64(weights, x, action, target)
        q32, loss32, g32 = torch_grad(weights, x, action, target, __import__('torch').float32)
        xz = np.where((np.asarray(x)[..., :1] < 0) & (np.arange(np.asarray(x).shape[-1]) > 0), 0.0, x)
        self.q64 = np.concatenate([qnet.forward64(weights, xz[a:a + 8192]) for a in range(0, xz.shape[0], 8192)])
        self.q_tol = 4.0 * float(np.abs(q32.astype(np.float64) - self.q64).max())
        ok = ~np.isnan(self.loss64)
        assert np.array_equal(np.isnan(loss32), ~ok)
        self.loss_tol = 4.0 * float(np.abs(loss32[ok].astype(np.float64) - self.loss64[ok]).max()) if ok.any() else 0.0
        self.g_tol = {k: 4.0 * max(float(np.abs(g32[k].astype(np.float64) - self.g64[k]).max()),
                                   2.0 ** -24 * float(np.abs(self.g64[k]).max())) for k in self.g64}

    def check_q(self, q):
        err = float(np.abs(np.asarray(q, dtype=np.float64) - self.q64).max())
        assert err <= self.q_tol, ('q', err, self.q_tol)
        return err / self.q_tol

    def check_loss(self, loss):
        loss = np.asarray(loss, dtype=np.float64)
        ok = ~np.isnan(self.loss64)
        assert np.array_equal(np.isnan(loss), ~ok), 'loss is NaN exactly where the action is out of range'
        if not ok.any():
            return 0.0
        err = float(np.abs(loss[ok] - self.loss64[ok]).max())
        assert err <= self.loss_tol, ('loss', err, self.loss_tol)
        return err / self.loss_tol

    def check_grad(self, flat):
        """flat: the packed gradient.  Returns the worst error / tol over the tensors."""
        from astro_amd import qnet
        g = qnet.unpack(np.asarray(flat), self.nships, self.nout)
        worst = 0.0
        bad = []
        for k, want in self.g64.items():
            assert np.isfinite(g[k]).all(), k
            r = float(np.abs(g[k].astype(np.float64) - want).max()) / self.g_tol[k] if self.g_tol[k] > 0 else 0.0
            if self.g_tol[k] == 0:
                assert not g[k].any(), k
            worst = max(worst, r)
            if r > 1.0:
                bad.append((k, r))
        assert not bad, ('error / tol per tensor', bad)
        return worst
