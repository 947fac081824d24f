"""astro_qforward / astro_qgrad on the device (include/astro_qtrain.h) against
qnet.grad64 and qnet.forward64, with the tolerances torch's float32 CPU
autograd sets on the same batch (tests/qtrain_util.py: Reference).

Every output buffer holds NaN before the call, loss and grad are followed by
64 guard elements, and the workspace is NaN on entry."""
import numpy as np
import pytest
import torch

from astro_amd import BatchedEnv, _lib, qnet
from astro_amd.config import DEFAULT_CONFIG
from tests import qtrain_util as qt

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARD = 64
SENTINEL = 12345.0
# the live-row counts every layout cycles through: tile edges (16, 17, 32, 33) and a sample of three tiles
COUNTS = (1, 2, 16, 17, 32, 33, 70)
ROWS = 72


def _net(w):
    return qnet.QNetwork.from_module(w, DEV)


def _guarded(n):
    buf = torch.full((n + GUARD,), float('nan'), dtype=torch.float32, device=DEV)
    buf[n:] = SENTINEL
    return buf


def _nan_workspace(net, n):
    need = int(_lib.load_qtrain().astro_qgrad_workspace_bytes(net.byref(), n))
    net._workspace = torch.full((max(1, need // 4),), float('nan'), dtype=torch.float32, device=DEV)
    return net._workspace


def _grad(net, x, action, target):
    """net.grad into NaN-filled guarded buffers with a NaN workspace: (loss, grad) as numpy."""
    n = x.shape[0]
    lbuf, gbuf = _guarded(n), _guarded(net.weights.numel())
    ws = _nan_workspace(net, n)
    loss, grad = net.grad(torch.as_tensor(x, device=DEV), torch.as_tensor(action, device=DEV),
                          torch.as_tensor(target, device=DEV), loss_out=lbuf[:n], grad_out=gbuf[:-GUARD])
    torch.cuda.synchronize()
    assert net._workspace is ws
    assert (lbuf[n:] == SENTINEL).all() and (gbuf[-GUARD:] == SENTINEL).all(), 'a guard element changed'
    return loss.cpu().numpy(), grad.cpu().numpy()


def _counts(n, rng):
    """70 rows first in the chunk, then one-row samples, then the cycle and random counts."""
    c = [70, 1, 1, 1, 1, 1] + [COUNTS[i % len(COUNTS)] for i in range(n)]
    c = np.array(c[:n] if n < 64 else c[:64] + list(rng.randint(1, 71, size=n - 64)))
    return c


@pytest.fixture(scope='module')
def pools():
    """Per kind: 517 samples (of 523 generated, near-ties dropped) with their
    actions, targets and weights; the references of their prefixes are cached."""
    out = {}
    for kind in ('duo', 'solo'):
        rng = np.random.RandomState(11 if kind == 'duo' else 12)
        w = qt.weights_of(kind)
        x, counts = qt.batch(kind, w, _counts(523, rng), ROWS, rng, n=517)
        assert counts[0] == 70 and (counts[1:6] == 1).all() and set(COUNTS) <= set(counts[:33].tolist())
        assert x.shape[1] > counts.max()
        out[kind] = dict(w=w, x=x, counts=counts, action=rng.randint(0, 6, size=517),
                         target=rng.uniform(-1, 1, size=517).astype(np.float32), refs={})
    return out


def _ref(pool, n):
    if n not in pool['refs']:
        pool['refs'][n] = qt.Reference(pool['w'], pool['x'][:n], pool['action'][:n], pool['target'][:n])
    return pool['refs'][n]


# ---------------------------------------------------------------------------
# 1. tile and segment edges

@pytest.mark.parametrize('kind', ['duo', 'solo'])
@pytest.mark.parametrize('n', [1, 31, 32, 33, 517])
def test_tile_and_segment_edges(pools, kind, n):
    p = pools[kind]
    ref = _ref(p, n)
    net = _net(p['w'])
    x = torch.as_tensor(p['x'][:n], device=DEV)
    qbuf, mbuf = _guarded(n * 6), _guarded(n)
    q = net.forward(x, out=qbuf[:n * 6].view(n, 6))
    m = net.qmax(x, out=mbuf[:n])
    torch.cuda.synchronize()
    assert (qbuf[n * 6:] == SENTINEL).all() and (mbuf[n:] == SENTINEL).all()
    rq = ref.check_q(q.cpu().numpy())
    assert torch.equal(m, q.max(1)[0])
    loss, grad = _grad(net, p['x'][:n], p['action'][:n], p['target'][:n])
    rl, rg = ref.check_loss(loss), ref.check_grad(grad)
    print('%s n %d: error / tol: q %.3f, loss %.3f, grad %.3f' % (kind, n, rq, rl, rg))


# ---------------------------------------------------------------------------
# 2. every nout, every action, out-of-range actions

@pytest.mark.parametrize('kind', ['duo', 'solo'])
@pytest.mark.parametrize('nout', [1, 2, 3, 4, 5, 6])
def test_every_nout_and_action(pools, kind, nout):
    p = pools[kind]
    n = 70
    w = qt.weights_of(kind, nout)
    action = np.arange(n) % nout
    action[7], action[40] = -1, nout
    ref = qt.Reference(w, p['x'][:n], action, p['target'][:n])
    assert np.isnan(ref.loss64[[7, 40]]).all() and np.isnan(ref.loss64).sum() == 2
    net = _net(w)
    loss, grad = _grad(net, p['x'][:n], action, p['target'][:n])
    rl, rg = ref.check_loss(loss), ref.check_grad(grad)
    q = net.forward(torch.as_tensor(p['x'][:n], device=DEV))
    assert tuple(q.shape) == (n, nout)
    rq = ref.check_q(q.cpu().numpy())
    # the two samples are out of the sum but in the mean: the same batch without them is 70 / 68 times this
    keep = np.ones(n, bool)
    keep[[7, 40]] = False
    _, g68 = qnet.grad64(w, p['x'][:n][keep], action[keep], p['target'][:n][keep])
    for k in g68:
        assert np.abs(g68[k] * 68 / 70 - ref.g64[k]).max() <= 1e-12 * np.abs(ref.g64[k]).max()
    # int64 actions are converted on the device
    loss2, grad2 = net.grad(torch.as_tensor(p['x'][:n], device=DEV), torch.as_tensor(action, device=DEV).long(),
                            torch.as_tensor(p['target'][:n], device=DEV))
    assert np.array_equal(grad2.cpu().numpy(), grad) and np.array_equal(loss2.cpu().numpy(), loss, equal_nan=True)
    # uint8 actions (it cannot hold -1: 200 is the out-of-range value), strided, with a strided target
    a8 = np.where(action < 0, 200, action).astype(np.uint8)
    wide = torch.zeros((n, 2), dtype=torch.uint8, device=DEV)
    wide[:, 0] = torch.as_tensor(a8, device=DEV)
    twide = torch.zeros((n, 3), device=DEV)
    twide[:, 1] = torch.as_tensor(p['target'][:n], device=DEV)
    assert wide[:, 0].dtype == torch.uint8 and not wide[:, 0].is_contiguous() and not twide[:, 1].is_contiguous()
    loss3, grad3 = net.grad(torch.as_tensor(p['x'][:n], device=DEV), wide[:, 0], twide[:, 1])
    assert np.array_equal(grad3.cpu().numpy(), grad) and np.array_equal(loss3.cpu().numpy(), loss, equal_nan=True)
    for dt in (torch.int16, torch.int32):
        loss4, grad4 = net.grad(torch.as_tensor(p['x'][:n], device=DEV), torch.as_tensor(action, device=DEV).to(dt),
                                torch.as_tensor(p['target'][:n], device=DEV))
        assert np.array_equal(grad4.cpu().numpy(), grad) and np.array_equal(loss4.cpu().numpy(), loss, equal_nan=True)
    print('%s nout %d: error / tol: q %.3f, loss %.3f, grad %.3f' % (kind, nout, rq, rl, rg))


# ---------------------------------------------------------------------------
# 3. the mask is column 0, anywhere

@pytest.mark.parametrize('kind', ['duo', 'solo'])
def test_padding_between_live_rows(kind):
    rng = np.random.RandomState(21)
    w = qt.weights_of(kind)
    x, counts = qt.batch(kind, w, _counts(101, rng), ROWS, rng, n=100, holes=True)
    live = ~(x[..., 0] < 0)
    # a padding row between live rows, NaN in every padding row's other columns
    assert ((live[:, 2:] & ~live[:, 1:-1]).any(1) | (counts == 1)).all() and np.isnan(x[~live][:, 1:]).all()
    assert not np.isnan(x[live]).any() and (live.sum(1) == counts).all()
    action, target = rng.randint(0, 6, size=100), rng.uniform(-1, 1, size=100).astype(np.float32)
    ref = qt.Reference(w, x, action, target)
    net = _net(w)
    q = net.forward(torch.as_tensor(x, device=DEV)).cpu().numpy()
    loss, grad = _grad(net, x, action, target)
    assert not np.isnan(q).any() and not np.isnan(loss).any() and not np.isnan(grad).any()
    print('%s holes: error / tol: q %.3f, loss %.3f, grad %.3f'
          % (kind, ref.check_q(q), ref.check_loss(loss), ref.check_grad(grad)))


# ---------------------------------------------------------------------------
# 4. ties go to the first live row

@pytest.mark.parametrize('kind', ['duo', 'solo'])
def test_ties_go_to_the_first_live_row(pools, kind):
    """Row o of f.1.weight zeroed: all live rows tie for unit o.  With the
    live rows of every sample in reverse order, grad64 changes in
    f.1.weight[o] alone (the other units' maxima are unique); the device
    agrees with the order it was given."""
    p = pools[kind]
    n, o = 100, 11
    w = qt.weights_of(kind)
    w['f.1.weight'][o] = 0.0
    x = p['x'][:n].copy()
    x[0, 0, 0] = -1.0     # a padding row first: sample 0's first live row is row 1
    assert qt.pool_gap(p['w'], x).min() >= qt.GAP
    ref = qt.Reference(w, x, p['action'][:n], p['target'][:n])
    rev = x.copy()
    for i in range(n):
        live = np.nonzero(~(x[i, :, 0] < 0))[0]
        rev[i, live] = x[i, live[::-1]]
    _, grev = qnet.grad64(w, rev, p['action'][:n], p['target'][:n])
    d = np.abs(grev['f.1.weight'][o] - ref.g64['f.1.weight'][o]).max()
    assert d > 1e-3 * np.abs(ref.g64['f.1.weight']).max()
    loss, grad = _grad(_net(w), x, p['action'][:n], p['target'][:n])
    rg = ref.check_grad(grad)
    g = qnet.unpack(grad, 1 if kind == 'solo' else 2, 6)
    e = np.abs(g['f.1.weight'][o] - ref.g64['f.1.weight'][o]).max()
    assert e <= 1e-3 * d, (e, d)
    print('%s ties: grad error / tol %.3f; row %d: %.3g from the first row, %.3g first to last' % (kind, rg, o, e, d))


# ---------------------------------------------------------------------------
# 5. a wave's second and third chunk

def test_second_and_third_chunk_of_a_wave():
    """65,589 samples are 2,050 chunks of 32: the grid's 256 x 4 waves take a
    second chunk each and the first two a third; the last chunk has 21."""
    n, rows = 65589, 4
    rng = np.random.RandomState(31)
    w = qt.weights_of('duo')
    x, counts = qt.batch('duo', w, rng.randint(1, 4, size=n + 300), rows, rng, n=n)
    action, target = rng.randint(0, 6, size=n), rng.uniform(-1, 1, size=n).astype(np.float32)
    ref = qt.Reference(w, x, action, target)
    net = _net(w)
    ws_bytes = int(_lib.load_qtrain().astro_qgrad_workspace_bytes(net.byref(), n))
    assert ws_bytes == 256 * 4 * net.weights.numel() * 4 and (n + 31) // 32 == 2 * 1024 + 2 and n % 32 == 21
    loss, grad = _grad(net, x, action, target)
    assert not np.isnan(loss).any()
    rl, rg = ref.check_loss(loss), ref.check_grad(grad)
    q = net.forward(torch.as_tensor(x, device=DEV)).cpu().numpy()
    print('n %d: error / tol: q %.3f, loss %.3f, grad %.3f' % (n, ref.check_q(q), rl, rg))


# ---------------------------------------------------------------------------
# 6. determinism

def test_bit_identical_from_call_to_call(pools):
    p = pools['duo']
    net = _net(p['w'])
    first = _grad(net, p['x'], p['action'], p['target'])
    again = _grad(net, p['x'], p['action'], p['target'])
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    # another (larger, differently filled) workspace
    net._workspace = torch.full((net._workspace.numel() * 2 + 4,), 3.0e38, dtype=torch.float32, device=DEV)[4:]
    x, a, t = (torch.as_tensor(v, device=DEV) for v in (p['x'], p['action'], p['target']))
    loss, grad = net.grad(x, a, t)
    assert np.array_equal(first[0], loss.cpu().numpy()) and np.array_equal(first[1], grad.cpu().numpy())


# ---------------------------------------------------------------------------
# 7. forward agrees with the acting kernel

def test_forward_agrees_with_the_acting_kernel():
    n = 1000
    w = qt.weights_of('duo')
    net = _net(w)
    env = BatchedEnv(DEFAULT_CONFIG, n, device=DEV, b_cap=32, dtype=torch.float32, auto_reset=True)
    env.reset()
    env.rollout(100, 'random', seed=5)
    f = env.features()
    assert int((f[:, :, 0] == 1).sum()) > n      # bullets in flight
    views = [f, qnet.swap_ego(f).contiguous()]
    qact = env.qvalues(net).cpu().numpy()
    worst = 0.0
    for s, v in enumerate(views):
        host = v.cpu().numpy()
        q64 = qnet.forward64(w, host)
        q32 = qt.torch_grad(w, host, np.zeros(n, int), np.zeros(n, np.float32), torch.float32)[0]
        tol = 4.0 * np.abs(q32.astype(np.float64) - q64).max()
        q = net.forward(v)
        assert torch.equal(net.qmax(v), q.max(1)[0])
        for got in (q.cpu().numpy(), qact[:, s]):
            err = np.abs(got - q64).max()
            assert err <= tol, (s, err, tol)
            worst = max(worst, err / tol)
    print('forward and astro_qvalues on a live state: worst error %.3f tol' % worst)


# ---------------------------------------------------------------------------
# 8. saturated outputs

def test_saturated_outputs(pools):
    p = pools['duo']
    n = 200
    w = qt.weights_of('duo', factor=10.0 / 3.0)      # torch-default weights x10
    x, counts = qt.batch('duo', w, p['counts'][:n + 20], ROWS, np.random.RandomState(41), n=n)
    ref = qt.Reference(w, x, p['action'][:n], p['target'][:n])
    net = _net(w)
    q = net.forward(torch.as_tensor(x, device=DEV)).cpu().numpy()
    sat = np.abs(q) == 1.0
    assert sat.sum() >= q.size // 20 and sat[np.arange(n), p['action'][:n]].sum() >= 5, 'not saturated'
    loss, grad = _grad(net, x, p['action'][:n], p['target'][:n])
    assert np.isfinite(grad).all() and np.isfinite(loss).all()
    print('x10: %d of %d q are +-1; error / tol: q %.3f, loss %.3f, grad %.3f'
          % ((np.abs(q) == 1.0).sum(), q.size, ref.check_q(q), ref.check_loss(loss), ref.check_grad(grad)))


# ---------------------------------------------------------------------------
# 9. sgd_step

def test_sgd_step_trains_the_buffer_the_acting_kernel_reads():
    n = 512
    w = qt.weights_of('duo')
    net = _net(w)
    env = BatchedEnv(DEFAULT_CONFIG, n, device=DEV, b_cap=32, dtype=torch.float32, auto_reset=True)
    env.reset()
    env.rollout(60, 'random', seed=7)
    f = env.features()
    g = torch.Generator().manual_seed(3)
    action = torch.randint(0, 6, (n,), generator=g).to(DEV)
    target = (torch.rand(n, generator=g) * 2 - 1).to(DEV)
    old = net.weights.clone()
    ptr = net.weights.data_ptr()
    _, grad = net.grad(f, action, target)
    loss0 = net.sgd_step(f, action, target, lr=1e-2)
    assert torch.equal(net.weights, torch.add(old, grad, alpha=-1e-2)) and not torch.equal(net.weights, old)
    assert net.weights.data_ptr() == ptr == net.c.weights
    for _ in range(19):
        loss = net.sgd_step(f, action, target)
    assert float(loss.mean()) < float(loss0.mean())
    # the acting kernel reads the trained buffer; state_dict() views it
    sd = net.state_dict()
    assert list(sd) == [k for k, _ in qnet.shapes(2, 6)] and sd['v0.bias'].data_ptr() == ptr + 4 * (net.weights.numel() - 6)
    m = qnet.ValueNetwork(False, 6)
    m.load_state_dict(sd)
    fresh = qnet.QNetwork.from_module(m, DEV)
    assert torch.equal(fresh.weights, net.weights)
    assert torch.equal(env.qvalues(net), env.qvalues(fresh))
    assert not torch.equal(env.qvalues(net), env.qvalues(_net(w)))
    print('20 SGD steps on %d samples: mean loss %.4f -> %.4f' % (n, float(loss0.mean()), float(loss.mean())))


# ---------------------------------------------------------------------------
# 10. td_targets

def test_td_targets_on_the_device(pools):
    p = pools['duo']
    n = 300
    rng = np.random.RandomState(51)
    x = p['x'][:n].copy()
    terminal = rng.rand(n) < 0.3
    x[terminal] = np.nan                      # a terminal sample's next state is anything
    reward = rng.uniform(-1, 1, size=n).astype(np.float32)
    discount = rng.uniform(0.5, 1.0, size=n).astype(np.float32)
    net = _net(p['w'])
    got = net.td_targets(torch.as_tensor(reward, device=DEV), torch.as_tensor(discount, device=DEV),
                         torch.as_tensor(x, device=DEV), torch.as_tensor(terminal, device=DEV)).cpu().numpy()
    ref = _ref(p, 517)
    want = np.where(terminal, reward, discount.astype(np.float64) * ref.q64[:n].max(1))
    assert got.dtype == np.float32 and np.array_equal(got[terminal], reward[terminal])
    # discount <= 1: the forward's tolerance, and the product's float32 rounding (|target| <= 1)
    assert np.abs(got - want).max() <= ref.q_tol + 2.0 ** -24
    got = net.td_targets(torch.as_tensor(reward, device=DEV), 0.5, torch.as_tensor(x, device=DEV),
                         torch.as_tensor(terminal, device=DEV).to(torch.uint8)).cpu().numpy()
    assert np.abs(got - np.where(terminal, reward, 0.5 * ref.q64[:n].max(1))).max() <= ref.q_tol + 2.0 ** -24


def test_inputs_are_validated(pools):
    p = pools['duo']
    net = _net(p['w'])
    x = torch.as_tensor(p['x'][:8], device=DEV)
    a, t = torch.zeros(8, dtype=torch.int8, device=DEV), torch.zeros(8, device=DEV)
    for bad in (x.cpu(), x.double(), x[:, :, :10], x.transpose(0, 1), x[:, ::2]):
        with pytest.raises(ValueError):
            net.forward(bad)
        with pytest.raises(ValueError):
            net.grad(bad, a, t)
    with pytest.raises(ValueError):
        net.forward(x, out=torch.empty(8, 5, device=DEV))
    with pytest.raises(ValueError):
        net.grad(x, a.float(), t)
    with pytest.raises(ValueError):
        net.grad(x, a.bool(), t)
    for bad_out in (np.zeros((8, 6), np.float32), [0.0] * 8):
        with pytest.raises(ValueError):
            net.forward(x, out=bad_out)
        with pytest.raises(ValueError):
            net.grad(x, a, t, loss_out=bad_out)
    with pytest.raises(ValueError):
        net.grad(x, a.cpu().numpy(), t)
    with pytest.raises(ValueError):
        net.td_targets(t.cpu(), 0.9, x, a)
    assert net._workspace is None or torch.is_tensor(net._workspace)
    assert _net(p['w'])._workspace is None
    with pytest.raises(ValueError):
        net.grad(x, a[:7], t)
    with pytest.raises(ValueError):
        net.grad(x, a, t.double())
    # wide integers do not wrap into range on their way to int8
    a64 = torch.zeros(8, dtype=torch.int64, device=DEV)
    a64[3], a64[5] = 256, -300
    assert torch.isnan(net.grad(x, a64, t)[0]).tolist() == [False, False, False, True, False, True, False, False]
    # no samples: zeros in grad
    loss, grad = net.grad(x[:0], a[:0], t[:0], grad_out=torch.full_like(net.weights, float('nan')))
    assert loss.numel() == 0 and not grad.any()
    assert tuple(net.forward(x[:0]).shape) == (0, 6)
