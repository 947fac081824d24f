"""CPU-only checks of the Q-network trainer's host side (astro_amd/qnet.py's
grad64 and td_targets, libastro_qtrain.so's argument checks)."""
import ctypes

import numpy as np
import pytest
import torch

import __graft_entry__
from astro_amd import _lib, qnet
from tests import qtrain_util as qt

def _padded_batch(kind, rng):
    """9 samples of up to 7 rows: trailing padding, a padding row in the
    middle of sample 2's rows (NaN outside column 0), one live row in sample 3."""
    x = qt.raw_batch(kind, [5, 7, 4, 1, 6, 2, 3, 7, 5], 7, rng)
    x[2, 4] = x[2, 2]
    x[2, 2, 0], x[2, 2, 1:] = -1.0, np.nan
    return x


@pytest.mark.parametrize('kind', ['duo', 'solo'])
@pytest.mark.parametrize('nout', [1, 3, 6])
def test_grad64_matches_torch_float64_autograd(kind, nout):
    rng = np.random.RandomState(nout)
    w = qt.weights_of(kind, nout)
    x = _padded_batch(kind, rng)
    live = ~(x[..., 0] < 0)
    assert live[2].tolist() == [True, True, False, True, True, False, False] and live[3].sum() == 1
    action = rng.randint(0, nout, size=x.shape[0])
    target = rng.uniform(-1, 1, size=x.shape[0])
    loss, g = qnet.grad64(w, x, action, target)
    q, tloss, tg = qt.torch_grad(w, x, action, target, torch.float64)
    assert list(g) == [n for n, _ in qnet.shapes(1 if kind == 'solo' else 2, nout)]
    assert np.abs(loss - tloss).max() <= 1e-12 * np.abs(tloss).max()
    for k in g:
        assert g[k].shape == tg[k].shape and g[k].dtype == np.float64
        assert np.abs(g[k] - tg[k]).max() <= 1e-12 * np.abs(tg[k]).max(), k
    # an out-of-range action: NaN loss, nothing added, still counted in the mean
    for bad in (-1, nout):
        a2 = action.copy()
        a2[4] = bad
        loss2, g2 = qnet.grad64(w, x, a2, target)
        _, tloss2, tg2 = qt.torch_grad(w, x, a2, target, torch.float64)
        assert np.isnan(loss2[4]) and np.array_equal(np.isnan(loss2), np.isnan(tloss2))
        for k in g:
            assert np.abs(g2[k] - tg2[k]).max() <= 1e-12 * np.abs(tg2[k]).max(), k
        assert any(not np.array_equal(g2[k], g[k]) for k in g)


def _a1_of_row(w, row):
    """f.1's input for one feature row, in float64."""
    h = np.asarray(row, dtype=np.float64) @ w['f0.weight'].astype(np.float64).T + w['f0.bias']
    h = (h / (1 + np.abs(h))) @ w['f.0.weight'].astype(np.float64).T + w['f.0.bias']
    return h / (1 + np.abs(h))


@pytest.mark.parametrize('kind', ['duo', 'solo'])
def test_grad64_sends_a_tie_to_the_first_live_row(kind):
    """Row o of f.1.weight zeroed: every live row ties for unit o.  For one
    sample, dL/d f.1.weight[o] = dL/d f.1.bias[o] * (f.1's input at the row
    that got the gradient): that row is the first live one."""
    rng = np.random.RandomState(5)
    o = 11
    w = qt.weights_of(kind)
    w['f.1.weight'][o] = 0.0
    x = qt.raw_batch(kind, [5, 7, 4, 1, 6, 2], 8, rng)
    x[1, 0, 0] = -1.0                     # sample 1's first LIVE row is row 1
    action = rng.randint(0, 6, size=x.shape[0])
    target = rng.uniform(-1, 1, size=x.shape[0])
    want = np.zeros(32)
    for i in range(x.shape[0]):
        live = np.nonzero(~(x[i, :, 0] < 0))[0]
        assert live[0] == (1 if i == 1 else 0)
        _, g = qnet.grad64(w, x[i:i + 1], action[i:i + 1], target[i:i + 1])
        gb = g['f.1.bias'][o]
        assert gb != 0
        first, last = gb * _a1_of_row(w, x[i, live[0]]), gb * _a1_of_row(w, x[i, live[-1]])
        assert np.abs(g['f.1.weight'][o] - first).max() <= 1e-14 * np.abs(first).max()
        if live.size > 1:
            assert np.abs(g['f.1.weight'][o] - last).max() > 1e-3 * np.abs(first).max()
        want += first / x.shape[0]
    # and in the batch: the samples' mean
    _, g = qnet.grad64(w, x, action, target)
    assert np.abs(g['f.1.weight'][o] - want).max() <= 1e-14 * np.abs(want).max()


def test_bad_arguments_without_gpu():
    """Every bad argument has its own negative code and a message, and is
    rejected before the device is touched (the pointers are not memory)."""
    __graft_entry__.build()
    lib = _lib.load_qtrain()
    P = ctypes.c_void_p
    good = dict(net=_lib.AstroQNet(weights=256, nships=2, nout=6), features=P(1024), n=40, rows=5, action=P(4096),
                target=P(8192), loss=P(12288), grad=P(16384), ws=P(65536))
    need = lib.astro_qgrad_workspace_bytes(ctypes.byref(good['net']), 40)
    assert need == 4 * 4934 * 4         # 2 chunks -> one workgroup of 4 waves, one partial each
    assert lib.astro_qgrad_workspace_bytes(None, 40) == 0
    assert lib.astro_qgrad_workspace_bytes(ctypes.byref(good['net']), 0) == 0
    assert lib.astro_qgrad_workspace_bytes(ctypes.byref(_lib.AstroQNet(nships=2, nout=7)), 40) == 0
    big = lib.astro_qgrad_workspace_bytes(ctypes.byref(good['net']), 2 ** 31 - 1)
    assert big == 256 * 4 * 4934 * 4    # the grid's cap

    def grad(ws_bytes=need, **kw):
        a = dict(good, **kw)
        net = None if a['net'] is None else ctypes.byref(a['net'])
        rc = lib.astro_qgrad(net, a['features'], a['n'], a['rows'], a['action'], a['target'], a['loss'], a['grad'],
                             a['ws'], ws_bytes, None)
        return rc, lib.astro_qtrain_last_error().decode()

    def fwd(q=P(12288), qmax=None, **kw):
        a = dict(good, **kw)
        net = None if a['net'] is None else ctypes.byref(a['net'])
        rc = lib.astro_qforward(net, a['features'], a['n'], a['rows'], q, qmax, None)
        return rc, lib.astro_qtrain_last_error().decode()

    cases = [
        (dict(net=None), 'net is NULL'),
        (dict(net=_lib.AstroQNet(weights=256, nships=3, nout=6)), 'nships'),
        (dict(net=_lib.AstroQNet(weights=256, nships=0, nout=6)), 'nships'),
        (dict(net=_lib.AstroQNet(weights=256, nships=2, nout=0)), 'nout'),
        (dict(net=_lib.AstroQNet(weights=256, nships=2, nout=7)), 'nout'),
        (dict(net=_lib.AstroQNet(weights=None, nships=2, nout=6)), 'weights'),
        (dict(net=_lib.AstroQNet(weights=258, nships=2, nout=6)), 'weights'),
        (dict(features=None), 'features is NULL'),
        (dict(n=-1), 'n < 0'),
        (dict(rows=0), 'rows'),
        (dict(action=None), 'action is NULL'),
        (dict(target=None), 'target is NULL'),
        (dict(grad=None), 'grad is NULL'),
        (dict(ws=None), 'workspace'),
        (dict(ws_bytes=need - 1), 'workspace'),
        (dict(features=P(1026)), 'aligned'),
        (dict(target=P(8193)), 'aligned'),
        (dict(loss=P(12290)), 'aligned'),
        (dict(grad=P(16385)), 'aligned'),
        (dict(ws=P(65544)), 'aligned'),
    ]
    codes = {}
    for kw, word in cases:
        rc, msg = grad(**kw)
        assert -200 < rc < 0 and word in msg, (kw, rc, msg)
        codes.setdefault(rc, set()).add(word)
    # one code per kind of mistake, and the codes of the header
    assert all(len(v) == 1 for v in codes.values()), codes
    assert sorted(codes) == [-119, -118, -117, -116, -115, -112, -111, -110, -105, -102, -101, -100]
    # astro_qforward: the same codes for what it shares
    for kw, word in cases[:10]:
        if 'ws_bytes' in kw or 'ws' in kw:
            continue
        rc, msg = fwd(**kw)
        assert -200 < rc < 0 and word in msg, (kw, rc, msg)
    rc, msg = fwd(q=None, qmax=None)
    assert rc == -114 and 'both NULL' in msg
    assert fwd(q=P(12289))[0] == -119 and fwd(q=None, qmax=P(3))[0] == -119
    # n == 0: astro_qforward has nothing to do, whatever the arrays are ...
    assert fwd(n=0, features=None)[0] == 0
    assert fwd(n=0, features=None, net=_lib.AstroQNet(weights=None, nships=1, nout=2))[0] == 0
    # ... but its other arguments are still checked, and astro_qgrad still needs grad (it writes zeros there)
    assert fwd(n=0, rows=0)[0] == -112 and fwd(n=0, q=None)[0] == -114
    # (its success path -- n == 0 with a valid grad returns 0 and zeroes grad -- launches the reduction
    # kernel, so it is checked on the device: tests/test_gpu_qtrain.py::test_inputs_are_validated)
    assert grad(n=0, features=None, action=None, target=None, ws=None, grad=None)[0] == -117


def test_td_targets_selects_by_terminal():
    """rl.py:281-291 on CPU tensors through the private helper: reward where
    terminal, discount * qmax elsewhere; a terminal sample's qmax may be NaN."""
    reward = torch.tensor([1.0, -1.0, 0.5, 0.0, 0.25])
    qmax = torch.tensor([0.5, float('nan'), -0.25, float('nan'), 1.0])
    terminal = torch.tensor([False, True, False, True, False])
    discount = torch.tensor([0.9, 0.5, 0.8, 0.7, 1.0])
    got = qnet._td_targets(reward, discount, qmax, terminal)
    want = np.array([0.9 * 0.5, -1.0, 0.8 * -0.25, 0.0, 1.0], dtype=np.float32)
    assert got.dtype == torch.float32
    assert np.array_equal(got.numpy(), np.where(terminal.numpy(), reward.numpy(), discount.numpy() * qmax.numpy()))
    assert np.allclose(got.numpy(), want, rtol=1e-7, atol=0) and not np.isnan(got.numpy()).any()
    # a scalar discount and a uint8 mask (the env's `done`)
    got = qnet._td_targets(reward, 0.5, qmax, terminal.to(torch.uint8))
    assert np.array_equal(got.numpy(), np.where(terminal.numpy(), reward.numpy(), np.float32(0.5) * qmax.numpy()))


def test_qnetwork_training_surface_needs_a_device():
    """The Python surface exists and QNetwork still refuses a CPU device."""
    for name in ('forward', 'qmax', 'td_targets', 'grad', 'sgd_step', 'state_dict'):
        assert callable(getattr(qnet.QNetwork, name))
    with pytest.raises(ValueError):
        qnet.QNetwork(qnet.pack(qt.weights_of('duo')), 2, 6, 'cpu')
