#!/usr/bin/env python3
"""Time the device Q-network trainer (QNetwork.grad / forward / qmax,
astro_qgrad / astro_qforward) against torch autograd on the c3 workload.

Workload: bench.py's c3 -- 65,536 envs of 3-planet games, b_cap 32, float32
state -- after 200 warm ticks of rollout(..., 'random'), so bullets are live;
``features = env.features()`` ([65536, p_pad + b_cap, 15]) and its first 1,024
samples (the reference's n_samples).

Timed as tools/bench_qnet.py does (HIP events around --reps windows of
--calls back-to-back calls; median, min and 90th percentile per call), at
both sizes:

  grad      net.grad(features, action, target): loss and packed gradient
  torch     astro_amd.qnet.ValueNetwork on the GPU in float32: forward,
            gather, squared error, mean, backward (the gradient's only other
            source)
  forward   net.forward(features) / net.qmax(features) against the module's
            forward under no_grad

Prints one JSON line (and writes it to --out): the times, the ratios, the
largest |g_fused - g_torch| per parameter tensor, the mean live rows, and the
fraction of the 157.3 TFLOPS f32 matrix peak that the multiply-accumulates of
forward plus both backward products on the live rows amount to over the fused
time.  Needs a HIP device.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from astro_amd import BatchedEnv, DEFAULT_CONFIG, qnet  # noqa: E402

PEAK_F32_MATRIX = 157.3e12   # FLOP/s, v_mfma_f32_32x32x2_f32


def timed(fn, reps, warmup, calls):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / calls)
    ms = np.array(ms) * 1e3
    return dict(median_us=float(np.median(ms)), min_us=float(ms.min()), p90_us=float(np.percentile(ms, 90)),
                reps=reps, calls_per_rep=calls)


def macs(features, nout):
    """Multiply-accumulates of (forward, forward + both backward products) on the live rows."""
    nh, nf = qnet.HIDDEN, features.shape[2]
    live = int((~(features[:, :, 0] < 0)).sum())
    n = features.shape[0]
    row_f = nf * nh + 2 * nh * nh
    head_f = 2 * nh * nh + nh * nout
    fwd = live * row_f + n * head_f
    bwd = live * (row_f + 2 * nh * nh) + n * (2 * head_f)
    return fwd, fwd + bwd, live / n


def bench(net, module, features, args):
    n = features.shape[0]
    g = torch.Generator().manual_seed(1)
    action = torch.randint(0, 6, (n,), generator=g).to(features.device)
    target = (torch.rand(n, generator=g) * 2 - 1).to(features.device)
    a8 = action.to(torch.int8)
    loss = torch.empty(n, device=features.device)
    grad = torch.empty_like(net.weights)
    q = torch.empty((n, 6), device=features.device)
    qm = torch.empty(n, device=features.device)
    out = {}

    def fused():
        net.grad(features, a8, target, loss_out=loss, grad_out=grad)

    def torch_grad():
        module.zero_grad(set_to_none=True)
        y = module(features).gather(1, action.view(-1, 1)).view(-1)
        losses = (target - y) ** 2
        losses.mean().backward()
        out['loss'] = losses.detach()

    def fwd():
        net.forward(features, out=q)

    def fwd_max():
        net.qmax(features, out=qm)

    def torch_fwd():
        with torch.no_grad():
            out['q'] = module(features)

    res = dict(n=n, rows=int(features.shape[1]))
    # alternate the paths' measurements so a busy neighbour hits both
    res['grad'] = timed(fused, args.reps, args.warmup, args.calls)
    res['torch_grad'] = timed(torch_grad, args.reps, args.warmup, args.calls)
    res['grad_again'] = timed(fused, args.reps, 2, args.calls)
    res['forward'] = timed(fwd, args.reps, args.warmup, args.calls)
    res['torch_forward'] = timed(torch_fwd, args.reps, args.warmup, args.calls)
    res['qmax'] = timed(fwd_max, args.reps, args.warmup, args.calls)
    tg = qnet.pack({k: p.grad for k, p in module.named_parameters()})
    fg = grad.cpu().numpy()
    diff, k = {}, 0
    for name, shape in qnet.shapes(2, 6):
        size = int(np.prod(shape))
        diff[name] = dict(max_abs_diff=float(np.abs(fg[k:k + size] - tg[k:k + size]).max()),
                          max_abs=float(np.abs(tg[k:k + size]).max()))
        k += size
    f_macs, fb_macs, mean_rows = macs(features, 6)
    t = min(res['grad']['median_us'], res['grad_again']['median_us']) * 1e-6
    tf = res['forward']['median_us'] * 1e-6
    res.update(mean_live_rows=mean_rows, macs_forward=f_macs, macs_forward_backward=fb_macs,
               grad_f32_matrix_peak_fraction=2 * fb_macs / t / PEAK_F32_MATRIX,
               forward_f32_matrix_peak_fraction=2 * f_macs / tf / PEAK_F32_MATRIX,
               grad_speedup_vs_torch=res['torch_grad']['median_us'] / (t * 1e6),
               forward_speedup_vs_torch=res['torch_forward']['median_us'] / res['forward']['median_us'],
               grad_vs_torch=diff,
               max_abs_loss_diff_vs_torch=float((loss - out['loss']).abs().max()),
               max_abs_q_diff_vs_torch=float((q - out['q']).abs().max()),
               qmax_is_row_max=bool(torch.equal(qm, q.max(1)[0])))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n-env', type=int, default=65536)
    ap.add_argument('--small', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--warm-ticks', type=int, default=200)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_qtrain needs a HIP device'
    dev = 'cuda:0'
    env = BatchedEnv(DEFAULT_CONFIG, args.n_env, device=dev, b_cap=32, p_pad=4, planets_only=3, auto_reset=True)
    env.reset()
    env.rollout(args.warm_ticks, 'random')
    torch.manual_seed(7)
    module = qnet.ValueNetwork(False, 6)
    with torch.no_grad():
        for p in module.parameters():
            p.mul_(3.0)
    module = module.to(dev)
    net = qnet.QNetwork.from_module(module, dev)
    features = env.features()
    res = dict(workload='c3', n_env=args.n_env, warm_ticks=args.warm_ticks, device=torch.cuda.get_device_name(0))
    res['full'] = bench(net, module, features, args)
    res['small'] = bench(net, module, features[:args.small].contiguous(), args)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
