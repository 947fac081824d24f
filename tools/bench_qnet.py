#!/usr/bin/env python3
"""Time the fused Q-network policy (BatchedEnv.qcontrols, astro_qvalues)
against the unfused path on the c3 workload.

Workload: bench.py's c3 -- 65,536 envs of 3-planet games, b_cap 32, float32
state -- after 200 warm ticks of rollout(..., 'random'), so bullets are live.

Timed (after warm-up, HIP events around --reps windows of --calls
back-to-back calls each; median, min and 90th percentile of the per-call
time over the windows):

  fused     env.qcontrols(net, q_out=q): Q values and argmax, one kernel
  torch     env.features(), astro_amd.qnet.ValueNetwork on the GPU in float32
            on the features and on their column-swapped copy, argmax
  features  env.features() alone

Prints one JSON line (and writes it to --out): the three times, the mean live
rows per env, the multiply-accumulates the network needs on the live rows
(useful) and those the kernel's MFMA tiles issue (rows padded to 32 per tile,
the head to 32 outputs), and the fraction of the 157.3 TFLOPS f32 matrix peak
that the useful ones over the fused time amount to.  Needs a HIP device.
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
    """Per-call time of fn: ``reps`` windows of ``calls`` back-to-back calls
    between two HIP events (one call per window would time the host's launch
    path, not the device)."""
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


def macs(env, nout):
    """(useful, issued) multiply-accumulates of one astro_qvalues call on env's state."""
    S, nh = env.S, qnet.HIDDEN
    nf = 5 + 5 * S
    rows = (env.nplanets + env.nbullets).cpu().numpy().astype(np.int64)
    per_row = nf * nh + 2 * nh * nh
    head = 2 * nh * nh + nh * nout
    useful = int(rows.sum()) * S * per_row + env.n_env * S * head
    ch = 32 // S                                       # envs per chunk (csrc/astro_qnet.hip)
    pad = (-rows.size) % ch
    items = np.pad(rows, (0, pad)).reshape(-1, ch).sum(1) * S
    tiles = int(((items + 31) // 32).sum())
    chunks = items.size
    issued = tiles * 32 * (6 * nh + 2 * nh * nh) + env.n_env * S * 5 * S * nh + chunks * 32 * 3 * nh * nh
    return useful, issued, float(rows.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n-env', type=int, default=65536)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--warm-ticks', type=int, default=200)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_qnet needs a HIP device'
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

    q = torch.empty((args.n_env, 2, 6), dtype=torch.float32, device=dev)
    feat = torch.empty((args.n_env, env.p_pad + env.b_cap, 15), dtype=torch.float32, device=dev)
    out = {}

    def fused():
        out['fused'] = env.qcontrols(net, q_out=q)

    def unfused():
        with torch.no_grad():
            f = env.features(out=feat)
            qq = torch.stack((module(f), module(qnet.swap_ego(f))), 1)
            out['torch_q'] = qq
            out['torch'] = qq.argmax(-1)

    def features():
        env.features(out=feat)

    res = dict(workload='c3', n_env=args.n_env, warm_ticks=args.warm_ticks, device=torch.cuda.get_device_name(0))
    # alternate the two paths' measurements so a busy neighbour hits both
    res['fused'] = timed(fused, args.reps, args.warmup, args.calls)
    res['torch'] = timed(unfused, args.reps, args.warmup, args.calls)
    res['features'] = timed(features, args.reps, args.warmup, args.calls)
    res['fused_again'] = timed(fused, args.reps, 2, args.calls)
    dq = (out['torch_q'] - q).abs().max().item()
    agree = (out['torch'].to(torch.int8) == out['fused']).float().mean().item()
    useful, issued, mean_rows = macs(env, 6)
    t = min(res['fused']['median_us'], res['fused_again']['median_us']) * 1e-6
    res.update(mean_live_rows=mean_rows, macs_useful=useful, macs_issued=issued,
               f32_matrix_peak_fraction=2 * useful / t / PEAK_F32_MATRIX,
               issued_peak_fraction=2 * issued / t / PEAK_F32_MATRIX,
               speedup_vs_torch=res['torch']['median_us'] / (t * 1e6),
               max_abs_q_diff_vs_torch_f32=dq, argmax_agreement=agree)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
