#!/usr/bin/env python3
"""Time the per-ship Q-network kernel (astro_qvalues_ships, include/astro_qduel.h)
against astro_qvalues on the c3 workload, and the training tick with a scripted
opponent, which now evaluates ship 0 only.

Workload: bench.py's c3 -- 65,536 envs of 3-planet games, two ships, b_cap 32,
float32 state -- warmed by --warm-ticks of rollout.  A and B are two
ValueNetworks of different seeds, scaled by 3 as tools/bench_actor.py scales its
network.

Timed as tools/bench_actor.py does (HIP events around --reps windows of --calls
back-to-back calls; median, min and 90th percentile per call), all sides in this
one process, taking turns over --passes:

  a  qcontrols(A)                  astro_qvalues, one network for both ships
  b  qcontrols((A, B))             astro_qvalues_ships, a network per ship
  c  qcontrols((A, None))          astro_qvalues_ships, ship 0 only
  d  qcontrols(A), qcontrols(B) and the column merge: two networks without the
     new kernel
  e  QTrainer.tick() with opponent='script', 1,024 samples per step, Adam

--tick-only times (e) alone and uses nothing the parent commit lacks, so the same
file can time another checkout: --root names the tree whose astro_amd is
imported.  Alternate the trees in one session and compare the medians.

Prints one JSON line (and writes it to --out).  Needs a HIP device with about
20 GB free.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch


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


def alternating(fns, passes, reps, warmup, calls):
    """{name: [one result per pass]}, the functions taking turns."""
    out = {k: [] for k in fns}
    for _ in range(passes):
        for k, fn in fns.items():
            out[k].append(timed(fn, reps, warmup, calls))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n-env', type=int, default=65536)
    ap.add_argument('--n-steps', type=int, default=100)
    ap.add_argument('--n-samples', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--passes', type=int, default=2)
    ap.add_argument('--warm-ticks', type=int, default=100)
    ap.add_argument('--tick-only', action='store_true', help='time (e) alone')
    ap.add_argument('--root', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'),
                    help='the checkout whose astro_amd is timed (built already)')
    ap.add_argument('--label', default='tree')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import astro_amd
    from astro_amd import BatchedEnv, DEFAULT_CONFIG, ReplayBuffer, actor, optim, qnet, train

    assert torch.cuda.is_available(), 'bench_league needs a HIP device'
    assert os.path.abspath(os.path.dirname(os.path.dirname(astro_amd.__file__))) == os.path.abspath(args.root)
    dev = 'cuda:0'
    N = args.n_env
    env = BatchedEnv(DEFAULT_CONFIG, N, device=dev, b_cap=32, p_pad=4, planets_only=3, auto_reset=True)
    env.reset()
    env.rollout(args.warm_ticks, 'random')

    def network(seed):
        torch.manual_seed(seed)
        module = qnet.ValueNetwork(False, 6)
        with torch.no_grad():
            for p in module.parameters():
                p.mul_(3.0)
        return qnet.QNetwork.from_module(module, dev)

    A, B = network(0), network(1)
    R, W, C, P = args.reps, args.warmup, args.calls, args.passes
    res = dict(workload='c3', label=args.label, n_env=N, nships=env.S, n_samples=args.n_samples,
               device=torch.cuda.get_device_name(0))

    if not args.tick_only:
        def merged():
            c = env.qcontrols(A)
            c[:, 1] = env.qcontrols(B)[:, 1]
            return c

        both = env.qcontrols((A, B))
        assert torch.equal(both, merged()) and torch.equal(env.qcontrols((A, None))[:, 0], both[:, 0])
        sides = alternating(dict(a=lambda: env.qcontrols(A), b=lambda: env.qcontrols((A, B)),
                                 c=lambda: env.qcontrols((A, None)), d=merged), P, R, W, C)
        res['qcontrols'] = sides
        res['qcontrols_median_us'] = {k: [r['median_us'] for r in v] for k, v in sides.items()}
        m = res['qcontrols_median_us']
        res['b_below_d_in_every_pass'] = all(b < d for b, d in zip(m['b'], m['d']))
        res['c_not_above_a_in_every_pass'] = all(c <= a for c, a in zip(m['c'], m['a']))
        res['b_over_a'] = [b / a for b, a in zip(m['b'], m['a'])]

    # (e) the training tick against ScriptBot
    rows, ticks = env.p_pad + env.b_cap, args.n_steps + 2
    buf = ReplayBuffer(N, rows, 2, ticks, n_steps=args.n_steps, device=dev)
    eg = actor.EpsilonGreedy(env, seed=1)
    tr = train.QTrainer(env, A, buf, eg, n_samples=args.n_samples, seed=3, optimizer=optim.Adam(lr=1e-4),
                        opponent='script')
    tr.run(ticks + 8)
    assert tr.nstep > 0
    res['tick_script'] = alternating(dict(tick=tr.tick), P, R, W, max(1, C // 4))['tick']
    res['tick_script_median_us'] = [r['median_us'] for r in res['tick_script']]
    env.check_errors()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a' if args.tick_only else 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
