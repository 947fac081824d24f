#!/usr/bin/env python3
"""Time the network-pool kernel (astro_qvalues_pool, include/astro_qpool.h)
against astro_qvalues_ships on the c3 workload, and the training tick with a
pool of opponents against the one with a single snapshot.

Workload and method: tools/bench_league.py's -- 65,536 envs of 3-planet games,
two ships, b_cap 32, float32 state, warmed by --warm-ticks of rollout; networks
of different seeds scaled by 3; HIP events around --reps windows of --calls
back-to-back calls (median, min and 90th percentile per call), all sides in this
one process, taking turns over --passes:

  a  qcontrols((A, B))                       astro_qvalues_ships, the yardstick
  b  qcontrols(Pool: A on ship 0, B on 1)    the same work as one span per ship
  c  qcontrols(Pool.versus(A, 8 rivals))     eight different networks on ship 1
  d  qcontrols(Pool.pairings(4 networks))    twelve blocks, a pairing each
  tick_snapshot / tick_pool                  QTrainer.tick() with opponent='snapshot' and with
                                             opponent='pool', pool_size=8: 1,024 samples, Adam

Prints one JSON line (and writes it to --out).  Needs a HIP device with about
20 GB free.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from astro_amd import BatchedEnv, DEFAULT_CONFIG, ReplayBuffer, actor, league, optim, qnet, train  # noqa: E402
from tools.bench_league import alternating  # noqa: E402


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
    ap.add_argument('--no-tick', action='store_true', help='skip the two training ticks')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_pool needs a HIP device'
    dev = 'cuda:0'
    N = args.n_env

    def world():
        env = BatchedEnv(DEFAULT_CONFIG, N, device=dev, b_cap=32, p_pad=4, planets_only=3, auto_reset=True)
        env.reset()
        env.rollout(args.warm_ticks, 'random')
        return env

    def network(seed):
        torch.manual_seed(seed)
        module = qnet.ValueNetwork(False, 6)
        with torch.no_grad():
            for p in module.parameters():
                p.mul_(3.0)
        return qnet.QNetwork.from_module(module, dev)

    env = world()
    nets = [network(k) for k in range(9)]
    A, B = nets[0], nets[1]
    two = league.Pool(env, [A, B], [(0, 0, N, 0), (1, 0, N, 1)])
    versus = league.Pool.versus(env, A, nets[1:9])
    pairings = league.Pool.pairings(env, nets[:4])
    R, W, C, P = args.reps, args.warmup, args.calls, args.passes
    res = dict(workload='c3', n_env=N, nships=env.S, n_samples=args.n_samples, device=torch.cuda.get_device_name(0))

    # what is timed is right: (b) is (a); (c)'s blocks are the per-ship form's with that rival
    both = env.qcontrols((A, B))
    assert torch.equal(env.qcontrols(two), both)
    c = env.qcontrols(versus)
    for j in (0, 7):
        lo, hi = j * N // 8, (j + 1) * N // 8
        assert torch.equal(c[lo:hi], env.qcontrols((A, nets[1 + j]))[lo:hi])
    sides = alternating(dict(a=lambda: env.qcontrols((A, B)), b=lambda: env.qcontrols(two),
                             c=lambda: env.qcontrols(versus), d=lambda: env.qcontrols(pairings)), P, R, W, C)
    res['qcontrols'] = sides
    m = res['qcontrols_median_us'] = {k: [r['median_us'] for r in v] for k, v in sides.items()}
    for k in 'bcd':
        res[k + '_over_a'] = [x / a for x, a in zip(m[k], m['a'])]
    res['c_below_8a_in_every_pass'] = all(x < 8 * a for x, a in zip(m['c'], m['a']))

    if not args.no_tick:
        rows, ticks = env.p_pad + env.b_cap, args.n_steps + 2

        def trainer(e, **kw):
            buf = ReplayBuffer(N, rows, 2, ticks, n_steps=args.n_steps, device=dev)
            tr = train.QTrainer(e, network(0), buf, actor.EpsilonGreedy(e, seed=1), n_samples=args.n_samples, seed=3,
                                optimizer=optim.Adam(lr=1e-4), opponent_sync=1000, **kw)
            tr.run(ticks + 8)
            assert tr.nstep > 0
            return tr

        snap, pool = trainer(env, opponent='snapshot'), trainer(world(), opponent='pool', pool_size=8)
        t = alternating(dict(tick_snapshot=snap.tick, tick_pool=pool.tick), P, R, W, max(1, C // 4))
        res['tick'] = t
        mt = res['tick_median_us'] = {k: [r['median_us'] for r in v] for k, v in t.items()}
        res['tick_pool_over_snapshot'] = [x / y for x, y in zip(mt['tick_pool'], mt['tick_snapshot'])]
        pool.env.check_errors()
    env.check_errors()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
