#!/usr/bin/env python3
"""Time the actor library (astro_amd.actor: astro_explore, astro_episodes) and
the training tick built on it (astro_amd.train.QTrainer) on the c3 workload.

Workload: bench.py's c3 -- 65,536 envs of 3-planet games, two ships, b_cap 32,
float32 state -- warmed by --warm-ticks of rollout; the replay ring has the
reference's n_steps 100 (102 rows) and is filled before the training tick is
timed.

Timed as tools/bench_replay.py does (HIP events around --reps windows of
--calls back-to-back calls; median, min and 90th percentile per call), every
comparison in this one process, its two sides alternating over --passes:

  step_launch   env.launch(control): the step kernel, the yardstick for a
                launch-bound call
  explore       EpsilonGreedy.apply(control, draw) with the reference's t_in 1.0
                and t_out 0.1 after 200 warm calls (about a tenth of the ships
                hold a policy)
  episodes      Episodes.push(reward, done) on the last step's outputs
  qcontrols     greedy / epsilon=0.1 / explore=eg
  tick          QTrainer.tick() against the loop it replaces (the same calls with
                qcontrols(epsilon=0.1)), 1,024 samples per step

Prints one JSON line (and writes it to --out).  Needs a HIP device with about
20 GB free.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from astro_amd import BatchedEnv, DEFAULT_CONFIG, ReplayBuffer, actor, qnet, train  # noqa: E402


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


def best(results):
    return min(r['median_us'] for r in results)


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
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_actor needs a HIP device'
    dev = 'cuda:0'
    N = args.n_env
    env = BatchedEnv(DEFAULT_CONFIG, N, device=dev, b_cap=32, p_pad=4, planets_only=3, auto_reset=True)
    env.reset()
    env.rollout(args.warm_ticks, 'random')
    module = qnet.ValueNetwork(False, 6)
    with torch.no_grad():
        for p in module.parameters():
            p.mul_(3.0)
    net = qnet.QNetwork.from_module(module, dev)
    R, W, C, P = args.reps, args.warmup, args.calls, args.passes
    res = dict(workload='c3', n_env=N, nships=env.S, n_steps=args.n_steps, n_samples=args.n_samples,
               device=torch.cuda.get_device_name(0))

    # the two kernels next to the step kernel's launch
    eg = actor.EpsilonGreedy(env, seed=1)
    control = env.controls('random', seed=1, tick0=0)
    draw = [0]

    def explore():
        draw[0] += 1
        eg.apply(control, draw[0])

    for _ in range(200):
        explore()
    res['ships_holding_a_policy'] = float((eg.policy >= 0).float().mean())
    env.step(control)
    reward, done = env.reward.clone(), env.done.clone()
    ep = actor.Episodes(env, 4)
    cptr = control.data_ptr()
    res['kernels'] = alternating(dict(step_launch=lambda: env.launch(cptr, stats=False), explore=explore,
                                      episodes=lambda: ep.push(reward, done)), P, R, W, C)
    res['bytes'] = dict(explore=N * 16 + 3 * N * env.S, episodes=N * (4 + 4 + 1))   # hdr line + policy r/w + control; length r/w + done
    k = res['kernels']
    res['explore_us'], res['episodes_us'], res['step_launch_us'] = best(k['explore']), best(k['episodes']), best(k['step_launch'])

    # acting
    res['qcontrols'] = alternating(dict(
        greedy=lambda: env.qcontrols(net),
        epsilon=lambda: env.qcontrols(net, epsilon=0.1, seed=1, tick0=draw[0]),
        explore=lambda: env.qcontrols(net, tick0=draw[0], explore=eg)), P, R, W, C)
    q = res['qcontrols']
    res['qcontrols_us'] = {name: best(q[name]) for name in q}

    # the training tick
    rows, ticks = env.p_pad + env.b_cap, args.n_steps + 2
    buf = ReplayBuffer(N, rows, 2, ticks, n_steps=args.n_steps, device=dev)
    tr = train.QTrainer(env, net, buf, eg, n_samples=args.n_samples, lr=1e-4, seed=3)
    tr.run(ticks + 8)
    assert tr.nstep > 0
    n = args.n_samples

    def parent_tick():
        t = buf.t
        env.features(out=buf.head())
        c = env.qcontrols(net, epsilon=0.1, seed=0, tick0=t)
        _, r, d = env.step(c)
        buf.push(c, r, d)
        if buf.eligible_lower_bound() >= n:
            ids = buf.sample(n, seed=3, draw=t)
            f, a, rr, dd, nf, term = buf.gather(ids)
            loss = net.sgd_step(f, a, net.td_targets(rr, dd, nf, term), lr=1e-4)
            buf.update_loss(ids, loss)

    res['tick'] = alternating(dict(qtrainer=tr.tick, parent_loop=parent_tick), P, R, W, max(1, C // 4))
    res['tick_us'] = dict(qtrainer=best(res['tick']['qtrainer']), parent_loop=best(res['tick']['parent_loop']))
    res['tick_ratio'] = res['tick_us']['qtrainer'] / res['tick_us']['parent_loop']
    env.check_errors()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
