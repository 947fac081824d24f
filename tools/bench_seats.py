#!/usr/bin/env python3
"""Time the seats kernel (astro_controls_seats, include/astro_seats.h) against
astro_controls on the c3 workload, and the training tick against a ladder of
eight next to opponent='script' and opponent='pool'.

Workload and method: tools/bench_pool.py's -- 65,536 envs of 3-planet games, two
ships, b_cap 32, float32 state, warmed by --warm-ticks of rollout; HIP events
around --reps windows of --calls back-to-back calls (median, min and 90th
percentile per call), all sides in this one process, taking turns over --passes:

  a  controls('script')                       astro_controls, the yardstick
  b  seat_controls(one seat per ship)         the same decisions through a two-entry table
  c  seat_controls(2 x 32 seats)              the full table: 32 blocks per ship, arguments of their own
  d  seat_controls(ship 1 only)               one seat: half the decisions
  tick_script / tick_ladder / tick_pool       QTrainer.tick() with opponent='script', a ladder of eight
                                              (four Scripts, 'nothing', 'random', two networks) and
                                              opponent='pool', pool_size=8: 1,024 samples, Adam
  tune_script                                 with --tune: one league.tune_script run (wall time)

Prints one JSON line (and writes it to --out).  Needs a HIP device with about
20 GB free.
"""
import argparse
import json
import os
import sys
import time

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
    ap.add_argument('--no-tick', action='store_true', help='skip the three training ticks')
    ap.add_argument('--tune', action='store_true', help='one tune_script run: 4,096 envs, 4 rounds of 4 candidates')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_seats needs a HIP device'
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
    scripts = [league.Script(0.1 + 0.005 * k, 0.45 - 0.005 * k) for k in range(32)]
    one = league.Seats(env, ['script'], [(0, 0, N, 0), (1, 0, N, 0)])
    full = league.Seats(env, scripts, [(s, k * N // 32, (k + 1) * N // 32, k) for k in range(32) for s in range(2)])
    half = league.Seats(env, ['script'], [(1, 0, N, 0)])
    R, W, C, P = args.reps, args.warmup, args.calls, args.passes
    res = dict(workload='c3', n_env=N, nships=env.S, n_samples=args.n_samples, device=torch.cuda.get_device_name(0))

    # what is timed is right: (b) is (a); (c)'s blocks are astro_controls' with that block's arguments
    whole = env.controls('script')
    out = torch.empty_like(whole)
    assert torch.equal(env.seat_controls(one, out=out), whole)
    c = env.seat_controls(full)
    for k in (0, 31):
        lo, hi = k * N // 32, (k + 1) * N // 32
        assert torch.equal(c[lo:hi], env.controls('script', script_args=scripts[k].args)[lo:hi])
    sides = alternating(dict(a=lambda: env.controls('script'), b=lambda: env.seat_controls(one, out=out),
                             c=lambda: env.seat_controls(full, out=out), d=lambda: env.seat_controls(half, out=out)),
                        P, R, W, C)
    res['controls'] = sides
    m = res['controls_median_us'] = {k: [r['median_us'] for r in v] for k, v in sides.items()}
    for k in 'bcd':
        res[k + '_over_a'] = [x / a for x, a in zip(m[k], m['a'])]
    res['b_within_a_quarter_in_every_pass'] = all(x <= 1.25 * a for x, a in zip(m['b'], m['a']))

    if not args.no_tick:
        rows, ticks = env.p_pad + env.b_cap, args.n_steps + 2

        def trainer(e, **kw):
            buf = ReplayBuffer(N, rows, 2, ticks, n_steps=args.n_steps, device=dev)
            tr = train.QTrainer(e, network(0), buf, actor.EpsilonGreedy(e, seed=1), n_samples=args.n_samples, seed=3,
                                optimizer=optim.Adam(lr=1e-4), **kw)
            tr.run(ticks + 8)
            assert tr.nstep > 0
            return tr

        ladder = [league.Script(0.0, 0.45), league.Script(0.3, 0.45), league.Script(0.1, 1.5), 'script', 'nothing',
                  'random', network(1), network(2)]
        runs = dict(tick_script=trainer(env, opponent='script'), tick_ladder=trainer(world(), opponent=ladder),
                    tick_pool=trainer(world(), opponent='pool', pool_size=8, opponent_sync=1000))
        t = alternating({k: v.tick for k, v in runs.items()}, P, R, W, max(1, C // 4))
        res['tick'] = t
        mt = res['tick_median_us'] = {k: [r['median_us'] for r in v] for k, v in t.items()}
        res['tick_ladder_over_script'] = [x / y for x, y in zip(mt['tick_ladder'], mt['tick_script'])]
        for tr in runs.values():
            tr.env.check_errors()

    if args.tune:
        small = BatchedEnv(DEFAULT_CONFIG, 4096, device=dev, b_cap=32, auto_reset=True)
        small.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        best, history = league.tune_script(small, max_trials=2000, threshold=0.95, max_mutations=4, scale=0.05,
                                           candidates=4, seed=0)
        res['tune_script'] = dict(n_env=4096, max_trials=2000, threshold=0.95, rounds=4, candidates=4, scale=0.05,
                                  seconds=time.perf_counter() - t0, best=best,
                                  rounds_log=[dict(verdicts=h['verdicts'], wins=h['wins'], games=h['games'],
                                                   passes=h['passes']) for h in history])
        small.check_errors()
    env.check_errors()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
