#!/usr/bin/env python3
"""Time the fork library (astro_amd.fork: astro_fork) against the same copies
made by torch indexing, on the c3 workload, and one Lookahead.play.

Workload: bench.py's c3 -- 65,536 envs of 3-planet games, two ships, b_cap 32,
float32 state -- after --warm-ticks of rollout.  Three forks:

  all       the whole batch into a second batch of its size, game and stream
  game      the same, the current game alone
  fanout    --fan-envs envs (evenly spread over the batch), each into six envs
            of a scratch batch, game and stream: Lookahead's plan

each timed two ways, alternating over --passes in this one process, as
tools/bench_actor.py times its kernels (HIP events around --reps windows of
--calls back-to-back calls; median, min and 90th percentile per call):

  fork      Fork.apply(): one launch
  torch     what a user writes without the library: ``dst.x[..., d] =
            src.x[..., s]`` for each of the seven arrays (a gather and an
            index_put each; all b_cap bullet slots, live or not)

and set against ``Fork.bytes`` (read plus written, live bullet rows only) at the
8 TB/s peak.  For the whole batch, ``copy_`` of the seven arrays is timed too:
what a user writes when no index is needed.

Then the wall time of ``Lookahead.play(opponent='script', games=1)`` on
--play-envs envs at each of --horizons, with the win / loss / no-winner shares
of its games: one seed (the envs' own), one game per env.

Prints one JSON line (and writes it to --out; the lookahead part to
--lookahead-out).  Needs a HIP device.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from astro_amd import BatchedEnv, DEFAULT_CONFIG, fork  # noqa: E402
from tools.bench_actor import alternating, best  # noqa: E402

PEAK = 8e12   # bytes per second


def torch_fork(src, dst, s, d, game, stream):
    """The same copy by advanced indexing (s, d: int64 index tensors)."""
    if game:
        dst.ships[:, d] = src.ships[:, s]
        dst.ships_b[:, d] = src.ships_b[:, s]
        dst.planets[:, d] = src.planets[:, s]
        dst.bullets[d] = src.bullets[s]
    if game and stream:
        dst.hdr[d] = src.hdr[s]
        dst.stream[d] = src.stream[s]
    elif game:
        dst.hdr[d, :2] = src.hdr[s, :2]
        dst.stream[d, 3] = src.stream[s, 3]
    else:
        dst.hdr[d, 2:] = src.hdr[s, 2:]
        dst.stream[d, :3] = src.stream[s, :3]
    if stream:
        dst.stream_ring[d] = src.stream_ring[s]


def torch_copy(src, dst):
    for k in ('ships', 'ships_b', 'planets', 'bullets', 'hdr', 'stream', 'stream_ring'):
        getattr(dst, k).copy_(getattr(src, k))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n-env', type=int, default=65536)
    ap.add_argument('--fan-envs', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--passes', type=int, default=2)
    ap.add_argument('--warm-ticks', type=int, default=300)
    ap.add_argument('--play-envs', type=int, default=1024)
    ap.add_argument('--horizons', type=int, nargs='*', default=[16, 64])
    ap.add_argument('--out', default='')
    ap.add_argument('--lookahead-out', default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_fork needs a HIP device'
    dev = 'cuda:0'
    N, F = args.n_env, args.fan_envs
    kw = dict(device=dev, b_cap=32, p_pad=4, planets_only=3, auto_reset=True)
    src = BatchedEnv(DEFAULT_CONFIG, N, **kw)
    src.reset()
    src.rollout(args.warm_ticks, 'random')
    whole = BatchedEnv(DEFAULT_CONFIG, N, env_offset=N, **kw)
    whole.reset()
    scratch = BatchedEnv(DEFAULT_CONFIG, 6 * F, env_offset=2 * N, **kw)
    scratch.reset()
    R, W, C, P = args.reps, args.warmup, args.calls, args.passes
    res = dict(workload='c3', n_env=N, nships=src.S, b_cap=src.b_cap, p_pad=src.p_pad, warm_ticks=args.warm_ticks,
               mean_live_bullets=float(src.nbullets.float().mean()), peak_bytes_per_s=PEAK,
               device=torch.cuda.get_device_name(0), cases={})

    fan_s = np.repeat(np.arange(F) * (N // F), 6)
    cases = dict(all=(fork.Fork(src, whole), whole, None, None, True, True),
                 game=(fork.Fork(src, whole, stream=False), whole, None, None, True, False),
                 fanout=(fork.Fork(src, scratch, fan_s, np.arange(6 * F)), scratch, fan_s, np.arange(6 * F), True, True))
    for name, (plan, dst, s, d, game, stream) in cases.items():
        s_t = torch.arange(N, device=dev) if s is None else torch.from_numpy(s).to(dev)
        d_t = torch.arange(N, device=dev) if d is None else torch.from_numpy(d).to(dev)
        fns = dict(fork=plan.apply, torch=lambda: torch_fork(src, dst, s_t, d_t, game, stream))
        if name == 'all':
            fns['torch_copy'] = lambda: torch_copy(src, dst)
        r = alternating(fns, P, R, W, C)
        nbytes = plan.bytes
        us = best(r['fork'])
        out = dict(pairs=plan.m, bytes=nbytes, fork_us=us, torch_us=best(r['torch']),
                   fork_over_torch=us / best(r['torch']), gb_per_s=nbytes / us / 1e3,
                   peak_us=nbytes / PEAK * 1e6, fork_over_peak=us / (nbytes / PEAK * 1e6), runs=r)
        if 'torch_copy' in r:
            out.update(torch_copy_us=best(r['torch_copy']), fork_over_torch_copy=us / best(r['torch_copy']))
        res['cases'][name] = out
    src.check_errors()

    look = dict(envs=args.play_envs, opponent='script', base='script', ship=0, games_per_env=1, discount=0.995,
                seeds=1, device=res['device'], horizons={})
    for h in args.horizons:
        env = BatchedEnv(DEFAULT_CONFIG, args.play_envs, device=dev, b_cap=32)
        env.reset()
        la = fork.Lookahead(env, ship=0, horizon=h)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        winner, length = la.play('script', games=1)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        env.check_errors()
        w = winner.cpu().numpy()[:, 0]
        ticks = -(-int(length.max()) // 64) * 64          # play's loop runs in blocks of 64 ticks
        look['horizons'][str(h)] = dict(win=float((w == 0).mean()), loss=float((w == 1).mean()),
                                        no_winner=float((w == -1).mean()), median_ticks=float(length.float().median()),
                                        wall_s=wall, ticks=ticks, ms_per_tick=wall / ticks * 1e3)
    res['lookahead'] = look
    line = json.dumps(res)
    print(line)
    for path, text in ((args.out, line), (args.lookahead_out, json.dumps(look))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, 'w') as f:
                f.write(text + '\n')


if __name__ == '__main__':
    main()
