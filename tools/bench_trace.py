#!/usr/bin/env python3
"""Time the trace library (astro_amd.record: astro_trace_state,
astro_trace_result) against the two other ways to get the same record, on the
c3 workload.

Workload: bench.py's c3 -- 65,536 envs of 3-planet games, two ships, b_cap 32,
float32 state -- warmed by --warm-ticks of rollout.  For M = 16, 256 and 4,096
recorded envs (evenly spread over the batch) and a ring of 64 slots with six Q
values per ship:

  trace        Recorder.state(control, q) + Recorder.result(reward, done): the
               two launches of one recorded tick
  torch        the same ring filled by torch indexing: one index_select per
               array (ships, bearings and planets are entity-major in the env, so
               each of them also needs the copy that makes it env-major).  It
               does NOT zero the dead planet and bullet rows, which the kernel
               does: the comparison leans towards torch
  to_host      what logs.record_games does per tick: env.to_host() of the whole
               batch (a host clock: it synchronises; independent of M)

trace and torch are timed as tools/bench_actor.py times its kernels (HIP events
around --reps windows of --calls back-to-back ticks; median, min and 90th
percentile per tick), alternating over --passes in this one process.  Then the
wall time of play_q(games=1) on --play-envs envs (games of --max-time seconds)
without a recorder, with a recorder of 64 envs that keeps every game those
envs play until the last env of the batch is done, and with one that stops at
each env's first game (limit=1), alternating, on fresh envs of equal seeds;
with a recorder the time includes decoding the ticks on the host.

Prints one JSON line (and writes it to --out).  Needs a HIP device.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from astro_amd import BatchedEnv, DEFAULT_CONFIG, qnet, record  # noqa: E402
from tools.bench_actor import alternating, best  # noqa: E402

SLOTS = 64


def torch_ring(env, ids, nout):
    dev, S, m = env.device, env.S, ids.numel()
    z = lambda *shape, dt=env.dtype: torch.zeros(shape, dtype=dt, device=dev)   # noqa: E731
    return dict(ships=z(SLOTS, m, S, 4), ships_b=z(SLOTS, m, S), planets=z(SLOTS, m, env.p_pad, 4),
                bullets=z(SLOTS, m, env.b_cap, 4), hdr=z(SLOTS, m, 4, dt=torch.int32), seed=z(SLOTS, m, dt=torch.int32),
                control=z(SLOTS, m, S, dt=torch.int8), q=z(SLOTS, m, S, nout, dt=torch.float32),
                reward=z(SLOTS, m, S, dt=torch.float32), done=z(SLOTS, m, dt=torch.uint8))


def torch_tick(env, ring, ids, slot, control, q, reward, done):
    """One recorded tick by torch indexing (the header's words stay two arrays: hdr and seed)."""
    ring['ships'][slot].copy_(torch.index_select(env.ships, 1, ids).permute(1, 0, 2))
    ring['ships_b'][slot].copy_(torch.index_select(env.ships_b, 1, ids).permute(1, 0))
    ring['planets'][slot].copy_(torch.index_select(env.planets, 1, ids).permute(1, 0, 2))
    torch.index_select(env.bullets, 0, ids, out=ring['bullets'][slot])
    torch.index_select(env.hdr, 0, ids, out=ring['hdr'][slot])
    torch.index_select(env.game_seed, 0, ids, out=ring['seed'][slot])
    torch.index_select(control, 0, ids, out=ring['control'][slot])
    torch.index_select(q, 0, ids, out=ring['q'][slot])
    torch.index_select(reward, 0, ids, out=ring['reward'][slot])
    torch.index_select(done, 0, ids, out=ring['done'][slot])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n-env', type=int, default=65536)
    ap.add_argument('--m', type=int, nargs='+', default=[16, 256, 4096])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--calls', type=int, default=32)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--passes', type=int, default=2)
    ap.add_argument('--warm-ticks', type=int, default=100)
    ap.add_argument('--play-envs', type=int, default=4096)
    ap.add_argument('--play-m', type=int, default=64)
    ap.add_argument('--max-time', type=float, default=20.0, help='max_time of the play_q games, seconds')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_trace needs a HIP device'
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
    res = dict(workload='c3', n_env=N, nships=env.S, b_cap=env.b_cap, p_pad=env.p_pad, slots=SLOTS, nout=net.nout,
               device=torch.cuda.get_device_name(0))

    q = env.qvalues(net)
    control = env.qcontrols(net)
    env.step(control)
    reward, done = env.reward.clone(), env.done.clone()
    el = 4
    res['record_bytes_per_env'] = (env.S + env.p_pad + env.b_cap) * 4 * el + env.S * el + 16 + env.S \
        + env.S * net.nout * 4 + env.S * 4 + 1
    res['per_m'] = {}
    for m in args.m:
        ids = [k * N // m for k in range(m)]
        rec = record.Recorder(env, ids, ticks=SLOTS, q=net.nout)
        ids_t = torch.tensor(ids, dtype=torch.int64, device=dev)
        ring = torch_ring(env, ids_t, net.nout)
        slot = [0]

        def trace():
            if rec.fill == SLOTS:
                rec.fill = 0            # the ring again from slot 0 (no drain: the device side alone is timed)
            rec.state(control, q)
            rec.result(reward, done)

        def by_torch():
            slot[0] = (slot[0] + 1) % SLOTS
            torch_tick(env, ring, ids_t, slot[0], control, q, reward, done)

        r = alternating(dict(trace=trace, torch=by_torch), P, R, W, C)
        # the two forms recorded the same live values (slot 1 of both was written last from the same state)
        same = all(torch.equal(rec.ring[k][1], ring[k][1]) for k in ('ships', 'ships_b', 'control', 'q', 'reward', 'done'))
        res['per_m'][str(m)] = dict(trace_us=best(r['trace']), torch_us=best(r['torch']),
                                    ratio=best(r['trace']) / best(r['torch']), same_values=bool(same), runs=r)

    t = []
    for _ in range(10):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        env.to_host()
        t.append(time.perf_counter() - t0)
    res['to_host_ms'] = dict(median=float(np.median(t)) * 1e3, min=float(np.min(t)) * 1e3)
    host = env.to_host()
    res['to_host_bytes'] = int(sum(v.nbytes for v in host.values()))
    env.check_errors()

    # play_q with and without a recorder
    cfg = DEFAULT_CONFIG._replace(max_time=args.max_time)
    walls = dict(plain=[], recorded=[], recorded_first_game=[])
    games = 0
    for _ in range(P):
        for name in walls:
            ev = BatchedEnv(cfg, args.play_envs, device=dev, b_cap=32, env_offset=1 << 20)
            ev.reset()
            rec = None
            if name != 'plain':
                rec = record.Recorder(ev, [k * args.play_envs // args.play_m for k in range(args.play_m)], q=True,
                                      limit=1 if name == 'recorded_first_game' else None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev.play_q(net, opponent='script', games=1, record=rec)
            torch.cuda.synchronize()
            walls[name].append(time.perf_counter() - t0)
            ev.check_errors()
            if name == 'recorded':
                games = sum(len(g) for g in rec.games.values())
                res['play_q_recorded_ticks'] = sum(len(g.ticks) for gs in rec.games.values() for g in gs)
    res['play_q'] = dict(envs=args.play_envs, m=args.play_m, max_time=args.max_time, opponent='script',
                         plain_s=min(walls['plain']), recorded_s=min(walls['recorded']),
                         recorded_first_game_s=min(walls['recorded_first_game']), runs=walls,
                         recorded_games=games)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
