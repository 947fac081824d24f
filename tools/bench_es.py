#!/usr/bin/env python3
"""Time the evolution strategy's three launches (astro_amd.es: astro_es_perturb,
astro_es_score, astro_es_gradient) against the same work in torch ops, and a
whole ``ESTrainer.generation()`` split into play and the rest.

tools/bench_search.py's method: HIP events around --reps windows of --calls
back-to-back calls, the contenders alternating over --passes in this one
process; the best pass's median per call is compared.

(a) perturb   ``es.perturb`` against the same rows built with ``torch.randn``
              and two elementwise ops (fresh Gaussian noise per call, written
              into a stored [pairs, nparams] tensor that the torch gradient
              would read back: the route without this library).
(b) score     ``es.score`` against the torch ops ``league.tournament`` counts
              with (a block index, a slot per code, one ``scatter_add_``) plus
              the masked tick sum and the fitness formula.
(c) gradient  ``es.gradient`` against ``(u_diff[:, None] * eps).sum(0)`` on a
              STORED noise tensor, with the rank transform in torch
              (``argsort`` twice; ties are not averaged there).
(d) generation  ``ESTrainer.generation()`` on --n-env envs, 2 * --pairs
              members, against ScriptBot: the whole call, and the same call
              with the three launches and the optimiser step taken out (play
              alone), both from the same forked states.

Prints one JSON line and writes it to --out.  Needs a HIP device.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from astro_amd import BatchedEnv, DEFAULT_CONFIG, es, qnet  # noqa: E402
from tools.bench_actor import alternating, best, timed  # noqa: E402


def torch_perturb(theta, sigma, eps, members):
    torch.randn(eps.shape, out=eps)
    d = sigma * eps
    torch.add(theta[None, :], d, out=members[0::2])
    torch.sub(theta[None, :], d, out=members[1::2])
    return members


def torch_score(winner, ticks, block, K, ship, draw, survive, timeout):
    """W, L, D per block as league.tournament counts them, the lost ticks, the fitness."""
    w = winner.to(torch.int64)
    one = torch.ones_like(w)
    code = torch.where(w == ship, one * 0, torch.where(w == -1, one * 2, torch.where(w == -2, one * 3, one)))
    slot = block[:, None] * 4 + code
    counts = torch.zeros(4 * K, dtype=torch.int64, device=winner.device)
    counts.scatter_add_(0, slot.reshape(-1), torch.ones(slot.numel(), dtype=torch.int64, device=winner.device))
    counts = counts.view(K, 4)
    lost = torch.zeros(K, dtype=torch.int64, device=winner.device)
    lost.scatter_add_(0, block[:, None].expand_as(w).reshape(-1),
                      torch.where(code == 1, ticks.clamp(max=timeout).to(torch.int64), one * 0).reshape(-1))
    W, L, D = counts[:, 0].double(), counts[:, 1].double(), counts[:, 2].double()
    return (((W - L) + draw * D + survive * (lost.double() / timeout)) / (W + L + D)).float()


def torch_gradient(fitness, eps, sigma, ranks):
    u = fitness
    if ranks:
        K = fitness.numel()
        u = fitness.argsort().argsort().float() / (K - 1) - 0.5
    du = (u[0::2] - u[1::2]).double()
    return (-(du[:, None] * eps.double()).sum(0) / (2.0 * eps.shape[0] * sigma)).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n-env', type=int, default=4096)
    ap.add_argument('--pairs', type=int, default=16)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--passes', type=int, default=2)
    ap.add_argument('--generations', type=int, default=5)
    ap.add_argument('--out', default=os.path.join('profiles', 'es', 'bench_es.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_es needs a HIP device'
    dev = 'cuda:0'
    R, W, C, P = args.reps, args.warmup, args.calls, args.passes
    sigma = 0.05
    torch.manual_seed(0)
    net = qnet.QNetwork.from_module(qnet.ValueNetwork(solo=False), dev)
    nparams = int(net.weights.numel())
    res = dict(device=torch.cuda.get_device_name(0), reps=R, calls=C, passes=P, nparams=nparams, perturb=[], score=[],
               gradient=[], generation=[])

    for pairs, n in ((1, 257), (16, nparams), (512, nparams)):
        theta = torch.randn(n, device=dev)
        members = torch.empty((2 * pairs, n), device=dev)
        eps = torch.empty((pairs, n), device=dev)
        t = alternating(dict(kernel=lambda: es.perturb(theta, members, pairs, sigma, 1, 0),
                             torch=lambda: torch_perturb(theta, sigma, eps, members)), P, R, W, C)
        res['perturb'].append(dict(pairs=pairs, nparams=n, stored_noise_bytes=int(eps.numel() * 4),
                                   kernel_us=best(t['kernel']), torch_us=best(t['torch']),
                                   kernel_over_torch=best(t['kernel']) / best(t['torch']), runs=t))
        for ranks in (True, False):
            fitness = torch.randn(2 * pairs, device=dev)
            grad = torch.empty(n, device=dev)
            shaping = 'ranks' if ranks else 'raw'
            eps_h = torch.from_numpy(es.noise_host(1, 0, 0, pairs, n)).to(dev)     # the noise the kernel regenerates
            g = es.gradient(fitness, n, sigma, 1, 0, shaping, out=grad)
            tg = torch_gradient(fitness, eps_h, sigma, ranks)
            err = float((g - tg).abs().max() / tg.abs().max().clamp(min=1e-30))
            t = alternating(dict(kernel=lambda: es.gradient(fitness, n, sigma, 1, 0, shaping, out=grad),
                                 torch=lambda: torch_gradient(fitness, eps_h, sigma, ranks)), P, R, W, C)
            res['gradient'].append(dict(pairs=pairs, nparams=n, shaping=shaping, max_rel_difference=err,
                                        kernel_us=best(t['kernel']), torch_us=best(t['torch']),
                                        kernel_over_torch=best(t['kernel']) / best(t['torch']), runs=t))

    rng = np.random.RandomState(0)
    for N, K, G in ((64, 4, 1), (args.n_env, 2 * args.pairs, 1), (65536, 32, 4)):
        winner = torch.from_numpy(rng.choice(np.array([0, 1, -1, -2], np.int8), size=(N, G))).to(dev)
        ticks = torch.from_numpy(rng.randint(1, 6000, size=(N, G)).astype(np.int32)).to(dev)
        block = torch.tensor([k for k, (lo, hi) in enumerate(es.blocks(N, K)) for _ in range(hi - lo)], dtype=torch.int64,
                             device=dev)
        fit = torch.empty(K, device=dev)
        f = es.score(winner, ticks, K, 0, 0.5, 0.5, 3000, fitness=fit)[0]
        tf = torch_score(winner, ticks, block, K, 0, 0.5, 0.5, 3000)
        same = bool(torch.equal(f.view(torch.int32), tf.view(torch.int32)))
        t = alternating(dict(kernel=lambda: es.score(winner, ticks, K, 0, 0.5, 0.5, 3000, fitness=fit),
                             torch=lambda: torch_score(winner, ticks, block, K, 0, 0.5, 0.5, 3000)), P, R, W, C)
        res['score'].append(dict(n_env=N, members=K, games=G, bit_identical=same, kernel_us=best(t['kernel']),
                                 torch_us=best(t['torch']), kernel_over_torch=best(t['kernel']) / best(t['torch']), runs=t))

    # a whole generation, and its play alone
    cfg = DEFAULT_CONFIG._replace(max_time=10.0)
    env = BatchedEnv(cfg, args.n_env, device=dev, b_cap=32, auto_reset=True)
    env.reset()
    tr = es.ESTrainer(env, net, opponent='script', pairs=args.pairs, sigma=sigma, draw=0.5, survive=0.5)
    snap = env.snapshot()
    ticks_run = [0]
    step = env.step

    def counted(*a, **kw):
        ticks_run[0] += 1
        return step(*a, **kw)
    env.step = counted

    def play_alone():
        env.restore(snap)
        tr.plan.apply()
        env._play_q(tr.seats, None, 1, None, None, 0)

    def whole():
        env.restore(snap)
        tr.pop.generation = 0          # the same noise, hence the same games, every time
        tr.generation()

    theta0 = net.weights.clone()

    def whole_from_theta0():
        net.weights.copy_(theta0)
        whole()

    def play_from_theta0():
        net.weights.copy_(theta0)
        tr.pop.generation = 0
        tr.perturb(0)
        play_alone()

    whole_from_theta0()
    ticks_run[0] = 0
    whole_from_theta0()
    per_generation = ticks_run[0]
    t = alternating(dict(generation=whole_from_theta0, play=play_from_theta0), P, args.generations, 1, 1)
    g_us, p_us = best(t['generation']), best(t['play'])
    rest = timed(lambda: (tr.perturb(0), es.score(tr.episodes.winner, tr.episodes.ticks, tr.pop.K, 0, 0.5, 0.5,
                                                  env.schedule.timeout_tick, fitness=tr.fitness), tr.update()), R, W, C)
    res['generation'].append(dict(n_env=args.n_env, members=tr.pop.K, nparams=nparams, opponent='script',
                                  ticks_per_generation=per_generation, generation_us=g_us, play_us=p_us,
                                  rest_by_difference_us=g_us - p_us, rest_back_to_back_us=rest['median_us'],
                                  rest_share=rest['median_us'] / g_us, runs=t, rest_runs=rest))
    env.check_errors()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
