#!/usr/bin/env python3
"""Time the search's value reduction (astro_amd.search: astro_search_values)
against the same reduction in torch ops, and a whole Lookahead tick with each.

Shape: --n-env envs (1,024) of DEFAULT_CONFIG, two ships, b_cap 32, aged
--warm-ticks (300) ticks of random play.  tools/bench_fork.py's method: HIP
events around --reps windows of --calls back-to-back calls, the contenders
alternating over --passes in this one process; the best pass's median per call
is compared.

(a) reduce   ``search.reduce`` (one launch, values and the decision) against
             ``search.reduce_torch`` (the ops ``fork.Lookahead`` ran before the
             kernel; values and the decision) on the SAME arrays: the outputs of
             a real branched step and rollout of the aged envs, at each of
             --horizons, with and without a leaf, with R = 1 and R = 6.  Their
             results are compared bit for bit before they are timed.
(b) tick     a whole ``Lookahead.controls()`` against the same tick with the
             torch reduction in the kernel's place -- the fork, the scripted
             controls, the step and the rollout are the same calls in both, so
             this is the tick before the kernel existed.

Prints one JSON line and writes it to --out.  Needs a HIP device.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from astro_amd import BatchedEnv, DEFAULT_CONFIG, fork, qnet, search  # noqa: E402
from tools.bench_actor import alternating, best  # noqa: E402


def torch_tick(la):
    """``Lookahead.controls()`` as it was before the kernel: the same launches, then the torch reduction."""
    sc = la.scratch
    la.plan.apply()
    c = sc.controls(la.base, script_args=la.script_args)
    c[:, la.ship] = la._branch
    _, r0, d0 = sc.step(c, auto_reset=True)
    r, d = sc.rollout(la.horizon - 1, la.base, auto_reset=True, script_args=la.script_args)
    own = la.env.controls(la.base, script_args=la.script_args)[:, la.ship]
    return search.reduce_torch(r0, d0, r, d, gamma=la._gamma, ship=la.ship, own=own)[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n-env', type=int, default=1024)
    ap.add_argument('--horizons', type=int, nargs='*', default=[16, 64])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--passes', type=int, default=2)
    ap.add_argument('--warm-ticks', type=int, default=300)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_search needs a HIP device'
    dev = 'cuda:0'
    N = args.n_env
    R, W, C, P = args.reps, args.warmup, args.calls, args.passes
    env = BatchedEnv(DEFAULT_CONFIG, N, device=dev, b_cap=32, auto_reset=True)
    env.reset()
    env.rollout(args.warm_ticks, 'random')
    torch.manual_seed(0)
    module = qnet.ValueNetwork(False, 6)
    net = qnet.QNetwork.from_module(module, dev)
    res = dict(n_env=N, nships=env.S, b_cap=env.b_cap, warm_ticks=args.warm_ticks, device=torch.cuda.get_device_name(0),
               reps=R, calls=C, passes=P, reduce=[], tick=[])

    for h in args.horizons:
        for reply in (False, True):
            la = fork.Lookahead(env, ship=0, horizon=h, leaf=net, reply=reply)
            la.values()
            r0, d0, r, d, q = la._outputs
            own = la._own()
            ended = float((torch.cat([d0[None], d]) != 0).any(0).float().mean())
            for leaf in (None, q):
                kw = dict(gamma=la._gamma, ship=0, replies=la.replies, leaf=leaf, own=own)
                v, c = search.reduce(r0, d0, r, d, **kw)
                tv, tc = search.reduce_torch(r0, d0, r, d, **kw)
                same = bool(torch.equal(v.view(torch.int32), tv.contiguous().view(torch.int32)) and torch.equal(c, tc))
                t = alternating(dict(kernel=lambda: search.reduce(r0, d0, r, d, **kw),
                                     torch=lambda: search.reduce_torch(r0, d0, r, d, **kw)), P, R, W, C)
                res['reduce'].append(dict(horizon=h, replies=la.replies, leaf=leaf is not None, branches=int(d0.numel()),
                                          ended_share=ended, bit_identical=same, kernel_us=best(t['kernel']),
                                          torch_us=best(t['torch']), kernel_over_torch=best(t['kernel']) / best(t['torch']),
                                          runs=t))
            del la
        la = fork.Lookahead(env, ship=0, horizon=h)
        same = bool(torch.equal(la.controls(), torch_tick(la)))
        t = alternating(dict(kernel=la.controls, torch=lambda: torch_tick(la)), P, R, W, max(C // 4, 2))
        res['tick'].append(dict(horizon=h, scratch_envs=la.scratch.n_env, same_controls=same, kernel_us=best(t['kernel']),
                                torch_us=best(t['torch']), kernel_over_torch=best(t['kernel']) / best(t['torch']), runs=t))
    env.check_errors()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
