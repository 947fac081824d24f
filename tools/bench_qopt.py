#!/usr/bin/env python3
"""Time the optimiser library (astro_amd.optim: astro_qopt_step) next to what it
replaces, and the training tick with and without QTrainer's options.

Timed as tools/bench_actor.py does (HIP events around --reps windows of --calls
back-to-back calls; median, min and 90th percentile per call), every comparison
in this one process, its sides alternating over --passes:

  apply        opt.apply(net, grad) for every kind, with and without a target
               network, on the two-ship network's 4,934 parameters
  add_         the parent's update, weights.add_(grad, alpha=-lr)
  torch_*      torch.optim.SGD / RMSprop / Adagrad / Adam stepping one 4,934-float
               parameter, in the default form and, where this torch takes the
               argument, fused=True
  step_launch  env.launch(control): the yardstick for a launch-bound call
  tick         QTrainer.tick() on the c3 workload with 1,024 samples: the
               defaults (sgd_step), SGD(1e-2) through the new path, and Adam with
               target_sync and double

Prints one JSON line (and writes it to --out).  Needs a HIP device with about
20 GB free at the default --n-env.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from astro_amd import BatchedEnv, DEFAULT_CONFIG, ReplayBuffer, actor, optim, qnet, train  # noqa: E402
from tools.bench_actor import alternating, best  # noqa: E402


def torch_rules(n, dev):
    """{name: step function} of torch.optim on one [n] parameter with a fixed gradient."""
    out = {}
    for name, cls, kw in (('sgd_momentum', torch.optim.SGD, dict(lr=1e-2, momentum=0.9)),
                          ('rmsprop', torch.optim.RMSprop, dict(lr=1e-2, eps=1e-3)),
                          ('adagrad', torch.optim.Adagrad, dict(lr=1e-2)),
                          ('adam', torch.optim.Adam, dict(lr=1e-3))):
        for form, extra in (('', {}), ('_fused', dict(fused=True))):
            p = torch.nn.Parameter(torch.randn(n, device=dev) * 0.3)
            p.grad = torch.randn(n, device=dev) * 1e-2
            try:
                o = cls([p], **kw, **extra)
                o.step()
            except (TypeError, RuntimeError, ValueError):
                continue            # this torch has no fused form of the rule
            out['torch_' + name + form] = o.step
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
    ap.add_argument('--out', default=os.path.join('profiles', 'qopt', 'bench_qopt.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_qopt needs a HIP device'
    dev = 'cuda:0'
    N = args.n_env
    R, W, C, P = args.reps, args.warmup, args.calls, args.passes
    env = BatchedEnv(DEFAULT_CONFIG, N, device=dev, b_cap=32, p_pad=4, planets_only=3, auto_reset=True)
    env.reset()
    env.rollout(args.warm_ticks, 'random')

    def network():
        module = qnet.ValueNetwork(False, 6)
        with torch.no_grad():
            for p in module.parameters():
                p.mul_(3.0)
        return qnet.QNetwork.from_module(module, dev)

    net = network()
    n = net.weights.numel()
    res = dict(workload='c3', n_env=N, nparams=n, n_samples=args.n_samples, device=torch.cuda.get_device_name(0),
               torch=torch.__version__)

    # the update rules: small gradients, so that hundreds of calls leave the weights finite
    grad = torch.randn(n, device=dev) * 1e-4
    target = net.clone()
    rules = dict(sgd=optim.SGD(1e-2), sgd_momentum=optim.SGD(1e-2, momentum=0.9), rmsprop=optim.RMSprop(),
                 adagrad=optim.Adagrad(), adam=optim.Adam(), adam_clip=optim.Adam(max_norm=1.0))
    fns = {}
    for name, o in rules.items():
        w = network()
        fns['apply_' + name] = lambda o=o, w=w: o.apply(w, grad)
    for name in ('sgd', 'adam'):
        o, w = type(rules[name])(**rules[name]._kw), network()
        fns['apply_%s_target' % name] = lambda o=o, w=w: o.apply(w, grad, target=target, tau=0.01)
    plain = network()
    fns['add_'] = lambda: plain.weights.add_(grad, alpha=-1e-2)
    fns.update(torch_rules(n, dev))
    control = env.controls('random', seed=1, tick0=0)
    cptr = control.data_ptr()
    fns['step_launch'] = lambda: env.launch(cptr, stats=False)
    res['rules'] = alternating(fns, P, R, W, C)
    res['rules_us'] = {k: best(v) for k, v in res['rules'].items()}

    # the training tick, three ways, each on a network, a ring and an exploration of its own
    rows, ticks = env.p_pad + env.b_cap, args.n_steps + 2

    def trainer(**kw):
        buf = ReplayBuffer(N, rows, 2, ticks, n_steps=args.n_steps, device=dev)
        eg = actor.EpsilonGreedy(env, seed=1)
        tr = train.QTrainer(env, network(), buf, eg, n_samples=args.n_samples, lr=1e-4, seed=3, **kw)
        tr.run(ticks + 8)
        assert tr.nstep > 0
        return tr

    trainers = dict(defaults=trainer(), sgd_optim=trainer(optimizer=optim.SGD(1e-4)),
                    adam_sync_double=trainer(optimizer=optim.Adam(1e-5), target_sync=100, double=True))
    res['tick'] = alternating({k: t.tick for k, t in trainers.items()}, P, R, W, max(1, C // 4))
    res['tick_us'] = {k: best(v) for k, v in res['tick'].items()}
    res['tick_all_medians_us'] = {k: [r['median_us'] for r in v] for k, v in res['tick'].items()}
    env.check_errors()
    res['finite'] = all(bool(torch.isfinite(t.net.weights).all()) for t in trainers.values())
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
