#!/usr/bin/env python3
"""Evolution strategies on the packed Q-network (astro_amd.es.ESTrainer) on a
fixed budget of env ticks, and how the centre network then plays: every
--every ticks (at the next generation's end) it plays --games games per
evaluation env as ship 0 against NothingBot and against ScriptBot, greedy, as
tools/train_q.py and tools/train_distill.py validate.  The evaluation envs are
re-created with the same seeds before every validation.

Two arms, one seed each (--seed), the same envs, budget and validation:

  script    the members play ScriptBot
  nothing   the members play NothingBot

The budget is DESIGN.md section 17's: --ticks (40,000) ticks of --n-env
(4,096) envs.  A tick here is one ``env.step`` of the training env, counted
around the trainer (a generation plays until every env has finished its
games, in windows of 64 ticks, so generations differ in length).  The training
games are cut at --train-max-time seconds so that one slow game does not hold
a generation up for 3,000 ticks.

Writes one JSON document to --out: the arguments, one curve per arm and, next
to them, the last points of profiles/actor/learning_curve.json and
profiles/search/distill_curve.json if those files exist.  No result is
expected of it: it reports what the budget gave, "it did not move" included.
One seed ranks nothing.  ``flat_generations`` counts the generations in which
every member had the same fitness: the estimate is then exactly zero;
``moved_l2`` is how far the centre is from where it began, and
``first_controls`` counts the controls 0..5 that the greedy centre picks in the
evaluation envs' first states.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

from astro_amd import BatchedEnv, DEFAULT_CONFIG, es, optim, qnet  # noqa: E402


def baselines():
    out = {}
    path = os.path.join(ROOT, 'profiles', 'actor', 'learning_curve.json')
    if os.path.exists(path):
        d = json.load(open(path))
        out['qtrainer_section17 (profiles/actor/learning_curve.json)'] = dict(first=d['curve'][0], last=d['curve'][-1])
    path = os.path.join(ROOT, 'profiles', 'search', 'distill_curve.json')
    if os.path.exists(path):
        d = json.load(open(path))
        for arm, v in d['arms'].items():
            out['%s (profiles/search/distill_curve.json)' % arm] = dict(first=v['curve'][0], last=v['curve'][-1])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n-env', type=int, default=4096)
    ap.add_argument('--ticks', type=int, default=40000)
    ap.add_argument('--every', type=int, default=5000)
    ap.add_argument('--eval-envs', type=int, default=1024)
    ap.add_argument('--games', type=int, default=1)
    ap.add_argument('--max-time', type=float, default=20.0, help='max_time of the evaluation games, seconds')
    ap.add_argument('--train-max-time', type=float, default=10.0, help='max_time of the training games, seconds')
    ap.add_argument('--pairs', type=int, default=16)
    ap.add_argument('--rounds', type=int, default=1)
    ap.add_argument('--sigma', type=float, default=0.05)
    ap.add_argument('--lr', type=float, default=1e-2)
    ap.add_argument('--optimizer', choices=['adam', 'sgd'], default='adam')
    ap.add_argument('--shaping', choices=['ranks', 'raw'], default='ranks')
    ap.add_argument('--draw', type=float, default=0.5)
    ap.add_argument('--survive', type=float, default=0.5)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--arms', nargs='*', default=['script', 'nothing'])
    ap.add_argument('--out', default=os.path.join('profiles', 'es', 'es_curve.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'train_es needs a HIP device'
    dev = 'cuda:0'
    train_cfg = DEFAULT_CONFIG._replace(max_time=args.train_max_time)
    eval_cfg = DEFAULT_CONFIG._replace(max_time=args.max_time)
    doc = dict(args=vars(args), device=torch.cuda.get_device_name(0), seeds=1, arms={}, compared_with=baselines())
    for arm in args.arms:
        torch.manual_seed(args.seed)
        env = BatchedEnv(train_cfg, args.n_env, device=dev, b_cap=32, auto_reset=True)
        env.reset()
        net = qnet.QNetwork.from_module(qnet.ValueNetwork(solo=False), dev)
        opt = optim.Adam(lr=args.lr) if args.optimizer == 'adam' else optim.SGD(args.lr)
        tr = es.ESTrainer(env, net, opponent=arm, pairs=args.pairs, rounds=args.rounds, sigma=args.sigma, optimizer=opt,
                          games=1, shaping=args.shaping, draw=args.draw, survive=args.survive, seed=args.seed)
        ticks = [0]
        step = env.step

        def counted(*a, **kw):
            ticks[0] += 1
            return step(*a, **kw)
        env.step = counted
        theta0 = net.weights.clone()
        curve, t0, flat = [], time.time(), [0]    # flat: generations whose members all had one fitness (no gradient)

        def validate():
            point = dict(tick=ticks[0], generation=tr.ngen, seconds=round(time.time() - t0, 2),
                         mean_fitness=None if tr.last is None else float(tr.last),
                         best_fitness=None if tr.last is None else float(tr.fitness.max()),
                         flat_generations=flat[0],
                         moved_l2=float((net.weights - theta0).norm()), theta0_l2=float(theta0.norm()),
                         finite=bool(torch.isfinite(net.weights).all()))
            for opponent in ('nothing', 'script'):
                ev = BatchedEnv(eval_cfg, args.eval_envs, device=dev, b_cap=32, env_offset=1 << 20)
                ev.reset()
                if opponent == 'nothing':   # what the greedy centre plays in the evaluation envs' first states
                    first = ev.qcontrols((net, None))[:, 0].to(torch.int64)
                    point['first_controls'] = torch.bincount(first, minlength=6).cpu().tolist()
                point[opponent] = tr.validate(ev, games=args.games, opponent=opponent)
            curve.append(point)
            print(json.dumps(dict(arm=arm, **point)), flush=True)

        validate()
        due = args.every
        while ticks[0] < args.ticks:
            tr.generation()
            flat[0] += int(torch.unique(tr.fitness).numel() == 1)
            if ticks[0] >= due or ticks[0] >= args.ticks:
                validate()
                due += args.every * max(1, (ticks[0] - due) // args.every + 1)
        env.check_errors()
        doc['arms'][arm] = dict(train_seconds=round(time.time() - t0, 2), generations=tr.ngen, ticks=ticks[0], curve=curve)
        del tr, env
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
