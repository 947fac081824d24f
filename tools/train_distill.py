#!/usr/bin/env python3
"""Train a Q-network on a search's values (astro_amd.train.Distiller) on a fixed
budget of ticks and record how the GREEDY network -- without any search --
plays: every --every ticks it plays --games games per evaluation env as ship 0
against NothingBot and against ScriptBot, as tools/train_q.py validates.  The
evaluation envs are re-created with the same seeds before every validation.

Three arms, one seed each (--seed), the same envs, tick budget and validation:

  teacher64   a horizon-64 ScriptBot ``fork.Lookahead`` without a leaf teaches
  expert16    horizon 16 with ``leaf_sync``: the teacher's leaf is the student,
              hard-copied every --leaf-sync steps (expert iteration)
  qtrainer    the baseline: ``QTrainer`` in the setting of DESIGN.md section 17
              that did best against ScriptBot (Adam lr 1e-3, a target network
              hard-copied every 1,000 steps, Double-DQN targets, self-play with
              sticky exploration)

The two distillation arms train with Adam at --lr on all 6 x n_env targets of
every tick, ship 1 of the training envs played by ScriptBot.  Writes one JSON
document to --out: the arguments and one curve per arm.  No result is expected
of it: it reports what the budget gave.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from astro_amd import BatchedEnv, DEFAULT_CONFIG, ReplayBuffer, actor, fork, optim, qnet, train  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n-env', type=int, default=1024)
    ap.add_argument('--ticks', type=int, default=20000)
    ap.add_argument('--every', type=int, default=2500)
    ap.add_argument('--eval-envs', type=int, default=1024)
    ap.add_argument('--games', type=int, default=1)
    ap.add_argument('--max-time', type=float, default=20.0, help='max_time of the evaluation games, seconds')
    ap.add_argument('--lr', type=float, default=1e-3)
    ap.add_argument('--leaf-sync', type=int, default=500)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--arms', nargs='*', default=['teacher64', 'expert16', 'qtrainer'])
    ap.add_argument('--out', default=os.path.join('profiles', 'search', 'distill_curve.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'train_distill needs a HIP device'
    dev = 'cuda:0'
    eval_cfg = DEFAULT_CONFIG._replace(max_time=args.max_time)
    doc = dict(args=vars(args), device=torch.cuda.get_device_name(0), seeds=1, arms={})
    for arm in args.arms:
        torch.manual_seed(args.seed)
        env = BatchedEnv(DEFAULT_CONFIG, args.n_env, device=dev, b_cap=32)
        env.reset()
        net = qnet.QNetwork.from_module(qnet.ValueNetwork(solo=False), dev)
        if arm == 'qtrainer':
            buf = ReplayBuffer(env.n_env, env.p_pad + env.b_cap, 2, 128, n_steps=100, device=dev)
            eg = actor.EpsilonGreedy(env, t_in=1.0, t_out=0.1, seed=args.seed)
            tr = train.QTrainer(env, net, buf, eg, n_samples=1024, seed=args.seed, optimizer=optim.Adam(lr=1e-3),
                                target_sync=1000, double=True)
        else:
            teacher = fork.Lookahead(env, ship=0, horizon=64 if arm == 'teacher64' else 16)
            tr = train.Distiller(env, net, teacher, optimizer=optim.Adam(lr=args.lr), opponent='script',
                                 leaf_sync=args.leaf_sync if arm == 'expert16' else 0, seed=args.seed)
        curve, t0 = [], time.time()

        def validate(tick):
            last = tr.last
            if isinstance(last, dict):
                last = float(last['loss']) / int(last['n'])
            point = dict(tick=tick, nstep=tr.nstep, seconds=round(time.time() - t0, 2),
                         loss_per_sample=None if last is None else float(last),
                         finite=bool(torch.isfinite(net.weights).all()))
            for opponent in ('nothing', 'script'):
                ev = BatchedEnv(eval_cfg, args.eval_envs, device=dev, b_cap=32, env_offset=1 << 20)
                ev.reset()
                point[opponent] = tr.validate(ev, games=args.games, opponent=opponent)
            curve.append(point)
            print(json.dumps(dict(arm=arm, **point)), flush=True)

        validate(0)
        for tick in range(args.every, args.ticks + 1, args.every):
            tr.run(args.every)
            validate(tick)
        env.check_errors()
        doc['arms'][arm] = dict(train_seconds=round(time.time() - t0, 2), curve=curve)
        del tr, env
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
