#!/usr/bin/env python3
"""Train a Q-network with astro_amd.train.QTrainer on a fixed budget of ticks
and record how it plays: every --every ticks the greedy network plays --games
games per evaluation env as ship 0 against NothingBot and against ScriptBot
(QTrainer.validate: env.play_q and Episodes.summary), as rl.train validates
every `interval` games (rl.py:352-369).

Training is self-play as in the reference: the network decides for both ships
of every env, with the reference's sticky exploration (EpsilonGreedy(1.0, 0.1),
one seed) and its learner constants (n_steps 100, discount 0.995, 1,024 samples
per step, SGD with lr 1e-2).  The evaluation envs are re-created with the same
seeds before every validation, so every point of the curve plays the same
games.  --optimizer, --target-sync, --double, --opponent, --max-norm and
--weight-decay select QTrainer's options (astro_amd.optim); without them the
run is the one described above.  --opponent snapshot --opponent-sync K trains
against a frozen copy of the network, refreshed every K optimisation steps;
--opponent pool --pool-size M against M such copies of different ages, each
playing ship 1 of a block of the envs, the oldest refreshed every K steps.
--tournament M adds league.tournament over M of the validations' networks.  The
settings are part of the arguments the curve file records.  --log-dir DIR saves
the validation games against ScriptBot of the first --log-envs evaluation envs,
recorded on the device with the network's Q values (astro_amd.record), as
DIR/<tick>/<env>_<k>.log in the reference's log format -- what rl.train saves
at each validation (rl.py:354-355), for the reference's viewer.

Writes one JSON document to --out: the arguments, and per validation the tick,
the optimisation steps so far, the last loss per sample, both summaries and,
after tick 0, the network against its copy from the previous validation and
against the tick-0 network (league.compare: both seats, wins and p_better).  No
result is expected of it: it reports what the budget gave.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from astro_amd import (BatchedEnv, DEFAULT_CONFIG, ReplayBuffer, actor, league, optim, qnet, record,  # noqa: E402
                       train)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n-env', type=int, default=4096)
    ap.add_argument('--ticks', type=int, default=20000)
    ap.add_argument('--every', type=int, default=2500)
    ap.add_argument('--eval-envs', type=int, default=1024)
    ap.add_argument('--games', type=int, default=1)
    ap.add_argument('--max-time', type=float, default=20.0, help='max_time of the evaluation games, seconds')
    ap.add_argument('--n-steps', type=int, default=100)
    ap.add_argument('--ring', type=int, default=128)
    ap.add_argument('--n-samples', type=int, default=1024)
    ap.add_argument('--lr', type=float, default=1e-2)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=os.path.join('profiles', 'actor', 'learning_curve.json'))
    ap.add_argument('--optimizer', choices=('sgd', 'momentum', 'rmsprop', 'adagrad', 'adam'), default='sgd',
                    help='sgd with no other option: QNetwork.sgd_step, as before; otherwise an astro_amd.optim rule '
                         '(momentum: SGD with momentum 0.9) at --lr')
    ap.add_argument('--target-sync', default=None,
                    help='an integer K: a target network hard-copied every K steps; a float in (0, 1): Polyak tau')
    ap.add_argument('--double', action='store_true', help='Double-DQN targets')
    ap.add_argument('--opponent', choices=('script', 'nothing', 'random', 'snapshot', 'pool'), default=None,
                    help='ship 1 of the training envs plays this bot instead of the network; snapshot: a frozen copy '
                         'of the network, refreshed every --opponent-sync optimisation steps; pool: --pool-size such '
                         'copies, each playing a block of the envs, the oldest refreshed every --opponent-sync steps')
    ap.add_argument('--opponent-sync', type=int, default=None,
                    help='with --opponent snapshot / pool: steps between refreshes')
    ap.add_argument('--pool-size', type=int, default=None, help='with --opponent pool: the number of frozen copies')
    ap.add_argument('--ladder', default=None,
                    help="a fixed ladder of scripted rivals instead of --opponent: comma-separated rungs, each 'nothing', "
                         "'random', 'script' or DISTANCE:THRESHOLD (a ScriptBot with those avoid_distance / "
                         "avoid_threshold), e.g. nothing,0.0:1.5,0.05:0.9,script; ship 1 of block j of the envs plays "
                         "rung j (league.Seats.versus), and every validation also plays each rung")
    ap.add_argument('--tournament', type=int, default=0,
                    help='M in 2..6: after the run, league.tournament over M of the validations\' networks (evenly '
                         'spaced, first and last included) on a fresh evaluation env; recorded as "tournament"')
    ap.add_argument('--max-norm', type=float, default=None, help='clip the gradient norm to this')
    ap.add_argument('--weight-decay', type=float, default=0.0)
    ap.add_argument('--log-dir', default=None,
                    help='save the recorded validation games against ScriptBot as DIR/<tick>/<env>_<k>.log')
    ap.add_argument('--log-envs', type=int, default=4, help='with --log-dir: the evaluation envs 0 .. n-1 are recorded')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'train_q needs a HIP device'
    dev = 'cuda:0'
    torch.manual_seed(args.seed)
    env = BatchedEnv(DEFAULT_CONFIG, args.n_env, device=dev, b_cap=32)
    env.reset()
    net = qnet.QNetwork.from_module(qnet.ValueNetwork(solo=False), dev)
    buf = ReplayBuffer(env.n_env, env.p_pad + env.b_cap, 2, args.ring, n_steps=args.n_steps, device=dev)
    eg = actor.EpsilonGreedy(env, t_in=1.0, t_out=0.1, seed=args.seed)
    sync = args.target_sync
    if sync is not None:
        sync = int(sync) if sync.lstrip('+').isdigit() else float(sync)
    opt = None      # the defaults: sgd_step, today's run
    if args.optimizer != 'sgd' or sync is not None or args.max_norm is not None or args.weight_decay:
        common = dict(lr=args.lr, weight_decay=args.weight_decay, max_norm=args.max_norm)
        opt = {'sgd': lambda: optim.SGD(**common), 'momentum': lambda: optim.SGD(momentum=0.9, **common),
               'rmsprop': lambda: optim.RMSprop(**common), 'adagrad': lambda: optim.Adagrad(**common),
               'adam': lambda: optim.Adam(**common)}[args.optimizer]()
    ladder = None
    if args.ladder:
        assert args.opponent is None, '--ladder goes without --opponent'
        ladder = [r if ':' not in r else league.Script(*map(float, r.split(':'))) for r in args.ladder.split(',')]
    tr = train.QTrainer(env, net, buf, eg, n_samples=args.n_samples, lr=args.lr, seed=args.seed, optimizer=opt,
                        target_sync=sync, double=args.double, opponent=ladder or args.opponent,
                        opponent_sync=args.opponent_sync,
                        pool_size=args.pool_size)
    checkpoints = []                               # (tick, the network then), one per validation
    eval_cfg = DEFAULT_CONFIG._replace(max_time=args.max_time)
    curve = []
    t0 = time.time()
    first, previous = net.clone(), net.clone()     # the network at tick 0 and at the validation before this one

    def against(other):
        ev = BatchedEnv(eval_cfg, args.eval_envs, device=dev, b_cap=32, env_offset=1 << 20)
        ev.reset()
        return league.compare(ev, net, other, games=args.games)

    def validate(tick):
        point = dict(tick=tick, nstep=tr.nstep, seconds=round(time.time() - t0, 2),
                     loss_per_sample=None if tr.last is None else float(tr.last['loss']) / int(tr.last['n']),
                     finite=bool(torch.isfinite(net.weights).all()))
        if opt is not None and opt.norm is not None:
            point.update(grad_norm=float(opt.norm), skipped=int(opt.skipped))
        for opponent in ('nothing', 'script'):
            ev = BatchedEnv(eval_cfg, args.eval_envs, device=dev, b_cap=32, env_offset=1 << 20)
            ev.reset()
            rec = None
            if args.log_dir and opponent == 'script':
                rec = record.Recorder(ev, range(min(args.log_envs, args.eval_envs)), q=True, limit=args.games)
            point[opponent] = tr.validate(ev, games=args.games, opponent=opponent, record=rec)
            if rec is not None:
                point['logs'] = len(rec.save(os.path.join(args.log_dir, str(tick))))
        if ladder:   # every rung, in blocks of one evaluation batch
            ev = BatchedEnv(eval_cfg, args.eval_envs, device=dev, b_cap=32, env_offset=1 << 20)
            ev.reset()
            w = ev.play_q(league.Seats.versus(ev, net, ladder), games=args.games)[0]
            K, N = len(ladder), args.eval_envs
            point['ladder'] = [dict(rung=args.ladder.split(',')[j],
                                    won=float((w[j * N // K:(j + 1) * N // K] == 0).float().mean()),
                                    lost=float((w[j * N // K:(j + 1) * N // K] == 1).float().mean()))
                               for j in range(K)]
        if tick:
            point['vs_previous'], point['vs_first'] = against(previous), against(first)
            previous.copy_from(net)
        if args.tournament:
            checkpoints.append((tick, net.clone()))
        curve.append(point)
        print(json.dumps(point), flush=True)

    validate(0)
    for tick in range(args.every, args.ticks + 1, args.every):
        tr.run(args.every)
        validate(tick)
    env.check_errors()
    doc = dict(args=vars(args), device=torch.cuda.get_device_name(0), train_seconds=round(time.time() - t0, 2),
               curve=curve)
    if args.tournament:
        M = min(args.tournament, len(checkpoints))
        picked = [checkpoints[round(k * (len(checkpoints) - 1) / (M - 1))] for k in range(M)]
        ev = BatchedEnv(eval_cfg, args.eval_envs, device=dev, b_cap=32, env_offset=1 << 20)
        ev.reset()
        doc['tournament'] = dict(ticks=[t for t, _ in picked],
                                 **league.tournament(ev, [n for _, n in picked], games=args.games))
        ev.check_errors()
        print(json.dumps(doc['tournament']), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
