#!/usr/bin/env python3
"""Time the device replay buffer (astro_amd.replay.ReplayBuffer: astro_replay_push
/ sample / gather / update) against its torch equivalents on the c3 workload.

Workload: bench.py's c3 -- 65,536 envs of 3-planet games, b_cap 32, float32
state, rows = p_pad + b_cap = 36, two ships -- with the reference's n_steps 100
and discount 0.995 and a ring of n_steps + 2 = 102 rows (13.4 M experience
ids, 14.4 GB of features), filled by --warm-ticks of rollout and then 110 ticks
of features(out=head) / controls('random') / step / push.  Every stored loss is
then set to an exponential variate, except 16,384 random ids left unscored.

Timed as tools/bench_qtrain.py does (HIP events around --reps windows of
--calls back-to-back calls; median, min and 90th percentile per call):

  push         buf.push(control, reward, done)
  sample       buf.sample(n) for n = 65,536 and 1,024, against
               torch.topk(keys, n, largest=False) + sort on keys of the same
               distribution (an exponential variate over the loss, generated
               by torch: `topk` alone and with the key generation), and
               torch.multinomial(loss, n, replacement=False) + sort (13.4 M
               categories are within its 2^24 limit)
  gather       buf.gather(ids) against advanced indexing plus swap_ego
  update_loss  buf.update_loss(ids, loss) against an indexed assignment
  step         one whole replay training step (sample, gather, td_targets,
               sgd_step, update_loss) next to net.grad alone on the same batch

Prints one JSON line (and writes it to --out): the times, the ratios to the
torch paths, and the replay operations' share of a training step.  Needs a HIP
device with about 20 GB free.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from astro_amd import BatchedEnv, DEFAULT_CONFIG, ReplayBuffer, qnet  # noqa: E402


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


def torch_gather(buf, ids):
    """buf.gather with torch indexing: the same six tensors (every column copied)."""
    N, S = buf.n_env, buf.nships
    flat = buf.features.view(-1, buf.rows, buf.nf)
    idx = ids.long()
    re, ship1 = idx // S, (idx % S == 1)[:, None, None]
    nxt = buf.next.view(-1)[re].long()
    f = flat[re]
    nf = flat[nxt.clamp(min=0) * N + re % N]
    if S == 2:
        f = torch.where(ship1, qnet.swap_ego(f), f)
        nf = torch.where(ship1, qnet.swap_ego(nf), nf)
    return (f, buf.action.view(-1)[idx], buf.reward.view(-1)[idx], buf.discount.view(-1)[re], nf,
            (nxt == -1).to(torch.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n-env', type=int, default=65536)
    ap.add_argument('--n-steps', type=int, default=100)
    ap.add_argument('--large', type=int, default=65536)
    ap.add_argument('--small', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--warm-ticks', type=int, default=100)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_replay needs a HIP device'
    dev = 'cuda:0'
    N = args.n_env
    env = BatchedEnv(DEFAULT_CONFIG, N, device=dev, b_cap=32, p_pad=4, planets_only=3, auto_reset=True)
    env.reset()
    env.rollout(args.warm_ticks, 'random')
    rows, ticks = env.p_pad + env.b_cap, args.n_steps + 2
    buf = ReplayBuffer(N, rows, 2, ticks, n_steps=args.n_steps, device=dev)
    for t in range(ticks + 8):
        env.features(out=buf.head())
        control = env.controls('random', seed=1, tick0=t)
        _, reward, done = env.step(control)
        buf.push(control, reward, done)
    torch.manual_seed(7)
    m = buf.loss.numel()
    buf.loss.view(-1).exponential_()
    buf.loss.view(-1)[torch.randperm(m, device=dev)[:16384]] = float('inf')
    module = qnet.ValueNetwork(False, 6)
    with torch.no_grad():
        for p in module.parameters():
            p.mul_(3.0)
    net = qnet.QNetwork.from_module(module, dev)
    res = dict(workload='c3', n_env=N, rows=rows, ticks=ticks, n_steps=args.n_steps, ids=m,
               eligible_lower_bound=buf.eligible_lower_bound(), device=torch.cuda.get_device_name(0))
    R, W, C = args.reps, args.warmup, args.calls
    draw = [0]

    for name, n in (('large', args.large), ('small', args.small)):
        out = dict(n=n)
        ids = torch.empty(n, dtype=torch.int32, device=dev)

        def sample():
            draw[0] += 1
            buf.sample(n, seed=3, draw=draw[0], out=ids)

        keys = torch.empty(m, device=dev)
        flat_loss = buf.loss.view(-1)

        def make_keys():
            keys.exponential_().div_(flat_loss)

        def topk():
            return torch.topk(keys, n, largest=False, sorted=False)[1].sort()[0]

        def keys_topk():
            make_keys()
            return topk()

        weights = torch.where(torch.isinf(flat_loss), torch.zeros_like(flat_loss), flat_loss)

        def multinomial():
            return torch.multinomial(weights, n, replacement=False).sort()[0]

        out['sample'] = timed(sample, R, W, C)
        make_keys()
        out['torch_topk'] = timed(topk, R, W, C)
        out['torch_keys_topk'] = timed(keys_topk, R, W, C)
        if m <= 2 ** 24:
            out['torch_multinomial'] = timed(multinomial, max(3, R // 4), 1, 1)
        out['sample_again'] = timed(sample, R, 1, C)
        assert buf.last_count() == n
        sample()
        vals = torch.rand(n, device=dev) + 0.01
        outs = buf.gather(ids)

        def gather():
            buf.gather(ids, out=outs)

        def t_gather():
            return torch_gather(buf, ids)

        out['gather'] = timed(gather, R, W, C)
        out['torch_gather'] = timed(t_gather, R, W, C)
        ref = t_gather()
        live = ~(ref[0][:, :, :1] < 0)
        out['gather_equals_torch'] = bool(
            all(torch.equal(outs[k], ref[k]) for k in (1, 2, 3, 5))
            and torch.equal(outs[0][:, :, 0], ref[0][:, :, 0])
            and torch.equal(torch.where(live, outs[0], 0.0), torch.where(live, ref[0], 0.0)))
        out['live_row_fraction'] = float(live.float().mean())

        def update():
            buf.update_loss(ids, vals)

        def t_update():
            flat_loss[ids.long()] = vals

        out['update_loss'] = timed(update, R, W, C)
        out['torch_update'] = timed(t_update, R, W, C)

        f, a, r, d, nf, term = outs
        target = net.td_targets(r, d, nf, term)
        lbuf, gbuf = torch.empty(n, device=dev), torch.empty_like(net.weights)

        def grad():
            net.grad(f, a, target, loss_out=lbuf, grad_out=gbuf)

        def step():
            sample()
            o = buf.gather(ids, out=outs)
            loss = net.sgd_step(o[0], o[1], net.td_targets(o[2], o[3], o[4], o[5]), lr=1e-4)
            buf.update_loss(ids, loss)

        out['grad'] = timed(grad, R, W, C)
        out['step'] = timed(step, R, W, C)
        replay_us = sum(out[k]['median_us'] for k in ('sample', 'gather', 'update_loss'))
        out.update(replay_us=replay_us, replay_share_of_step=replay_us / out['step']['median_us'],
                   sample_vs_grad=out['sample']['median_us'] / out['grad']['median_us'],
                   sample_speedup_vs_torch_topk=out['torch_topk']['median_us'] / out['sample']['median_us'],
                   sample_speedup_vs_torch_keys_topk=out['torch_keys_topk']['median_us'] / out['sample']['median_us'],
                   gather_speedup_vs_torch=out['torch_gather']['median_us'] / out['gather']['median_us'],
                   update_speedup_vs_torch=out['torch_update']['median_us'] / out['update_loss']['median_us'])
        if 'torch_multinomial' in out:
            out['sample_speedup_vs_torch_multinomial'] = (out['torch_multinomial']['median_us']
                                                          / out['sample']['median_us'])
        res[name] = out

    control = env.controls('random', seed=1, tick0=0)
    reward, done = env.reward.clone(), env.done.clone()
    res['push'] = timed(lambda: buf.push(control, reward, done), R, W, C)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
