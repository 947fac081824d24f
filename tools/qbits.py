#!/usr/bin/env python3
"""Do astro_qvalues, astro_qvalues_ships and astro_qvalues_pool of this tree give,
bit for bit, what another build of the three libraries gives?

    ASTRO_QNET_LIB=... ASTRO_QDUEL_LIB=... ASTRO_QPOOL_LIB=... python tools/qbits.py [--out FILE]

The three variables name the other build (astro_amd/_lib.py reads them).  A fresh
child process per build -- the other one with the variables, the tree's without
-- evaluates the same seeded cases and writes every q and control to a file; the
two files are then compared byte for byte.  Cases: 1 and 2 ships, float32 and
float64 state, n_env 1, 31, 33 and 130 (p_pad 4, b_cap 32, aged by 60 ticks of
random rollout), nout 6 and 3, epsilon 0 and 0.3; astro_qvalues; astro_qvalues_ships
for both ships and for ship 1 alone, and astro_qvalues_pool with two networks over
the spans [0, 17) and [17, 130) of ship 0 and [5, 70) of ship 1 (cut at n_env),
each with max_blocks 0 and 1.  Exit status 1 if a byte differs.  Needs a HIP device.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

NAMES = ('ASTRO_QNET_LIB', 'ASTRO_QDUEL_LIB', 'ASTRO_QPOOL_LIB')
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def evaluate(path):
    """Every case's q and control, appended to `path`; `path`.json: [[case, first byte], ...]."""
    import torch
    from astro_amd import BatchedEnv, DEFAULT_CONFIG, SOLO_CONFIG, _lib, league, qnet
    dev, index = 'cuda:0', []

    def network(S, nout, seed):
        torch.manual_seed(100 * S + 10 * nout + seed)
        module = qnet.ValueNetwork(S == 1, nout)
        with torch.no_grad():
            for p in module.parameters():
                p.mul_(3.0)
        return qnet.QNetwork.from_module(module, dev)

    with open(path, 'wb') as f:
        shapes = ((S, d, n) for S in (1, 2) for d in (torch.float32, torch.float64) for n in (1, 31, 33, 130))
        for S, dtype, n in shapes:
            cfg = SOLO_CONFIG if S == 1 else DEFAULT_CONFIG
            env = BatchedEnv(cfg, n, device=dev, b_cap=32, p_pad=4, dtype=dtype)
            env.reset()
            env.rollout(60, 'random', seed=n)
            for nout, eps in ((o, e) for o in (6, 3) for e in (0.0, 0.3)):
                A, B = network(S, nout, 0), network(S, nout, 1)
                coin = env.policy('random', 9, 4) if eps else None
                spans = [(0, 0, min(17, n), 0), (0, min(17, n), n, 1)]
                spans += [(1, min(5, n), min(70, n), 0)] if S == 2 else []
                pool = league.Pool(env, [A, B], spans)
                calls = [('qvalues', lambda q, c: env._qvalues(A, q, c, coin, eps))]
                for mb in (0, 1):
                    forms = [('both', (A, B)[:S])] + ([('ship1', (None, B))] if S == 2 else [])
                    calls += [('ships %s mb%d' % (name, mb), lambda q, c, nets=env._per_ship(nets), mb=mb:
                               env._qvalues_ships(nets, q, c, coin, eps, max_blocks=mb)) for name, nets in forms]
                    calls.append(('pool mb%d' % mb, lambda q, c, mb=mb:
                                  env._qvalues_pool(pool, q, c, coin, eps, max_blocks=mb)))
                for name, call in calls:
                    q = torch.zeros((n, S, nout), dtype=torch.float32, device=dev)
                    c = torch.zeros((n, S), dtype=torch.int8, device=dev)
                    call(q, c)
                    index.append(['S%d %s n%d nout%d eps%g %s' % (S, str(dtype)[6:], n, nout, eps, name), f.tell()])
                    f.write(q.cpu().numpy().tobytes() + c.cpu().numpy().tobytes())
            env.check_errors()
    libs = [_lib.QNET_LIB_PATH, _lib.QDUEL_LIB_PATH, _lib.QPOOL_LIB_PATH]   # what this process loaded
    json.dump(dict(libs=libs, index=index), open(path + '.json', 'w'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', default='', help='(internal) evaluate the cases into this file')
    ap.add_argument('--out', default='')
    ap.add_argument('--timeout', type=int, default=300, help="a child's time limit, seconds")
    args = ap.parse_args()
    if args.child:
        return evaluate(args.child)
    assert all(os.environ.get(k) for k in NAMES), 'set %s to the other build' % ', '.join(NAMES)
    tree = {k: v for k, v in os.environ.items() if k not in NAMES}
    with tempfile.TemporaryDirectory() as d:
        for label, env in (('other', dict(os.environ)), ('tree', tree)):   # stops at the first child that fails
            subprocess.run([sys.executable, os.path.abspath(__file__), '--child', os.path.join(d, label)], env=env,
                           check=True, timeout=args.timeout)
        a, b = (open(os.path.join(d, k), 'rb').read() for k in ('other', 'tree'))
        other, mine = (json.load(open(os.path.join(d, k + '.json'))) for k in ('other', 'tree'))
    index = mine['index']
    assert other['libs'] == [os.environ[k] for k in NAMES] and not set(mine['libs']) & set(other['libs'])
    assert index == other['index'] and len(a) == len(b) > 0
    bad = int(np.count_nonzero(np.frombuffer(a, np.uint8) != np.frombuffer(b, np.uint8)))
    lines = ['other build: ' + ' '.join(os.path.basename(os.environ[k]) for k in NAMES),
             '%d cases, %d bytes of q and control per build, %d differing bytes' % (len(index), len(a), bad)]
    ends = [first for _, first in index[1:]] + [len(a)]
    for (name, first), end in zip(index, ends):
        same = a[first:end] == b[first:end]
        lines.append('%-9s %6d bytes  %s' % ('identical' if same else 'DIFFERENT', end - first, name))
    print('\n'.join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, 'w').write('\n'.join(lines) + '\n')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
