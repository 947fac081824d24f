"""bench.py's plain run and --dump-outputs on the GPU.

A plain run (no --full) times the steps and prints the headline fields only;
--dump-outputs writes what the last timed step left a caller with.  The test
runs the benchmark twice with the same arguments (the dumps must be equal,
array for array) and replays the run's launches in this process -- reset,
burn-in rollout, settle and warmup launches, the untimed graph replays and
the timed steps, as eager BatchedEnv.step calls -- to check that the dump is
that state and not another tick's.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_ENV, STEPS, WARMUP, BURN_IN = 4096, 6, 2, 20
SECONDARY = {'roofline', 'issue_roofline', 'cpu_baseline', 'speedup_vs_cpu', 'rollout', 'rollout_script',
             'observation', 'single_game', 'stats', 'gpu_ms_per_step', 'region_host_us'}


def _bench(out_dir):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(STEPS), '--warmup',
           str(WARMUP), '--burn-in', str(BURN_IN), '--n-env', str(N_ENV), '--warm-ms', '0.2', '--graph', '4',
           '--dump-outputs', str(out_dir)]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip().startswith('{')]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


@pytest.mark.gpu
def test_plain_run_headline_and_reproducible_dump(tmp_path):
    import torch
    import bench
    from astro_amd import BatchedEnv, DEFAULT_CONFIG

    j, a = _bench(tmp_path / 'a')
    _, b = _bench(tmp_path / 'b')

    assert j['steps'] == STEPS and j['warmup'] == WARMUP and j['full'] is False and j['device_errors'] == 0
    assert j['value'] > 0 and j['unit'] == 'env-steps/s' and j['higher_is_better'] is True
    assert abs(j['value'] - N_ENV * STEPS / (j['ms_per_step'] * 1e-3 * STEPS)) <= 1e-6 * j['value']
    assert j['metric'] == bench.METRIC and j['dtype'] == 'f64 math / f32 state'
    assert not SECONDARY & set(j)
    # two graphs (4 + 2 launches); 0.2 ms of warm replays at the nominal 10 us per launch
    assert j['warm_rounds'] == 4 and '4+2' in j['timed_region']

    assert set(a) == set(b) == {'reward', 'done', 'env_index', 'ships', 'ships_b', 'planets', 'bullets', 'tick',
                                'nplanets', 'nbullets', 'flags', 'game_seed'}
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a['env_index'], np.arange(N_ENV))

    # the same launches, eagerly, in this process
    w = bench.WORKLOADS['c3']
    env = BatchedEnv(DEFAULT_CONFIG, N_ENV, device='cuda:0', b_cap=w['b_cap'], p_pad=w['p_pad'], auto_reset=True,
                     planets_only=w['planets_only'])
    env.reset()
    env.rollout(BURN_IN, 'random', tick0=1 << 40, stats=False)
    ctl = torch.from_numpy(bench.controls(0, N_ENV, env.S, WARMUP + STEPS)).cuda()
    timed = list(range(WARMUP, WARMUP + STEPS))
    # settle, warmup, each graph's first replay, the warm rounds, the timed region
    for t in [0, 1, 2] + list(range(WARMUP)) + timed * (1 + j['warm_rounds'] + 1):
        _, rew, done = env.step(ctl[t], stats=False)
    h = env.to_host()
    assert np.array_equal(a['reward'], rew.cpu().numpy()) and np.array_equal(a['done'], done.cpu().numpy())
    # (a game re-created by the last step is at tick 0; the oldest has played every tick of the run)
    assert a['tick'].max() == BURN_IN + 3 + WARMUP + STEPS * (2 + j['warm_rounds'])
    assert np.array_equal(a['tick'], h['tick'])
    assert np.array_equal(a['nplanets'], h['nplanets']) and np.array_equal(a['nbullets'], h['nbullets'])
    assert np.array_equal(a['flags'], h['flags'])
    assert np.array_equal(a['game_seed'], env.game_seed.cpu().numpy().view(np.uint32))
    assert np.array_equal(a['ships'], h['ships']) and np.array_equal(a['ships_b'], h['ships_b'])
    pv = np.arange(h['planets'].shape[1])[None, :] < h['nplanets'][:, None]
    bv = np.arange(h['bullets'].shape[1])[None, :] < h['nbullets'][:, None]
    assert bv.any() and np.array_equal(a['bullets'][bv], h['bullets'][bv]) and not a['bullets'][~bv].any()
    assert np.array_equal(a['planets'][pv], h['planets'][pv]) and not a['planets'][~pv].any()
