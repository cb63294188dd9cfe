#!/usr/bin/env python3
"""Throughput of the first-person renderer (libigw_render.so) on one MI355X; prints one JSON line (and writes it to
--out).  Timings are HIP-event windows after warm-up:

  render   N envs x 64 x 64 RGB, one igw_render_pov launch per frame batch: us per launch, frames / s, and the
           write bound (N*H*W*C bytes over the 8 TB/s HBM peak and over the 6.29 TB/s a streaming kernel reaches)
  step     at 65,536 envs: walking step alone vs step + render (what VecGridWorld(renderer='hip') costs per step)
  facade   the 1-env gym facade: step without pov vs with pov (host wall clock, each step ends in a synchronise)

    python tools/bench_render.py [--envs 1,4096,65536,524288] [--iters 50] [--out profiles/r07_render_bench.json]

The VALU side of the kernel comes from a separate profiler run ("First-person frames": measured numbers).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK, HBM_STREAM = 8.0e12, 6.29e12   # B/s: MI355X spec, and the guide's measured streaming write/read rate


def _batch(n, seed=1):
    from gridworld_amd import VecGridWorld, workloads
    env = VecGridWorld(n)
    rng = np.random.RandomState(seed)
    pose = np.stack([rng.uniform(-8, 8, n), rng.uniform(0, 4, n), rng.uniform(-8, 8, n), rng.uniform(-180, 180, n),
                     rng.uniform(-60, 60, n)], 1)
    starts = workloads.uniform20(n, seed=seed).numpy()
    env.set_tasks(workloads.rt20(n, seed=seed).numpy(), starts, init_pose=pose)
    env.reset()
    return env


def _time(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters   # us per call


def bench_render(n, iters, warmup, W=64, H=64, C=3):
    env = _batch(n)
    out = torch.empty((n, H, W, C), dtype=torch.uint8, device='cuda')
    us = _time(lambda: env.render_pov(out=out, channels=C), iters, warmup)
    nbytes = n * H * W * C
    res = {'envs': n, 'size': [W, H], 'channels': C, 'us_per_launch': round(us, 2),
           'frames_per_s': round(n / (us * 1e-6), 1), 'bytes_written': nbytes,
           'write_bound_us_spec': round(nbytes / HBM_PEAK * 1e6, 2),
           'write_bound_us_measured_rate': round(nbytes / HBM_STREAM * 1e6, 2),
           'achieved_write_TBps': round(nbytes / (us * 1e-6) / 1e12, 3)}
    del env, out
    torch.cuda.empty_cache()
    return res


def bench_step(n, iters, warmup):
    env = _batch(n)
    acts = env.fill_actions(iters + warmup, seed=3)
    out = torch.empty((n, 64, 64, 3), dtype=torch.uint8, device='cuda')
    k = [0]

    def step():
        env.step_walking_ptr(acts[k[0] % acts.shape[0]])
        k[0] += 1

    def step_render():
        step()
        env.render_pov(out=out)
    a = _time(step, iters, warmup)
    b = _time(step_render, iters, warmup)
    return {'envs': n, 'step_us': round(a, 2), 'step_plus_render_us': round(b, 2),
            'render_share_of_step_plus_render': round((b - a) / b, 3)}


def bench_facade(steps):
    import gridworld_amd as G
    res = {}
    for name, kw in (('no_pov', dict(render=False, vector_state=True)), ('pov', dict(renderer='hip'))):
        env = G.make('IGLUGridworld-v0', **kw)
        env.set_task(G.Task('chat', G.workloads.rt20(1, 3)[0].numpy().astype(np.int32)))
        env.reset()
        for t in range(20):
            env.step(t % 18)
        t0 = time.perf_counter()
        for t in range(steps):
            env.step(t % 18)
        res[name + '_us_per_step'] = round((time.perf_counter() - t0) / steps * 1e6, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', default='1,4096,65536,524288')
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--facade-steps', type=int, default=500)
    ap.add_argument('--skip', default='', help='comma list of parts to skip: step, facade')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_render.py needs a GPU')
    from gridworld_amd import render as R, build as B
    skip = set(filter(None, a.skip.split(',')))
    line = {'tool': 'tools/bench_render.py', 'render_build_id': R.build_id(), 'step_build_id': B.source_hash(),
            'device': torch.cuda.get_device_name(0), 'render': []}
    for n in [int(v) for v in a.envs.split(',')]:
        try:
            line['render'].append(bench_render(n, a.iters, a.warmup))
        except torch.cuda.OutOfMemoryError as e:
            line['render'].append({'envs': n, 'skipped': 'out of memory: %s' % str(e)[:80]})
    if 'step' not in skip:
        line['step'] = bench_step(65536, a.iters, a.warmup)
    if 'facade' not in skip:
        line['facade'] = bench_facade(a.facade_steps)
    s = json.dumps(line)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(s + '\n')


if __name__ == '__main__':
    main()
