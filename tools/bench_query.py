#!/usr/bin/env python3
"""Cost of the action mask (igw_action_mask) on one MI355X; prints one JSON line and writes it to
--out.  Per batch size (65,536 and 2,097,152 envs of an auto-resetting rt20 batch, stepped 60 times with uniform random
actions; the task table holds 4,096 rows) four variants are measured ALTERNATELY in one process (a, b, c, d, a, b, ...
--repeats times each), every figure the median of its HIP-event windows with the min - max spread:

  mask               one igw_action_mask launch into a preallocated tensor
  mask_look_sample   the same launch with the look cells and the sampled actions
  step               env.step() alone
  today              what answers the question without the query: for each of the 8 place / break actions,
                     load_state_dict() of a saved state and one step() (the comparison of the grids is not timed)

    python tools/bench_query.py [--out profiles/r13_query_bench.json]

A profiler's kernel trace belongs in a run of its own (rocprofv3 --kernel-trace --stats -- python tools/bench_query.py
--envs 65536 --repeats 1).
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_render as BR  # noqa: E402

TASKS = 4096


def _spread(us):
    return {'us_median': round(float(np.median(us)), 2), 'us_min': round(min(us), 2), 'us_max': round(max(us), 2),
            'windows': len(us)}


def bench(n, iters, slow_iters, warmup, repeats):
    from gridworld_amd import VecGridWorld, query as Q, workloads
    env = VecGridWorld(n, autoreset=True, num_tasks=TASKS)
    env.set_tasks(workloads.rt20(TASKS, seed=1).numpy(),
                  env_task=torch.arange(n, dtype=torch.int32) % TASKS)
    env.reset()
    acts = env.fill_actions(60, seed=3)
    for t in range(60):
        env.step(acts[t])
    mask = torch.empty((n, Q.ACTIONS), dtype=torch.uint8, device=env.device)
    look = torch.empty((n, 2), dtype=torch.int16, device=env.device)
    drawn = torch.empty((n,), dtype=torch.int32, device=env.device)
    probes = [torch.full((n,), p, dtype=torch.int32, device=env.device) for p in Q.PROBES]
    saved = env.state_dict()
    state = {'t': 0}

    def step():
        env.step(acts[state['t'] % 60])
        state['t'] += 1

    def today():
        for a in probes:
            env.load_state_dict(saved)
            env.step(a)
    variants = {'mask': (lambda: env.action_mask(out=mask), iters),
                'mask_look_sample': (lambda: env.action_mask(out=(mask, look, drawn), look=True, sample=(7, state['t'])),
                                     iters),
                'step': (step, iters),
                'today': (today, slow_iters)}
    us = {k: [] for k in variants}
    for r in range(repeats):
        for k, (fn, it) in variants.items():
            us[k].append(BR._time(fn, it, warmup if r == 0 else 1))
    env.load_state_dict(saved)
    env.action_mask(out=mask)
    res = {k: _spread(v) for k, v in us.items()}
    med = lambda k: res[k]['us_median']  # noqa: E731
    res.update(envs=n, task_rows=TASKS, share_of_bits_set=round(float(mask.float().mean()), 4),
               state_dict_bytes=int(sum(v.numel() * v.element_size() for v in saved.values() if torch.is_tensor(v))),
               mask_over_step=round(med('mask') / med('step'), 3),
               mask_no_dearer_than_a_step_with_spreads_apart=res['mask']['us_max'] <= res['step']['us_min'],
               today_over_mask=round(med('today') / med('mask'), 1),
               mask_bytes_read=n * (64 + 192), mask_bytes_written=n * Q.ACTIONS,
               mask_achieved_TBps=round(n * (64 + 192 + Q.ACTIONS) / (med('mask') * 1e-6) / 1e12, 3))
    del env, saved, probes
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--envs', default='65536,2097152')
    ap.add_argument('--iters', type=int, default=40, help='launches per window of mask / step')
    ap.add_argument('--slow-iters', type=int, default=2, help='rounds of 8 candidates per window of today')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--git-commit', default=None, help='the commit to stamp (default: git rev-parse HEAD)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_query.py needs a GPU')
    from gridworld_amd import _lib as L, query as Q
    line = {'tool': 'tools/bench_query.py', 'query_build_id': Q.build_id(), 'build_id': L.build_id(),
            'git_commit': a.git_commit or BR._git_commit(), 'device': torch.cuda.get_device_name(0), 'sizes': []}
    for n in a.envs.split(','):
        line['sizes'].append(bench(int(n), a.iters, a.slow_iters, a.warmup, max(1, a.repeats)))
    BR._emit(line, a.out)


if __name__ == '__main__':
    main()
