#!/usr/bin/env python3
"""Cost of the worth query (igw_worth) on one MI355X; prints one JSON line and writes it to --out.
Per batch size (4,096 and 65,536 envs of an auto-resetting rt20 batch without SizeReward, stepped 60 times with uniform
random actions; the task table holds 4,096 rows) the variants are measured ALTERNATELY in one process (a, b, c, ..., a,
b, ... --repeats times each), every figure the median of its HIP-event windows with the min - max spread:

  best               one igw_worth launch: best alone, into a preallocated tensor
  word_best          word + best, into preallocated tensors
  step               env.step() alone
  goal_gain          env.goal(gain=True) into preallocated tensors (the two mask launches in front of it counted)
  today              the map without the query, at --today-envs envs (64: 487,872 evaluations) and scaled per env: every
                     env's synthetic grid replicated 7,623 times in torch, one cell edited in each copy, and
                     vec_env.task_eval on the rows (its results come back as numpy)

    python tools/bench_worth.py [--out profiles/r20_worth_bench.json]
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
HBM_PEAK = 8e12
EDITS = 7 * 1089
# bytes per env from the kernel's own access list (include/igw_worth.h), rt20: no starting grids.  The colour index
# belongs to the task table's 4,096 rows (5.9 MB), which every env of the batch shares.
READ = 1104 + 1024 + 16 + 16 + 16 + 1440       # grid row, histogram row, episode record, agent piece, bbox, colour index
WRITE = {'best': 16, 'word_best': 16 + 7 * 1104 * 2}


def _spread(us):
    return {'us_median': round(float(np.median(us)), 2), 'us_min': round(min(us), 2), 'us_max': round(max(us), 2),
            'windows': len(us)}


def bench(n, iters, slow_iters, warmup, repeats, today_envs):
    from gridworld_amd import VecGridWorld, vec_env as V, workloads
    env = VecGridWorld(n, autoreset=True, num_tasks=TASKS, size_reward=False)
    env.set_tasks(workloads.rt20(TASKS, seed=1).numpy(), env_task=torch.arange(n, dtype=torch.int32) % TASKS)
    env.reset()
    acts = env.fill_actions(60, seed=3)
    for t in range(60):
        env.step(acts[t])
    out = env.worth()
    goal = env.goal(gain=True)
    state = {'t': 0}
    m = min(today_envs, n)
    cells = torch.arange(EDITS, device=env.device) % 1089
    colour = (torch.arange(EDITS, device=env.device) // 1089).to(torch.int8)

    def step():
        env.step(acts[state['t'] % 60])
        state['t'] += 1

    def today():
        task = env.env_task[:m].long()
        s = env.grid_buf[:m] - env.task_start[task]                                   # [m, 1104]
        rows = s[:, None, :].expand(m, EDITS, s.shape[1]).contiguous()
        rows[:, torch.arange(EDITS, device=env.device), cells] = colour[None, :] - env.task_start[task][:, cells]
        V.task_eval(env.task_target[task].repeat_interleave(EDITS, 0), rows.reshape(m * EDITS, -1), device=env.device)
    variants = {'best': (lambda: env.worth(outputs=('best',), out={'best': out['best']}), iters),
                'word_best': (lambda: env.worth(out=out), iters),
                'step': (step, iters),
                'goal_gain': (lambda: env.goal(gain=True, out=goal), iters),
                'today': (today, slow_iters)}
    us = {k: [] for k in variants}
    for r in range(repeats):
        for k, (fn, it) in variants.items():
            us[k].append(BR._time(fn, it, warmup if r == 0 else 1))
    res = {k: _spread(v) for k, v in us.items()}
    med = lambda k: res[k]['us_median']  # noqa: E731
    env.worth(out=out)
    w = torch.as_strided(out['word'], (n, 7, 1089), (7 * 1104, 1104, 1)).to(torch.int32)
    valid = w >= 0
    right = torch.where(valid, ((w & 0xfff) ^ 0x800) - 0x800, torch.zeros_like(w))
    by = {k: READ + v for k, v in WRITE.items()}
    today_per_env = med('today') / m
    res.update(envs=n, task_rows=TASKS, today_envs=m, today_evaluations=m * EDITS,
               today_us_per_env=round(today_per_env, 2), today_us_scaled_to_envs=round(today_per_env * n, 1),
               today_over_word_best=round(today_per_env * n / med('word_best'), 1),
               valid_edits_per_env=round(float(valid.sum()) / n, 1),
               edits_with_right_not_0_per_env=round(float((right != 0).sum()) / n, 1),
               bytes_per_env=by,
               us_at_8TBps={k: round(n * b / HBM_PEAK * 1e6, 2) for k, b in by.items()},
               share_of_8TBps={k: round(n * b / HBM_PEAK * 1e6 / med(k), 3) for k, b in by.items()},
               word_store_GBps=round(n * 7 * 1104 * 2 / (med('word_best') * 1e-6) / 1e9, 1),
               word_store_share_of_8TBps=round(n * 7 * 1104 * 2 / (med('word_best') * 1e-6) / HBM_PEAK, 3),
               word_best_over_best=round(med('word_best') / med('best'), 2),
               word_best_over_step=round(med('word_best') / med('step'), 1),
               word_best_over_goal_gain=round(med('word_best') / med('goal_gain'), 1))
    del env, out, goal
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--envs', default='4096,65536')
    ap.add_argument('--iters', type=int, default=40, help='launches per window of the queries and the step')
    ap.add_argument('--slow-iters', type=int, default=1, help='rounds per window of today')
    ap.add_argument('--today-envs', type=int, default=64, help='envs of the batch today\'s way is run on')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--git-commit', default=None, help='the commit to stamp (default: git rev-parse HEAD)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_worth.py needs a GPU')
    from gridworld_amd import _lib as L, goal as G, query as Q, worth as W
    line = {'tool': 'tools/bench_worth.py', 'worth_build_id': W.build_id(), 'goal_build_id': G.build_id(),
            'query_build_id': Q.build_id(), 'build_id': L.build_id(), 'git_commit': a.git_commit or BR._git_commit(),
            'device': torch.cuda.get_device_name(0), 'sizes': []}
    for n in a.envs.split(','):
        line['sizes'].append(bench(int(n), a.iters, a.slow_iters, a.warmup, max(1, a.repeats), a.today_envs))
    BR._emit(line, a.out)


if __name__ == '__main__':
    main()
