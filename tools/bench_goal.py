#!/usr/bin/env python3
"""Cost of the goal query (igw_goal) on one MI355X; prints one JSON line and writes it to --out.
Per batch size (65,536 and 2,097,152 envs of an auto-resetting rt20 batch without SizeReward, stepped 60 times with
uniform random actions; the task table holds 4,096 rows) the variants are measured ALTERNATELY in one process (a, b, c,
..., a, b, ... --repeats times each), every figure the median of its HIP-event windows with the min - max spread:

  align_fit          one igw_goal launch: align and fit, into preallocated tensors
  todo               + todo
  want_todo          + want
  full               + gain and ends, with what gain=True launches in front (two igw_action_mask launches, the copy of
                     the agent records)
  step               env.step() alone
  today_align        the alignment without the query: the synthetic rows gathered in torch (grid - start[task],
                     target[task]) and vec_env.task_eval on them (its results come back as numpy)
  today_gain         the rewards without the query: for each of the 8 place / break actions, load_state_dict() of a
                     saved state and one step()

    python tools/bench_goal.py [--out profiles/r14_goal_bench.json]
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
# bytes per env from the kernel's own access list (include/igw_goal.h), rt20: no starting grids.  The target rows and
# the colour index belong to the task table's 4,096 rows (4.5 MB + 5.9 MB), which every env of the batch shares.
READ = {'align_fit': 1024 + 16 + 16, 'todo': 1104 + 1104, 'want': 0, 'gain': 16 + 18 + 4}
WRITE = {'align_fit': 4 + 8, 'todo': 1104, 'want': 1104, 'gain': 72 + 18}
MASKS = 2 * (64 + 192) + 2 * 18 + 4 + 2 * 64   # the two mask launches and the copy of the agent records
GAIN_PER_ACTING_ACTION = 160 + 2            # one level block of the colour index, a grid and a start byte


def _spread(us):
    return {'us_median': round(float(np.median(us)), 2), 'us_min': round(min(us), 2), 'us_max': round(max(us), 2),
            'windows': len(us)}


def bench(n, iters, slow_iters, warmup, repeats):
    from gridworld_amd import VecGridWorld, query as Q, vec_env as V, workloads
    env = VecGridWorld(n, autoreset=True, num_tasks=TASKS, size_reward=False)
    env.set_tasks(workloads.rt20(TASKS, seed=1).numpy(),
                  env_task=torch.arange(n, dtype=torch.int32) % TASKS)
    env.reset()
    acts = env.fill_actions(60, seed=3)
    for t in range(60):
        env.step(acts[t])
    out = env.goal(want=True, gain=True)
    probes = [torch.full((n,), p, dtype=torch.int32, device=env.device) for p in Q.PROBES]
    saved = env.state_dict()
    state = {'t': 0}
    pick = lambda *keys: {k: out[k] for k in ('align', 'fit') + keys}  # noqa: E731

    def step():
        env.step(acts[state['t'] % 60])
        state['t'] += 1

    def today_align():
        task = env.env_task.long()
        V.task_eval(env.task_target[task], env.grid_buf - env.task_start[task], device=env.device)

    def today_gain():
        for a in probes:
            env.load_state_dict(saved)
            env.step(a)
    variants = {'align_fit': (lambda: env.goal(todo=False, out=pick()), iters),
                'todo': (lambda: env.goal(out=pick('todo')), iters),
                'want_todo': (lambda: env.goal(want=True, out=pick('want', 'todo')), iters),
                'full': (lambda: env.goal(want=True, gain=True, out=out), iters),
                'step': (step, iters),
                'today_align': (today_align, slow_iters),
                'today_gain': (today_gain, slow_iters)}
    us = {k: [] for k in variants}
    for r in range(repeats):
        for k, (fn, it) in variants.items():
            us[k].append(BR._time(fn, it, warmup if r == 0 else 1))
    env.load_state_dict(saved)
    env.goal(want=True, gain=True, out=out)
    res = {k: _spread(v) for k, v in us.items()}
    med = lambda k: res[k]['us_median']  # noqa: E731
    acting = float((env._goal_scratch()[0][:, list(Q.PROBES)] != 0).float().sum(1).mean())
    by = {'align_fit': READ['align_fit'] + WRITE['align_fit']}
    by['todo'] = by['align_fit'] + READ['todo'] + WRITE['todo']
    by['want_todo'] = by['todo'] + READ['want'] + WRITE['want']
    by['full'] = by['want_todo'] + READ['gain'] + WRITE['gain'] + MASKS + round(acting * GAIN_PER_ACTING_ACTION)
    res.update(envs=n, task_rows=TASKS, acting_probe_actions_per_env=round(acting, 3),
               share_of_envs_with_a_match=round(float((out['fit'][:, 0] > 0).float().mean()), 4),
               bytes_per_env=by,
               us_at_8TBps={k: round(n * b / HBM_PEAK * 1e6, 2) for k, b in by.items()},
               share_of_8TBps={k: round(n * b / HBM_PEAK * 1e6 / med(k), 3) for k, b in by.items()},
               align_fit_over_step=round(med('align_fit') / med('step'), 3),
               align_fit_no_dearer_than_a_step_with_spreads_apart=res['align_fit']['us_max'] <= res['step']['us_min'],
               today_align_over_todo=round(med('today_align') / med('todo'), 1),
               today_gain_over_full=round(med('today_gain') / med('full'), 1),
               full_cheaper_than_todays_routes=res['full']['us_max'] < min(res['today_align']['us_min'],
                                                                           res['today_gain']['us_min']))
    del env, saved, probes, out
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--envs', default='65536,2097152')
    ap.add_argument('--iters', type=int, default=40, help='launches per window of the queries and the step')
    ap.add_argument('--slow-iters', type=int, default=2, help='rounds per window of today_align / today_gain')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--git-commit', default=None, help='the commit to stamp (default: git rev-parse HEAD)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_goal.py needs a GPU')
    from gridworld_amd import _lib as L, goal as G, query as Q
    line = {'tool': 'tools/bench_goal.py', 'goal_build_id': G.build_id(), 'query_build_id': Q.build_id(),
            'build_id': L.build_id(), 'git_commit': a.git_commit or BR._git_commit(),
            'device': torch.cuda.get_device_name(0), 'sizes': []}
    for n in a.envs.split(','):
        line['sizes'].append(bench(int(n), a.iters, a.slow_iters, a.warmup, max(1, a.repeats)))
    BR._emit(line, a.out)


if __name__ == '__main__':
    main()
