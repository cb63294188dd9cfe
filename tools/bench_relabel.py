#!/usr/bin/env python3
"""Cost of the relabel query (igw_relabel) on one MI355X against replaying the episodes; prints one
JSON line and writes it to --out.  Per batch size (4,096 and 65,536 logged episodes of 250 steps: an auto-resetting rt20
batch without SizeReward, max_steps = 250, stepped 250 times with uniform random actions with the trajectory log on; the
task table holds 4,096 rows) and per number of goals G (1: the final grid; 4: HER's "future" entries, relabel_future)
the variants are measured ALTERNATELY in one process (a, b, ..., a, b, ... --repeats times each), every figure the
median of its HIP-event windows with the min - max spread:

  relabel       one igw_relabel launch (G.relabel on prepared first / length / starts / at): reward + done + end, into
                preallocated tensors
  relabel_env   env.relabel(goals): the same launch behind the torch operations that take slots, lengths and starting
                rows from the log's heads
  replay        the way without the query, per goal: set_tasks(hindsight targets) on a second VecGridWorld(autoreset=
                False) batch, reset, rollout_actions(the logged actions, return_rewards=True); the G goals one after
                the other

Before anything is timed the two sides are compared: on the envs whose logged episode ran its 250 steps the replayed
rewards and dones equal the relabelled ones bit for bit (an env that completed its target earlier logged a shorter
episode, which the replay of the 250 actions does not reproduce; such envs are counted, not compared).

    python tools/bench_relabel.py [--out profiles/r21_relabel_bench.json]
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

TASKS, STEPS = 4096, 250
HBM_PEAK = 8e12
NAMES = ('reward', 'done', 'end')


def _spread(us):
    return {'us_median': round(float(np.median(us)), 2), 'us_min': round(min(us), 2), 'us_max': round(max(us), 2),
            'windows': len(us)}


def bench(n, goal_counts, iters, slow_iters, warmup, repeats):
    import gridworld_amd as G
    from gridworld_amd import VecGridWorld, vec_env as V, workloads
    kw = dict(size_reward=False, max_steps=STEPS)
    env = VecGridWorld(n, autoreset=True, num_tasks=TASKS, **kw)
    env.set_tasks(workloads.rt20(TASKS, seed=1).numpy(), env_task=torch.arange(n, dtype=torch.int32) % TASKS)
    rec, heads = env.enable_trajectory_log(n)
    env.reset()
    acts = env.fill_actions(STEPS, seed=3)
    for t in range(STEPS):
        env.step(acts[t])
    twin = VecGridWorld(n, autoreset=False, num_tasks=n, **kw)
    first, length, task, valid = V.finished_episodes(heads, 0, STEPS)
    starts = env.task_start.index_select(0, task)
    assert bool(valid.all())
    whole = length == STEPS
    words = rec.view(n * 2, STEPS, 64)[:, :, 40:42].index_select(0, first // STEPS).contiguous().view(torch.int16)[..., 0]
    logged = torch.arange(STEPS, device=env.device)[None] < length[:, None]
    snap = twin.state_dict()
    res = {'episodes': n, 'steps': STEPS, 'task_rows': TASKS, 'episodes_of_250_steps': int(whole.sum()),
           'logged_steps': int(length.sum()), 'p_changed': round(float(((words != -1) & logged).sum()) / float(length.sum()), 4),
           'goals': []}
    for g in goal_counts:
        at = length[:, None].contiguous() if g == 1 else G.relabel_future(length, g, seed=7)
        goals = 'final' if g == 1 else at
        out = G.relabel.outputs(n, g, STEPS, NAMES, env.device)
        target = G.relabel(rec, first, length, starts, at=at, outputs=('target',))['target']
        rows = [target[:, k].reshape(n, -1).contiguous() for k in range(g)]

        def replay(fresh=False):
            got = []
            for k in range(g):
                if fresh:   # (an agent's vertical speed, sub-step count and hotbar slot leak through a reset)
                    twin.load_state_dict(snap)
                twin.set_tasks(rows[k])
                twin.reset()
                got.append(twin.rollout_actions(acts, return_rewards=True))
            return got
        # the two sides compute the same thing (where the logged episode is the 250 actions)
        G.relabel(rec, first, length, starts, at=at, outputs=NAMES, out=out)
        same = 0
        for k, (rw, dn) in enumerate(replay(fresh=True)):
            a, b = out['reward'][:, k][whole], rw.t()[whole]
            assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), (n, g, k)
            assert torch.equal(out['done'][:, k][whole], dn.t()[whole]), (n, g, k)
            same += int(whole.sum())
        variants = {'relabel': (lambda: G.relabel(rec, first, length, starts, at=at, outputs=NAMES, out=out), iters),
                    'relabel_env': (lambda: env.relabel(goals, outputs=NAMES, out=out), iters),
                    'replay': (replay, slow_iters)}
        us = {k: [] for k in variants}
        for r in range(repeats):
            for k, (fn, it) in variants.items():
                us[k].append(BR._time(fn, it, warmup if r == 0 else 1))
        row = {k: _spread(v) for k, v in us.items()}
        med = lambda k: row[k]['us_median']  # noqa: E731
        written = n * g * (STEPS * 5 + 4)                              # reward + done per step, end per pair
        read = n * (STEPS * 64 + 1104 + 12) + n * g * 4                # whole records move (64-byte lines), start row, first / length, at
        row.update(goals=g, pairs_compared_bit_for_bit=same, bytes_written=written, bytes_read=read,
                   us_at_8TBps=round((written + read) / HBM_PEAK * 1e6, 2),
                   share_of_8TBps=round((written + read) / HBM_PEAK * 1e6 / med('relabel'), 3),
                   replay_over_relabel=round(med('replay') / med('relabel'), 1),
                   replay_over_relabel_env=round(med('replay') / med('relabel_env'), 1),
                   ns_per_episode_goal={k: round(med(k) * 1e3 / (n * g), 2) for k in variants})
        res['goals'].append(row)
        del out, target, rows
    del env, twin, rec, heads
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--episodes', default='4096,65536')
    ap.add_argument('--goals', default='1,4')
    ap.add_argument('--iters', type=int, default=50, help='launches per window of the query')
    ap.add_argument('--slow-iters', type=int, default=2, help='rounds per window of the replay')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--git-commit', default=None, help='the commit to stamp (default: git rev-parse HEAD)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_relabel.py needs a GPU')
    from gridworld_amd import _lib as L, relabel as R
    line = {'tool': 'tools/bench_relabel.py', 'relabel_build_id': R.build_id(), 'build_id': L.build_id(),
            'git_commit': a.git_commit or BR._git_commit(), 'device': torch.cuda.get_device_name(0), 'sizes': []}
    for n in a.episodes.split(','):
        line['sizes'].append(bench(int(n), [int(g) for g in a.goals.split(',')], a.iters, a.slow_iters, a.warmup,
                                   max(1, a.repeats)))
    BR._emit(line, a.out)


if __name__ == '__main__':
    main()
