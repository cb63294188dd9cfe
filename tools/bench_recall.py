#!/usr/bin/env python3
"""Cost of the recall query (igw_recall) on one MI355X against composing it from the launches that
existed before it; prints one JSON line and writes it to --out.  The log: 65,536 envs (an auto-resetting rt20 batch
without SizeReward, max_steps = 250, the task table holds 4,096 rows) stepped 250 times with uniform random actions with
the trajectory log on.  Per batch size (4,096 and 65,536 samples drawn from that log with recall.sample) and per stack
K (1 and 4), for grid + target one-hot + agent in the world frame as float16, the variants are measured ALTERNATELY in
one process (a, b, c, a, b, c, ... --repeats times each), every figure the median of its HIP-event windows with the min -
max spread:

  recall        one igw_recall launch (G.recall on prepared first / length / starts / init_pose / goal rows): obs +
                next_obs + record + valid, into preallocated tensors
  recall_env    env.recall(spec, episode=, step=, goals='own'): the same launch behind the torch operations that take
                slots, lengths, starting rows and reset poses from the log's heads and the task table
  today         the way without the query, per distinct entry of the two stacks (K + 1 of them): one
                relabel(outputs=('target',), at=entry) launch that rebuilds the grids, the torch operations that fabricate
                64-byte agent records (float64 x, y, z, yaw from the record's float32 agentPos, or the reset pose for
                entry 0) and 16-byte aux records, one stateless igw_vox_obs launch; then the `cat` of the entries into
                the two stacks and the gather of the step's record

Before anything is timed the two sides are compared: `today` equals `recall` bit for bit on obs, next_obs and record.

    python tools/bench_recall.py [--out profiles/r22_recall_bench.json]
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
ALL = ('obs', 'next_obs', 'record', 'valid')


def _spread(us):
    return {'us_median': round(float(np.median(us)), 2), 'us_min': round(min(us), 2), 'us_max': round(max(us), 2),
            'windows': len(us)}


def make_log(n):
    from gridworld_amd import VecGridWorld, vec_env as V, workloads
    env = VecGridWorld(n, autoreset=True, num_tasks=TASKS, size_reward=False, max_steps=STEPS)
    env.set_tasks(workloads.rt20(TASKS, seed=1).numpy(), env_task=torch.arange(n, dtype=torch.int32) % TASKS)
    rec, heads = env.enable_trajectory_log(n)
    env.reset()
    acts = env.fill_actions(STEPS, seed=3)
    for t in range(STEPS):
        env.step(acts[t])
    first, length, task, valid = V.finished_episodes(heads, 0, STEPS)
    assert bool(valid.all())
    starts = env.task_start.index_select(0, task)
    init = env.task_meta.index_select(0, task)[:, :40].contiguous().view(torch.float64)
    goal = env.task_target.index_select(0, task) + starts
    return env, rec, first, length, starts, init, goal


def bench(log, b, stacks, iters, slow_iters, warmup, repeats):
    import gridworld_amd as G
    from gridworld_amd import relabel as RL, vox as X
    env, rec, first, length, starts, init, goal = log
    dev, n = env.device, first.shape[0]
    episode, step = G.recall.sample(length, b, seed=5)
    ep = episode.long()
    # what `today` gathers once per minibatch: the sampled episodes as relabel's E = B episodes
    rows = rec.view(-1, 64)
    res = {'samples': b, 'logged_envs': n, 'steps': STEPS, 'mean_step': round(float(step.float().mean()), 1), 'stacks': []}
    for k in stacks:
        spec = G.VoxSpec(planes=(('grid', 'onehot'), ('target', 'onehot')), agent=True, dtype=torch.float16, stack=k)
        one = G.VoxSpec(planes=spec.planes, agent=True, dtype=torch.float16, stack=1)
        out = G.recall.outputs(spec, b, ALL, dev)
        agent = torch.zeros((b, 64), dtype=torch.uint8, device=dev)
        aux = torch.zeros((b, 16), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream

        def entry(s):
            """[B, C, 9, 11, 11]: the planes of entry s [B] of the sampled episodes, the way without the query."""
            f_b, l_b, st_b = first.index_select(0, ep), length.index_select(0, ep), starts.index_select(0, ep)
            grid = RL.relabel(rec, f_b, l_b, st_b, at=s[:, None].to(torch.int32).contiguous(), outputs=('target',),
                              pad=STEPS)['target']
            at = (f_b + s.long() - 1).clamp(min=0)
            pose32 = rows.index_select(0, at)[:, :20].contiguous().view(torch.float32)
            logged = torch.stack([pose32[:, 0], pose32[:, 1], pose32[:, 2], pose32[:, 4]], 1).to(torch.float64)
            pose = torch.where((s == 0)[:, None], init.index_select(0, ep)[:, :4], logged)
            agent.view(torch.float64)[:, :4] = pose
            aux.view(torch.int32)[:, 2] = episode
            grid_rows = torch.as_strided(grid, (b, 1104), (1104, 1), grid.storage_offset())
            return X.launch(agent, aux, b, one, [(grid_rows.data_ptr(), None, 1104, 0), (goal.data_ptr(), None, 1104, 1)],
                            None, None, True, dev, stream)

        def today():
            t = step.long()
            planes = [entry((t - k + j).clamp(min=0)) for j in range(k + 1)]
            return (torch.cat(planes[:k], 1), torch.cat(planes[1:], 1),
                    rows.index_select(0, first.index_select(0, ep) + t - 1))

        def recall():
            return G.recall(rec, first, length, starts, init, episode, step, spec, goal=goal, outputs=ALL, out=out,
                            pad=STEPS)

        def recall_env():
            return env.recall(spec, episode=episode, step=step, goals='own', out=out)
        # the two sides compute the same thing
        got = recall()
        obs, nxt, record = today()
        assert bool(got['valid'].all())
        assert torch.equal(got['obs'].view(torch.int16), obs.view(torch.int16)), (b, k, 'obs')
        assert torch.equal(got['next_obs'].view(torch.int16), nxt.view(torch.int16)), (b, k, 'next_obs')
        assert torch.equal(got['record'], record), (b, k, 'record')
        del obs, nxt, record
        variants = {'recall': (recall, iters), 'recall_env': (recall_env, iters), 'today': (today, slow_iters)}
        us = {name: [] for name in variants}
        for r in range(repeats):
            for name, (fn, it) in variants.items():
                us[name].append(BR._time(fn, it, warmup if r == 0 else 1))
        row = {name: _spread(v) for name, v in us.items()}
        med = lambda name: row[name]['us_median']  # noqa: E731
        written = b * (2 * int(np.prod(spec.shape(1))) * 2 + 64 + 1)
        read = int(step.sum()) * 64 + b * (2 * 1104 + 64 + 8 + 4 + 4 + 8)   # record lines of the walk, start and goal rows
        row.update(stack=k, compared_bit_for_bit=True, bytes_written=written, bytes_read=read,
                   write_TBps={name: round(written / (med(name) * 1e-6) / 1e12, 3) for name in ('recall', 'recall_env')},
                   share_of_8TBps=round(written / HBM_PEAK * 1e6 / med('recall'), 3),
                   today_over_recall=round(med('today') / med('recall'), 2),
                   today_over_recall_env=round(med('today') / med('recall_env'), 2),
                   ns_per_sample={name: round(med(name) * 1e3 / b, 2) for name in variants})
        res['stacks'].append(row)
        del out, got
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--envs', type=int, default=65536, help='logged envs')
    ap.add_argument('--samples', default='4096,65536')
    ap.add_argument('--stacks', default='1,4')
    ap.add_argument('--iters', type=int, default=20, help='launches per window of the query')
    ap.add_argument('--slow-iters', type=int, default=3, help='rounds per window of the composition')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--git-commit', default=None, help='the commit to stamp (default: git rev-parse HEAD)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_recall.py needs a GPU')
    from gridworld_amd import _lib as L, recall as R
    line = {'tool': 'tools/bench_recall.py', 'recall_build_id': R.build_id(), 'build_id': L.build_id(),
            'git_commit': a.git_commit or BR._git_commit(), 'device': torch.cuda.get_device_name(0), 'sizes': []}
    log = make_log(a.envs)
    for b in a.samples.split(','):
        line['sizes'].append(bench(log, int(b), [int(k) for k in a.stacks.split(',')], a.iters, a.slow_iters, a.warmup,
                                   max(1, a.repeats)))
    BR._emit(line, a.out)


if __name__ == '__main__':
    main()
