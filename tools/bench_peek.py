#!/usr/bin/env python3
"""Cost of the peek query (igw_peek) on one MI355X; prints one JSON line and writes it to --out.
Per batch size (4,096 and 65,536 envs of an auto-resetting rt20 batch with size_reward=False, stepped 60 times with
uniform random actions; the task table holds 4,096 rows) and per shape (K, H) = (18, 1), (324, 2), (64, 8), (256, 16) --
K shared random candidates of H actions, (18, 1) the 18 actions -- the variants are measured ALTERNATELY in one process
(a, b, c, a, b, ... --repeats times each), every figure the median of its HIP-event windows with the min - max spread:

  peek      one env.peek(out=...) with outputs ('ret', 'ends')
  peek_all  ... with all five outputs
  step      env.step() alone
  today     what answers the question without the query: a second VecGridWorld of N * K rows (at most --chunk-rows of
            them at a time), every state row of the batch replicated K times into it, one
            rollout_actions(return_rewards=True) over the H actions and a torch reduction of the rewards up to each
            first `done` to the return.  The replication is part of what is timed, as a user pays it; the second
            batch's construction and its action tensor are not.  Skipped above --today-rows replicated rows.
  goal      (18, 1) only: env.goal(gain=True, out=...)

    python tools/bench_peek.py [--out profiles/r17_peek_bench.json]
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
SHAPES = ((18, 1), (324, 2), (64, 8), (256, 16))
ROW_BUFFERS = ('grid_buf', 'occ_buf', 'hist_buf', 'agent_buf', 'aux_buf')


def _spread(us):
    return {'us_median': round(float(np.median(us)), 2), 'us_min': round(min(us), 2), 'us_max': round(max(us), 2),
            'windows': len(us)}


def _candidates(k, h, dev):
    if (k, h) == (18, 1):
        return torch.arange(18, dtype=torch.int32, device=dev).reshape(18, 1)
    g = torch.Generator().manual_seed(100 * k + h)
    return torch.randint(0, 18, (k, h), generator=g, dtype=torch.int32).to(dev)


class Today:
    """The second batch of `rows` = per * K rows and what plays the candidates on it."""

    def __init__(self, env, targets, cand, chunk_rows):
        from gridworld_amd import VecGridWorld
        k, h = cand.shape
        self.env, self.k = env, k
        self.per = max(1, min(env.num_envs, chunk_rows // k))
        rows = self.per * k
        self.big = VecGridWorld(rows, autoreset=False, num_tasks=TASKS, size_reward=False, max_steps=env.max_steps)
        self.big.set_tasks(targets, env_task=torch.arange(rows, dtype=torch.int32) % TASKS)
        self.big.reset()
        self.actions = cand.t().repeat(1, self.per).contiguous()      # [H, rows]: row i * K + k plays candidate k
        self.ret = torch.empty((env.num_envs, k), dtype=torch.float32, device=env.device)

    def __call__(self):
        env, big, k = self.env, self.big, self.k
        for lo in range(0, env.num_envs, self.per):
            m = min(self.per, env.num_envs - lo)
            for name in ROW_BUFFERS:
                src, dst = getattr(env, name), getattr(big, name)
                dst[:m * k].view(m, k, -1).copy_(src[lo:lo + m].view(m, 1, -1).expand(m, k, -1))
            rewards, dones = big.rollout_actions(self.actions, return_rewards=True)
            ended_before = (dones.cumsum(0) - dones) != 0
            self.ret[lo:lo + m] = torch.where(ended_before, torch.zeros_like(rewards), rewards).sum(0)[:m * k].view(m, k)
        return self.ret


def bench(n, iters, slow_iters, warmup, repeats, chunk_rows, today_rows):
    from gridworld_amd import VecGridWorld, workloads
    targets = workloads.rt20(TASKS, seed=1).numpy()
    env = VecGridWorld(n, autoreset=True, num_tasks=TASKS, size_reward=False)
    env.set_tasks(targets, env_task=torch.arange(n, dtype=torch.int32) % TASKS)
    env.reset()
    acts = env.fill_actions(60, seed=3)
    for t in range(60):
        env.step(acts[t])
    saved = env.state_dict()
    state = {'t': 0}

    def step():
        env.step(acts[state['t'] % 60])
        state['t'] += 1
    res = {'envs': n, 'task_rows': TASKS, 'shapes': []}
    for k, h in SHAPES:
        env.load_state_dict(saved)
        cand = _candidates(k, h, env.device)
        few = env.peek(cand, outputs=('ret', 'ends'))
        every = env.peek(cand)
        variants = {'peek': (lambda: env.peek(cand, outputs=('ret', 'ends'), out=few), iters),
                    'peek_all': (lambda: env.peek(cand, out=every), iters),
                    'step': (step, iters)}
        today = None
        if n * k <= today_rows:
            today = Today(env, targets, cand, chunk_rows)
            variants['today'] = (today, slow_iters)
        if (k, h) == (18, 1):
            gain = env.goal(todo=False, gain=True)
            variants['goal'] = (lambda: env.goal(todo=False, gain=True, out=gain), iters)
        us = {name: [] for name in variants}
        for r in range(repeats):
            for name, (fn, it) in variants.items():
                if name != 'step':
                    env.load_state_dict(saved)      # (the steps in between moved the state; all answer the same one)
                us[name].append(BR._time(fn, it, warmup if r == 0 else 1))
        env.load_state_dict(saved)
        got = env.peek(cand, out=every)
        w = {name: _spread(v) for name, v in us.items()}
        med = lambda name: w[name]['us_median']  # noqa: E731
        w.update(K=k, H=h, candidates=n * k, candidate_steps=n * k * h,
                 peek_candidate_steps_per_s=round(n * k * h / (med('peek') * 1e-6), 0),
                 peek_all_candidate_steps_per_s=round(n * k * h / (med('peek_all') * 1e-6), 0),
                 peek_over_step=round(med('peek') / med('step'), 3),
                 steps_that_change_a_cell=round(float((got['change'] >= 0).sum()) / (n * k * h), 4),
                 candidates_that_end=round(float((got['ends'] > 0).sum()) / (n * k), 4))
        if today is not None:
            torch.cuda.synchronize()
            same = bool(torch.equal(today().view(torch.int32), got['ret'].view(torch.int32))) if h == 1 else None
            w.update(today_over_peek=round(med('today') / med('peek'), 1), today_rows_per_launch=today.per * k,
                     today_return_equals_peek_bitwise_at_H1=same)
        else:
            w['today'] = f'skipped: {n * k} replicated rows are more than --today-rows {today_rows}'
        if 'goal' in w:
            w['goal_over_peek'] = round(med('goal') / med('peek'), 3)
        res['shapes'].append(w)
        del today, few, every
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--envs', default='4096,65536')
    ap.add_argument('--iters', type=int, default=10, help='launches per window of peek / step / goal')
    ap.add_argument('--slow-iters', type=int, default=1, help='rounds per window of today')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--chunk-rows', type=int, default=1 << 22, help='rows of the second batch of today')
    ap.add_argument('--today-rows', type=int, default=1 << 25, help='today is skipped above this many replicated rows')
    ap.add_argument('--git-commit', default=None, help='the commit to stamp (default: git rev-parse HEAD)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_peek.py needs a GPU')
    from gridworld_amd import _lib as L, peek as P
    line = {'tool': 'tools/bench_peek.py', 'peek_build_id': P.build_id(), 'build_id': L.build_id(),
            'git_commit': a.git_commit or BR._git_commit(), 'device': torch.cuda.get_device_name(0), 'sizes': []}
    for n in a.envs.split(','):
        line['sizes'].append(bench(int(n), a.iters, a.slow_iters, a.warmup, max(1, a.repeats), a.chunk_rows, a.today_rows))
    BR._emit(line, a.out)


if __name__ == '__main__':
    main()
