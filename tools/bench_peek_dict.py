#!/usr/bin/env python3
"""Cost of the peek query of the flying and walking Dict spaces (igw_peek_flying, igw_peek_walking_dict; DESIGN.md
section 15) on one MI355X; prints one JSON line and writes it to --out.  65,536 envs of an auto-resetting rt20 batch with
size_reward=False, stepped 60 times with random actions of the space (the task table holds 4,096 rows); flying with
(K, H) = (64, 8) and (256, 16), the walking Dict space with (64, 8); K shared random candidates of H actions.  The
variants are measured ALTERNATELY in one process (a, b, c, a, b, ... --repeats times each), every figure the median of
its HIP-event windows with the min - max spread:

  peek      one env.peek_dict(out=...) with outputs ('ret', 'ends')
  peek_all  ... with all five outputs
  step      env.step() alone (windows of --step-iters launches: one takes about 16 us)
  today     the only other way the project offers: a second VecGridWorld of N * K rows (at most --chunk-rows of them at a
            time), every state row of the batch replicated K times into it, the H actions played on it -- flying: one
            rollout_actions(return_rewards=True) (igw_rollout_flying_actions); walking Dict, which has no fused rollout:
            H calls of step() -- and a torch reduction of the rewards up to each first `done` to the return.  The
            replication is part of what is timed, as a user pays it; the second batch's construction and its action
            tensors are not.  This is the yardstick, not the code under test.

    python tools/bench_peek_dict.py [--out profiles/r19_peek_dict_bench.json]
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
POINTS = (('flying', 64, 8), ('flying', 256, 16), ('walking_dict', 64, 8))
ROW_BUFFERS = ('grid_buf', 'occ_buf', 'hist_buf', 'agent_buf', 'aux_buf')
KW = {'flying': dict(action_space='flying'), 'walking_dict': dict(action_space='walking', discretize=False)}


def _spread(us):
    return {'us_median': round(float(np.median(us)), 2), 'us_min': round(min(us), 2), 'us_max': round(max(us), 2),
            'windows': len(us)}


def random_actions(space, lead, seed, dev):
    """The space's dict of device tensors of leading shape `lead`: a place in 30 % of the actions, a break in 20 %, a
    hotbar change in 25 %, movement in half of them, camera deltas within +-30 degrees."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *tail: torch.rand(tuple(lead) + tail, generator=g)  # noqa: E731
    act = u()
    place, brk = act < 0.30, (act >= 0.30) & (act < 0.50)
    hot = torch.where(u() < 0.25, torch.randint(1, 7, tuple(lead), generator=g), torch.zeros(tuple(lead), dtype=torch.int64))
    cam = ((u(2) * 2 - 1) * 30).float()
    moving = u() < 0.5
    if space == 'flying':
        mv = (u(3) * 2 - 1) * moving[..., None]
        mv[..., 2] *= u() < 0.3
        out = dict(movement=mv.float(), camera=cam, inventory=hot.int(), placement=(place.int() + 2 * brk.int()))
    else:
        b = torch.stack([moving & (u() < p) for p in (0.5, 0.2, 0.25, 0.25)] + [u() < 0.1, brk, place, hot.bool()], -1).to(torch.uint8)
        b[..., 7] = hot.to(torch.uint8)
        out = dict(buttons=b, camera=cam)
    return {k: v.contiguous().to(dev) for k, v in out.items()}


class Today:
    """The second batch of `rows` = per * K rows and what plays the candidates on it."""

    def __init__(self, space, env, targets, cand, k, h, chunk_rows):
        from gridworld_amd import VecGridWorld
        self.space, self.env, self.k, self.h = space, env, k, h
        self.per = max(1, min(env.num_envs, chunk_rows // k))
        rows = self.per * k
        self.big = VecGridWorld(rows, autoreset=False, num_tasks=TASKS, size_reward=False, max_steps=env.max_steps, **KW[space])
        self.big.set_tasks(targets, env_task=torch.arange(rows, dtype=torch.int32) % TASKS)
        self.big.reset()
        # [H, rows, ...]: row i * K + k plays candidate k
        self.actions = {key: v.transpose(0, 1).repeat(1, self.per, *([1] * (v.dim() - 2))).contiguous() for key, v in cand.items()}
        self.ret = torch.empty((env.num_envs, k), dtype=torch.float32, device=env.device)

    def __call__(self):
        env, big, k = self.env, self.big, self.k
        for lo in range(0, env.num_envs, self.per):
            m = min(self.per, env.num_envs - lo)
            for name in ROW_BUFFERS:
                src, dst = getattr(env, name), getattr(big, name)
                dst[:m * k].view(m, k, -1).copy_(src[lo:lo + m].view(m, 1, -1).expand(m, k, -1))
            if self.space == 'flying':
                rewards, dones = big.rollout_actions(self.actions, return_rewards=True)
            else:
                rw, dn = [], []
                for t in range(self.h):
                    _, r, d, _ = big.step({key: v[t] for key, v in self.actions.items()})
                    rw.append(r.clone())
                    dn.append(d.clone())
                rewards, dones = torch.stack(rw), torch.stack(dn)
            ended_before = (dones.cumsum(0) - dones) != 0
            self.ret[lo:lo + m] = torch.where(ended_before, torch.zeros_like(rewards), rewards).sum(0)[:m * k].view(m, k)
        return self.ret


def bench(space, n, points, iters, step_iters, slow_iters, warmup, repeats, chunk_rows):
    from gridworld_amd import VecGridWorld, workloads
    targets = workloads.rt20(TASKS, seed=1).numpy()
    env = VecGridWorld(n, autoreset=True, num_tasks=TASKS, size_reward=False, **KW[space])
    env.set_tasks(targets, env_task=torch.arange(n, dtype=torch.int32) % TASKS)
    env.reset()
    acts = random_actions(space, (60, n), 3, env.device)
    for t in range(60):
        env.step({k: v[t] for k, v in acts.items()})
    saved = env.state_dict()
    state = {'t': 0}

    def step():
        env.step({k: v[state['t'] % 60] for k, v in acts.items()})
        state['t'] += 1
    res = []
    for k, h in points:
        env.load_state_dict(saved)
        cand = random_actions(space, (k, h), 100 * k + h, env.device)
        few = env.peek_dict(cand, outputs=('ret', 'ends'))
        every = env.peek_dict(cand)
        today = Today(space, env, targets, cand, k, h, chunk_rows)
        variants = {'peek': (lambda: env.peek_dict(cand, outputs=('ret', 'ends'), out=few), iters),
                    'peek_all': (lambda: env.peek_dict(cand, out=every), iters),
                    'step': (step, step_iters), 'today': (today, slow_iters)}
        us = {name: [] for name in variants}
        for r in range(repeats):
            for name, (fn, it) in variants.items():
                if name != 'step':
                    env.load_state_dict(saved)      # (the steps in between moved the state; all answer the same one)
                us[name].append(BR._time(fn, it, warmup if r == 0 else 1))
        env.load_state_dict(saved)
        got = env.peek_dict(cand, out=every)
        w = {name: _spread(v) for name, v in us.items()}
        med = lambda name: w[name]['us_median']  # noqa: E731
        torch.cuda.synchronize()
        w.update(space=space, envs=n, K=k, H=h, candidates=n * k, candidate_steps=n * k * h,
                 peek_candidate_steps_per_s=round(n * k * h / (med('peek') * 1e-6), 0),
                 peek_over_step=round(med('peek') / med('step'), 3), today_over_peek=round(med('today') / med('peek'), 2),
                 today_rows_per_launch=today.per * k,
                 today_return_differs_from_peek_float32_sum=int((today().view(torch.int32) != got['ret'].view(torch.int32)).sum()),
                 steps_that_change_a_cell=round(float((got['change'] >= 0).sum()) / (n * k * h), 4),
                 candidates_that_end=round(float((got['ends'] > 0).sum()) / (n * k), 4))
        res.append(w)
        del today, few, every
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--envs', type=int, default=65536)
    ap.add_argument('--iters', type=int, default=10, help='launches per window of peek / step')
    ap.add_argument('--step-iters', type=int, default=500, help='launches per window of step (about 16 us each)')
    ap.add_argument('--slow-iters', type=int, default=1, help='rounds per window of today')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--chunk-rows', type=int, default=1 << 22, help='rows of the second batch of today')
    ap.add_argument('--git-commit', default=None, help='the commit to stamp (default: git rev-parse HEAD)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_peek_dict.py needs a GPU')
    from gridworld_amd import _lib as L, peek_dict as D
    line = {'tool': 'tools/bench_peek_dict.py', 'peek_dict_build_id': D.build_id(), 'build_id': L.build_id(),
            'git_commit': a.git_commit or BR._git_commit(), 'device': torch.cuda.get_device_name(0), 'task_rows': TASKS,
            'points': []}
    for space in ('flying', 'walking_dict'):
        points = [(k, h) for s, k, h in POINTS if s == space]
        line['points'] += bench(space, a.envs, points, a.iters, a.step_iters, a.slow_iters, a.warmup, max(1, a.repeats), a.chunk_rows)
    BR._emit(line, a.out)


if __name__ == '__main__':
    main()
