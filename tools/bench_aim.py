#!/usr/bin/env python3
"""Cost of the aim query (igw_aim) on one MI355X; prints one JSON line and writes it to --out.
Per batch size (4,096 and 65,536 envs of an auto-resetting rt20 batch, stepped 60 times with uniform random actions; the
task table holds 4,096 rows) and per window (max_turns 4, 12 and 72) three variants are measured ALTERNATELY in one
process (a, b, c, a, b, ... --repeats times each), every figure the median of its HIP-event windows with the min - max
spread:

  aim     one igw_aim launch into preallocated planes
  step    env.step() alone
  today   what answers the question without the query: the agent and occupancy rows replicated once per direction of
          the window with the rotation rewritten, one igw_action_mask(look=True) launch over all the copies, then a
          torch scatter-min of the directions' codes per cell.  The copies of --chunk-rows rows at a time (65,536 envs
          x up to 2,664 directions that exist are up to 45 GB of copies); the replication is part of what is timed, as a user pays it.
          (It looks at the inventory, which igw_aim does not: the timing is what is compared, not the answer.)

    python tools/bench_aim.py [--out profiles/r16_aim_bench.json]
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
WINDOWS = (4, 12, 72)


def _spread(us):
    return {'us_median': round(float(np.median(us)), 2), 'us_min': round(min(us), 2), 'us_max': round(max(us), 2),
            'windows': len(us)}


def _lattice(max_turns, dev):
    """(di, dj, code) of the window's directions, before the pitch says which of them exist."""
    dj, di = torch.meshgrid(torch.arange(-36, 37, device=dev), torch.arange(-36, 36, device=dev), indexing='ij')
    keep = di.abs() + dj.abs() <= max_turns
    di, dj = di[keep], dj[keep]
    return di, dj, ((di.abs() + dj.abs()) << 16 | (dj + 36) << 8 | (di + 36)).to(torch.int32)


def _today(env, max_turns, chunk_rows, planes):
    """The planes by replication + igw_action_mask + scatter-min, `chunk_rows` replicated rows at a time."""
    from gridworld_amd import aim as A, query as Q
    agent, _, occ = env._rows
    n, dev = env.num_envs, env.device
    di, dj, code = _lattice(max_turns, dev)
    D = int(di.numel())
    per = max(1, chunk_rows // D)
    poses = agent.view(torch.float64)                 # [n, 8]: x, y, z, yaw, pitch, dy, 16 bytes of integers
    big = torch.iinfo(torch.int32).max
    for lo in range(0, n, per):
        m = min(per, n - lo)
        pitch_d = poses[lo:lo + m, 4:5] + 5.0 * dj
        e, d = ((pitch_d >= -90.0) & (pitch_d <= 90.0)).nonzero(as_tuple=True)     # the directions that exist, env by env
        rep = poses[lo + e]
        rep[:, 3] += 5.0 * di[d]
        rep[:, 4] = pitch_d[e, d]
        occ_rep = occ[lo + e]
        copies = int(e.numel())
        mask = torch.empty((copies, Q.ACTIONS), dtype=torch.uint8, device=dev)
        look = torch.empty((copies, 2), dtype=torch.int16, device=dev)
        Q.action_mask_into(rep.data_ptr(), occ_rep.data_ptr(), copies, env.select_and_place, mask.data_ptr(),
                           look.data_ptr(), None, 0, 0, 0, env._stream())
        look = look.long()
        for k, col in (('break', 0), ('place', 1)):
            cell = e * A.ROW + torch.where(look[:, col] >= 0, look[:, col], torch.full_like(look[:, col], A.ROW - 1))
            rows = torch.full((m * A.ROW,), big, dtype=torch.int32, device=dev)
            rows.scatter_reduce_(0, cell, code[d], 'amin')
            rows = rows.view(m, A.ROW)
            rows[:, A.CELLS:] = big
            planes[k][lo:lo + m] = torch.where(rows == big, torch.full_like(rows, -1), rows)
    return planes


def bench(n, iters, slow_iters, warmup, repeats, chunk_rows):
    from gridworld_amd import VecGridWorld, aim as A, workloads
    env = VecGridWorld(n, autoreset=True, num_tasks=TASKS)
    env.set_tasks(workloads.rt20(TASKS, seed=1).numpy(), env_task=torch.arange(n, dtype=torch.int32) % TASKS)
    env.reset()
    acts = env.fill_actions(60, seed=3)
    for t in range(60):
        env.step(acts[t])
    out = {k: A.plane(n, env.device) for k in ('place', 'break')}
    rows = {k: torch.empty((n, A.ROW), dtype=torch.int32, device=env.device) for k in ('place', 'break')}
    saved = env.state_dict()
    state = {'t': 0}

    def step():
        env.step(acts[state['t'] % 60])
        state['t'] += 1
    res = {'envs': n, 'task_rows': TASKS, 'windows': []}
    for max_turns in WINDOWS:
        env.load_state_dict(saved)
        dj = _lattice(max_turns, env.device)[1]
        lattice = int(dj.numel())
        pitch_d = env._rows[0].view(torch.float64)[:, 4:5] + 5.0 * dj     # the directions that exist: what igw_aim marches
        rays = int(((pitch_d >= -90.0) & (pitch_d <= 90.0)).sum())
        variants = {'aim': (lambda: env.aim(max_turns=max_turns, out=out), iters),
                    'step': (step, iters),
                    'today': (lambda: _today(env, max_turns, chunk_rows, rows), slow_iters)}
        us = {k: [] for k in variants}
        for r in range(repeats):
            for k, (fn, it) in variants.items():
                if k == 'today':
                    env.load_state_dict(saved)      # (the steps in between moved the state; both answer the same one)
                us[k].append(BR._time(fn, it, warmup if r == 0 else 1))
        env.load_state_dict(saved)
        got = env.aim(max_turns=max_turns, out=out)
        w = {k: _spread(v) for k, v in us.items()}
        med = lambda k: w[k]['us_median']  # noqa: E731
        w.update(max_turns=max_turns, lattice_directions=lattice, rays=rays, rays_per_env=round(rays / n, 1),
                 reachable_place_cells_per_env=round(float((got['place'] >= 0).sum()) / n, 2),
                 reachable_break_cells_per_env=round(float((got['break'] >= 0).sum()) / n, 2),
                 aim_over_step=round(med('aim') / med('step'), 3), today_over_aim=round(med('today') / med('aim'), 1),
                 aim_ns_per_ray=round(med('aim') * 1e3 / rays, 4))
        res['windows'].append(w)
    del env, saved, out, rows
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--envs', default='4096,65536')
    ap.add_argument('--iters', type=int, default=20, help='launches per window of aim / step')
    ap.add_argument('--slow-iters', type=int, default=1, help='rounds per window of today')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--chunk-rows', type=int, default=1 << 24, help='replicated rows per igw_action_mask launch of today')
    ap.add_argument('--git-commit', default=None, help='the commit to stamp (default: git rev-parse HEAD)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_aim.py needs a GPU')
    from gridworld_amd import _lib as L, aim as A
    line = {'tool': 'tools/bench_aim.py', 'aim_build_id': A.build_id(), 'build_id': L.build_id(),
            'git_commit': a.git_commit or BR._git_commit(), 'device': torch.cuda.get_device_name(0), 'sizes': []}
    for n in a.envs.split(','):
        line['sizes'].append(bench(int(n), a.iters, a.slow_iters, a.warmup, max(1, a.repeats), a.chunk_rows))
    BR._emit(line, a.out)


if __name__ == '__main__':
    main()
