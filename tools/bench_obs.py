#!/usr/bin/env python3
"""Cost of the training-layout observation (igw_render_pov_obs; DESIGN.md section 8, "Training-layout observations")
on one MI355X; prints one JSON line and writes it to --out.  The batch is 65,536 envs x 64 x 64 of a stepped rt20 batch.
Per configuration (grey u8 K = 4, RGB f16 K = 1, RGB u8 K = 4) four variants are measured ALTERNATELY in one process
(a, b, c, d, a, b, ... --repeats times each), every figure the median of its HIP-event windows of --iters launches
with the min - max spread:

  fused_with_frame   one igw_render_pov_obs launch writing the frame and shifting the stack in place
  fused_no_frame     the same with out = NULL
  today              render_pov(), then the torch ops of tests/obs_model.py on the device (the route a user has today)
  render_pov_alone   the frame alone

--lib PATH also measures the colour-only entries of libigw_render.so on this build and on the library at PATH (the
parent commit's), alternating in the same way (tools/bench_render.py: bench_ab).

    python tools/bench_obs.py [--lib parent/libigw_render.so] [--out profiles/r12_obs_bench.json]

A profiler's kernel trace belongs in a run of its own (rocprofv3 --kernel-trace --stats -- python tools/bench_obs.py
--configs grey_u8_k4 --repeats 1).
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import bench_render as BR  # noqa: E402

CONFIGS = {'grey_u8_k4': dict(gray=True, stack=4),
           'rgb_f16_k1': dict(dtype='float16', scale=1 / 255),
           'rgb_u8_k4': dict(stack=4)}


def _spread(ms):
    return {'ms_per_launch_median': round(float(np.median(ms)), 4), 'ms_per_launch_min': round(min(ms), 4),
            'ms_per_launch_max': round(max(ms), 4), 'repeats': len(ms)}


def bench_config(env, name, iters, warmup, repeats):
    import obs_model as OM
    from gridworld_amd import render as R
    spec = R.ObsSpec(**CONFIGS[name])
    n = env.num_envs
    frame = torch.empty((n, 64, 64, 3), dtype=torch.uint8, device=env.device)
    stack = env.render_pov_obs(spec)
    state = {'prev': OM.observe(env.render_pov(out=frame), None, None, spec)}

    def today():
        state['prev'] = OM.observe(env.render_pov(out=frame), state['prev'], env.done, spec)
    variants = {'fused_with_frame': lambda: env.render_pov_obs(spec, out=stack, restart=env.done, frame=frame),
                'fused_no_frame': lambda: env.render_pov_obs(spec, out=stack, restart=env.done),
                'today': today,
                'render_pov_alone': lambda: env.render_pov(out=frame)}
    ms = {k: [] for k in variants}
    for r in range(repeats):
        for k, fn in variants.items():
            ms[k].append(BR._time(fn, iters, warmup if r == 0 else 1) / 1e3)
    res = {k: _spread(v) for k, v in ms.items()}
    med = lambda k: res[k]['ms_per_launch_median']  # noqa: E731
    elem = torch.empty((), dtype=spec.dtype).element_size()
    res.update(config=name, spec=repr(spec), envs=n, size=[64, 64],
               stack_bytes=int(np.prod(spec.shape(n, (64, 64)))) * elem,
               shift_traffic_bytes=2 * (spec.stack - 1) * spec.planes * n * 4096 * elem,
               today_over_fused_with_frame=round(med('today') / med('fused_with_frame'), 3),
               fused_beats_today_with_spreads_apart=res['fused_with_frame']['ms_per_launch_max']
               < res['today']['ms_per_launch_min'],
               fused_with_frame_minus_render_pov_ms=round(med('fused_with_frame') - med('render_pov_alone'), 4),
               fused_no_frame_minus_render_pov_ms=round(med('fused_no_frame') - med('render_pov_alone'), 4))
    del stack, frame, state
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--configs', default=','.join(CONFIGS))
    ap.add_argument('--envs', type=int, default=65536)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--lib', default=None, help='the parent build of libigw_render.so, for the colour-only comparison')
    ap.add_argument('--episodes', type=int, default=512, help='--lib: logged episodes of the episodes entry')
    ap.add_argument('--steps', type=int, default=250)
    ap.add_argument('--git-commit', default=None, help='the commit to stamp (default: git rev-parse HEAD)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_obs.py needs a GPU')
    from gridworld_amd import render as R
    line = {'tool': 'tools/bench_obs.py', 'render_obs_build_id': R.OBS_BINDING.build_id(),
            'render_build_id': R.build_id(),
            'git_commit': a.git_commit or BR._git_commit(), 'device': torch.cuda.get_device_name(0), 'configs': []}
    env = BR._batch(a.envs)
    acts = env.fill_actions(60, seed=3)
    for t in range(60):
        env.step_walking_ptr(acts[t])
    for name in a.configs.split(','):
        if name not in CONFIGS:
            raise SystemExit(f'unknown config {name!r}; the configs are {list(CONFIGS)}')
        line['configs'].append(bench_config(env, name, a.iters, a.warmup, max(1, a.repeats)))
    del env
    torch.cuda.empty_cache()
    if a.lib:
        mine = R.load()
        BR._use_library(a.lib)
        other, R.BINDING.lib = R.BINDING.lib, mine
        line['parent_render_build_id'] = other.igw_render_build_id().decode()
        line['colour_only_alternating'] = BR.bench_ab(a.iters, a.warmup, max(1, a.repeats), a.episodes, a.steps, other)
    BR._emit(line, a.out)


if __name__ == '__main__':
    main()
