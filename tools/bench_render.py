#!/usr/bin/env python3
"""Throughput of the first-person renderer (libigw_render.so) on one MI355X; prints one JSON line (and writes it to
--out).  Timings are HIP-event windows after warm-up:

  render   N envs x 64 x 64 RGB, one igw_render_pov launch per frame batch: us per launch, frames / s, and the
           write bound (N*H*W*C bytes over the 8 TB/s HBM peak and over the 6.29 TB/s a streaming kernel reaches)
  step     at 65,536 envs: walking step alone vs step + render (what VecGridWorld(renderer='hip') costs per step)
  facade   the 1-env gym facade: step without pov vs with pov (host wall clock, each step ends in a synchronise)

    python tools/bench_render.py [--envs 1,4096,65536,524288] [--iters 50] [--out profiles/r07_render_bench.json]

--mode episodes measures the log frames (igw_render_episodes) instead, on episodes of --steps walking steps logged
for --episodes envs (default 4,096 x 250: 1.03 M frames of 64 x 64 RGB):

  episodes  one igw_render_episodes launch over all of them: us per launch, frames / s
  logged64  the frames of 64 logged envs two ways: igw_render_pov of the 64 rows after every step (--steps launches,
            summed) against one igw_render_episodes launch for the 64 finished episodes

    python tools/bench_render.py --mode episodes [--out profiles/r08_render_episodes_bench.json]

--mode views measures the free-camera views (igw_render_views), each shape one launch, and, in the same process,
igw_render_pov on as many 64 x 64 frames as shape (a) as the yardstick, --repeats times each for the run-to-run spread:

  a  4,096 grids x 8 look-at views at 64 x 64     b  64 grids x 8 views at 512 x 512     c  1 grid x 180 orbit views at
  640 x 640: ms per launch, frames / s, megapixels / s

    python tools/bench_render.py --mode views [--out profiles/r09_render_views_bench.json]

--mode aux measures the planes (igw_render_*_aux: depth, label, surface; DESIGN.md section 8 "Planes"), in one
process, as medians of --repeats runs with the min - max spread:

  colour_only  the three colour-only entries: igw_render_pov at 65,536 envs x 64 x 64, igw_render_episodes on
               --episodes x --steps logged steps, igw_render_views on shape (a)
  aux          igw_render_pov_aux at 65,536 envs with colour and all three planes, and with the planes alone;
               igw_render_views_aux on shape (a) with colour and planes

--mode ab --lib PATH measures the three colour-only entries on the package's library and on the one at PATH,
alternating in ONE process over the same buffers (this, parent, this, parent, ...), --repeats times each.

--lib PATH measures another build of libigw_render.so (the parent commit's, say) in place of the package's: the
colour_only part runs on any build, the aux part only where the library has the entries.

    python tools/bench_render.py --mode aux [--lib parent/libigw_render.so] [--out profiles/r10_render_aux_bench.json]

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


def _logged_episodes(n, steps):
    """n walking envs stepped `steps` times with the whole batch logged (max_steps = steps, so every env finishes one
    episode at the last step): (env, records, device arrays first / length / frame0 / start / pose of the finished
    episodes, frames)."""
    from gridworld_amd import VecGridWorld, workloads
    env = VecGridWorld(n, max_steps=steps, autoreset=True)
    rng = np.random.RandomState(2)
    pose = np.stack([rng.uniform(-8, 8, n), rng.uniform(0, 4, n), rng.uniform(-8, 8, n), rng.uniform(-180, 180, n),
                     rng.uniform(-60, 60, n)], 1)
    env.set_tasks(workloads.rt20(n, seed=2).numpy(), workloads.uniform20(n, seed=2).numpy(), init_pose=pose)
    rec, heads = env.enable_trajectory_log(n, steps)
    env.reset()
    acts = env.fill_actions(steps, seed=5)
    for t in range(steps):
        env.step_walking_ptr(acts[t])
    torch.cuda.synchronize()
    h = heads.cpu().numpy()
    slot = np.argmax(h[:, :, 3], axis=1)                  # the slot whose episode finished
    assert (h[np.arange(n), slot, 3] == 1).all() and (h[np.arange(n), slot, 1] == steps).all()
    task = h[np.arange(n), slot, 0].astype(np.int64)
    dev = env.device
    rows = torch.from_numpy(task).to(dev)
    arrays = dict(first=torch.from_numpy((np.arange(n) * 2 + slot) * steps).to(dev),
                  length=torch.full((n,), steps, dtype=torch.int32, device=dev),
                  frame0=torch.arange(n, dtype=torch.int64, device=dev) * (steps + 1),
                  start=env.task_start.index_select(0, rows),
                  pose=env.task_meta.index_select(0, rows)[:, :40].contiguous().view(torch.float64))
    return env, rec, arrays


def _episodes_call(env, rec, a, m, steps, out):
    from gridworld_amd import render as R
    stream = torch.cuda.current_stream().cuda_stream
    return lambda: R.render_episodes_into(rec.data_ptr(), rec.shape[0] * 2 * steps, a['first'].data_ptr(),
                                          a['length'].data_ptr(), a['frame0'].data_ptr(), a['start'].data_ptr(),
                                          a['pose'].data_ptr(), m, steps, env._atlas(), out.data_ptr(), out.shape[0],
                                          64, 64, 3, stream)


def bench_episodes(n, steps, iters, warmup):
    env, rec, a = _logged_episodes(n, steps)
    frames = n * (steps + 1)
    out = torch.empty((frames, 64, 64, 3), dtype=torch.uint8, device='cuda')
    us = _time(_episodes_call(env, rec, a, n, steps, out), iters, warmup)
    res = {'episodes': n, 'steps': steps, 'frames': frames, 'size': [64, 64], 'channels': 3,
           'us_per_launch': round(us, 1), 'frames_per_s': round(frames / (us * 1e-6), 1)}
    # 64 logged envs: one launch for their episodes, against igw_render_pov of the same 64 rows after every step
    out64 = torch.empty((64 * (steps + 1), 64, 64, 3), dtype=torch.uint8, device='cuda')
    one = _time(_episodes_call(env, rec, a, 64, steps, out64), iters, warmup)
    live = torch.empty((64, 64, 64, 3), dtype=torch.uint8, device='cuda')
    from gridworld_amd import render as R
    stream = torch.cuda.current_stream().cuda_stream
    rows64 = (env.agent_buf.data_ptr(), env.grid_buf.data_ptr(), env.occ_buf.data_ptr(), 64)
    per_step = _time(lambda: R.render_into(*rows64, env._atlas(), live.data_ptr(), 64, 64, 3, stream), iters * 5,
                     warmup)
    res['logged64'] = {'episodes': 64, 'frames': 64 * (steps + 1),
                       'render_pov_us_per_launch': round(per_step, 2),
                       'render_pov_every_step_us': round(per_step * steps, 1),
                       'render_episodes_one_launch_us': round(one, 1),
                       'speedup': round(per_step * steps / one, 2)}
    return res


def _spread(us):
    return {'us_per_launch_median': round(float(np.median(us)), 1), 'us_per_launch_min': round(min(us), 1),
            'us_per_launch_max': round(max(us), 1), 'repeats': len(us)}


def bench_views(iters, warmup, repeats):
    import gridworld_amd as G
    from gridworld_amd import workloads
    dev = torch.device('cuda', torch.cuda.current_device())
    atlas = torch.from_numpy(G.render.default_atlas()).to(dev)
    centre = (0.0, 1.5, 0.0)
    shapes = (('a', 4096, 8, (64, 64), G.orbit_poses(centre, 12, 4.5, 8, phase=10)),
              ('b', 64, 8, (512, 512), G.orbit_poses(centre, 12, 4.5, 8, phase=10)),
              ('c', 1, 180, (640, 640), G.orbit_poses(centre, 14, 5.5, 180)))
    res = {}
    for name, n_grids, per_grid, (W, H), ring in shapes:
        grids = workloads.uniform20(n_grids, seed=6).to(device=dev, dtype=torch.int8).reshape(n_grids, 1089).contiguous()
        m = n_grids * per_grid
        poses = torch.from_numpy(np.tile(ring, (n_grids, 1))).to(dev)
        view_grid = torch.arange(n_grids, dtype=torch.int32, device=dev).repeat_interleave(per_grid)
        out = torch.empty((m, H, W, 3), dtype=torch.uint8, device=dev)
        it = max(3, iters // 5) if W > 64 else iters
        us = [_time(lambda: G.render_views(grids, poses, view_grid=view_grid, size=(W, H), atlas=atlas, out=out), it,
                    warmup) for _ in range(repeats)]
        med = float(np.median(us))
        res[name] = dict(_spread(us), grids=n_grids, views=m, size=[W, H], channels=3,
                         ms_per_launch=round(med * 1e-3, 3), frames_per_s=round(m / (med * 1e-6), 1),
                         megapixels_per_s=round(m * W * H / med, 1))
        del out
        torch.cuda.empty_cache()
    # the yardstick: igw_render_pov on as many 64 x 64 frames as (a), eyes inside the zone (a task's init_pose)
    n = 4096 * 8
    env = _batch(n)
    out = torch.empty((n, 64, 64, 3), dtype=torch.uint8, device=dev)
    us = [_time(lambda: env.render_pov(out=out), iters, warmup) for _ in range(repeats)]
    med = float(np.median(us))
    res['pov_yardstick'] = dict(_spread(us), envs=n, size=[64, 64], channels=3, ms_per_launch=round(med * 1e-3, 3),
                                frames_per_s=round(n / (med * 1e-6), 1), megapixels_per_s=round(n * 4096 / med, 1))
    # the same scenes both ways: the views kernel on the batch's own grids from the agents' own poses
    torch.cuda.synchronize()
    own = torch.from_numpy(np.ascontiguousarray(env.agent_buf.cpu().numpy()[:, :40]).view(np.float64)).to(dev)
    us = [_time(lambda: env.render_views(own, out=out), iters, warmup) for _ in range(repeats)]
    med = float(np.median(us))
    res['views_of_the_yardstick_scenes'] = dict(_spread(us), views=n, size=[64, 64], channels=3,
                                                ms_per_launch=round(med * 1e-3, 3),
                                                frames_per_s=round(n / (med * 1e-6), 1),
                                                megapixels_per_s=round(n * 4096 / med, 1))
    return res


def _views_a(dev):
    """Shape (a) of bench_views: 4,096 grids x 8 look-at views at 64 x 64 (grids, poses, view_grid, atlas)."""
    import gridworld_amd as G
    from gridworld_amd import workloads
    ring = G.orbit_poses((0.0, 1.5, 0.0), 12, 4.5, 8, phase=10)
    grids = workloads.uniform20(4096, seed=6).to(device=dev, dtype=torch.int8).reshape(4096, 1089).contiguous()
    poses = torch.from_numpy(np.tile(ring, (4096, 1))).to(dev)
    view_grid = torch.arange(4096, dtype=torch.int32, device=dev).repeat_interleave(8)
    return grids, poses, view_grid, torch.from_numpy(G.render.default_atlas()).to(dev)


def bench_aux(iters, warmup, repeats, episodes, steps):
    import gridworld_amd as G
    from gridworld_amd import render as R
    dev = torch.device('cuda', torch.cuda.current_device())
    have_aux = hasattr(R.load(), 'igw_render_pov_aux')
    n = 65536
    pix = n * 4096

    def timed(fn, its=iters, frames=n):
        us = [_time(fn, its, warmup) for _ in range(repeats)]
        med = float(np.median(us))
        return dict(_spread(us), ms_per_launch=round(med * 1e-3, 3), frames_per_s=round(frames / (med * 1e-6), 1))
    colour, aux = {}, {}
    env = _batch(n)
    rgb = torch.empty((n, 64, 64, 3), dtype=torch.uint8, device=dev)
    colour['pov'] = dict(timed(lambda: env.render_pov(out=rgb)), envs=n, size=[64, 64], channels=3)
    if have_aux:
        planes = {'depth': torch.empty((n, 64, 64), dtype=torch.float32, device=dev),
                  'label': torch.empty((n, 64, 64), dtype=torch.uint8, device=dev),
                  'surface': torch.empty((n, 64, 64), dtype=torch.int16, device=dev)}
        both = dict(planes, rgb=rgb)
        aux['pov_aux_colour_and_planes'] = dict(
            timed(lambda: env.render_pov(out=both, outputs=('rgb', 'depth', 'label', 'surface'))), envs=n,
            plane_bytes=7 * pix, plane_store_bound_ms_at_stream_rate=round(7 * pix / HBM_STREAM * 1e3, 3))
        aux['pov_aux_planes_only'] = dict(timed(lambda: env.render_pov(out=planes,
                                                                         outputs=('depth', 'label', 'surface'))), envs=n)
        for k in ('depth', 'label', 'surface'):
            one = {k: planes[k]}
            aux['pov_aux_' + k + '_only'] = dict(timed(lambda: env.render_pov(out=one, outputs=(k,))), envs=n)
        del planes, both
    del env
    torch.cuda.empty_cache()
    # views, shape (a)
    grids, poses, view_grid, atlas = _views_a(dev)
    m = poses.shape[0]
    out = torch.empty((m, 64, 64, 3), dtype=torch.uint8, device=dev)
    colour['views_a'] = dict(timed(lambda: G.render_views(grids, poses, view_grid=view_grid, atlas=atlas, out=out),
                                   frames=m), views=m, size=[64, 64], channels=3)
    if have_aux:
        both = {'rgb': out, 'depth': torch.empty((m, 64, 64), dtype=torch.float32, device=dev),
                'label': torch.empty((m, 64, 64), dtype=torch.uint8, device=dev),
                'surface': torch.empty((m, 64, 64), dtype=torch.int16, device=dev)}
        aux['views_a_aux_colour_and_planes'] = dict(
            timed(lambda: G.render_views(grids, poses, view_grid=view_grid, atlas=atlas, out=both,
                                         outputs=('rgb', 'depth', 'label', 'surface')), frames=m), views=m)
        del both
    del out, grids, poses
    torch.cuda.empty_cache()
    # episodes
    env, rec, a = _logged_episodes(episodes, steps)
    frames = episodes * (steps + 1)
    out = torch.empty((frames, 64, 64, 3), dtype=torch.uint8, device=dev)
    colour['episodes'] = dict(timed(_episodes_call(env, rec, a, episodes, steps, out), its=max(3, iters // 5),
                                    frames=frames), episodes=episodes, steps=steps, frames=frames)
    res = {'colour_only': colour}
    if have_aux:
        res['aux'] = aux
    return res


def bench_ab(iters, warmup, repeats, episodes, steps, other):
    """The three colour-only entries on the package's library and on `other` (a CDLL of another build), ALTERNATING
    in one process over the same buffers: this, other, this, other, ... `repeats` times each, so that whatever drifts
    between processes or over a session falls on both alike."""
    import gridworld_amd as G
    from gridworld_amd import render as R
    dev = torch.device('cuda', torch.cuda.current_device())
    mine = R.load()
    n = 65536
    env = _batch(n)
    rgb = torch.empty((n, 64, 64, 3), dtype=torch.uint8, device=dev)
    grids, poses, view_grid, atlas = _views_a(dev)
    vout = torch.empty((poses.shape[0], 64, 64, 3), dtype=torch.uint8, device=dev)
    lenv, rec, a = _logged_episodes(episodes, steps)
    eout = torch.empty((episodes * (steps + 1), 64, 64, 3), dtype=torch.uint8, device=dev)
    calls = {'pov': (lambda: env.render_pov(out=rgb), iters),
             'views_a': (lambda: G.render_views(grids, poses, view_grid=view_grid, atlas=atlas, out=vout), iters),
             'episodes': (_episodes_call(lenv, rec, a, episodes, steps, eout), max(3, iters // 5))}
    res = {}
    for name, (fn, its) in calls.items():
        us = {'this': [], 'parent': []}
        for _ in range(repeats):
            for who, lib in (('this', mine), ('parent', other)):
                R.BINDING.lib = lib
                us[who].append(_time(fn, its, warmup))
        R.BINDING.lib = mine
        res[name] = {who: _spread(v) for who, v in us.items()}
        res[name]['this_median_within_parent_spread_or_faster'] = \
            res[name]['this']['us_per_launch_median'] <= res[name]['parent']['us_per_launch_max']
    return res


def _use_library(path):
    """Binds another build of libigw_render.so in place of the package's (whatever entries it has)."""
    import ctypes
    from gridworld_amd import render as R
    lib = ctypes.CDLL(os.path.abspath(path))
    for name, (res, args) in R.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    R.BINDING.lib = lib


def _git_commit():
    import subprocess
    try:
        return subprocess.check_output(['git', 'rev-parse', 'HEAD'], cwd=ROOT, text=True,
                                       stderr=subprocess.DEVNULL).strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', default='1,4096,65536,524288')
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--facade-steps', type=int, default=500)
    ap.add_argument('--skip', default='', help='comma list of parts to skip: step, facade')
    ap.add_argument('--out', default=None)
    ap.add_argument('--mode', default='render', choices=('render', 'episodes', 'views', 'aux', 'ab'))
    ap.add_argument('--lib', default=None, help='another build of libigw_render.so to measure instead of the package\'s')
    ap.add_argument('--repeats', type=int, default=5, help='--mode views: repeats of every measurement')
    ap.add_argument('--git-commit', default=None, help='--mode views: the commit to stamp (default: git rev-parse)')
    ap.add_argument('--episodes', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=250)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_render.py needs a GPU')
    from gridworld_amd import render as R, build as B
    skip = set(filter(None, a.skip.split(',')))
    if a.mode == 'ab':
        if not a.lib:
            sys.exit('--mode ab needs --lib, the other build')
        mine = R.load()
        _use_library(a.lib)
        other, R.BINDING.lib = R.BINDING.lib, mine
        line = {'tool': 'tools/bench_render.py', 'render_build_id': R.build_id(),
                'parent_render_build_id': other.igw_render_build_id().decode(),
                'device': torch.cuda.get_device_name(0),
                'colour_only_alternating': bench_ab(a.iters, a.warmup, max(1, a.repeats), a.episodes, a.steps, other)}
        return _emit(line, a.out)
    if a.lib:
        _use_library(a.lib)
    line = {'tool': 'tools/bench_render.py', 'render_build_id': R.build_id(), 'step_build_id': B.source_hash(),
            'device': torch.cuda.get_device_name(0)}
    if a.mode == 'views':
        line['git_commit'] = a.git_commit or _git_commit()
        line['views'] = bench_views(a.iters, a.warmup, max(1, a.repeats))
        return _emit(line, a.out)
    if a.mode == 'aux':
        line['git_commit'] = a.git_commit or _git_commit()
        line['aux_bench'] = bench_aux(a.iters, a.warmup, max(1, a.repeats), a.episodes, a.steps)
        return _emit(line, a.out)
    if a.mode == 'episodes':
        line['episodes'] = bench_episodes(a.episodes, a.steps, a.iters, a.warmup)
        return _emit(line, a.out)
    line['render'] = []
    for n in [int(v) for v in a.envs.split(',')]:
        try:
            line['render'].append(bench_render(n, a.iters, a.warmup))
        except torch.cuda.OutOfMemoryError as e:
            line['render'].append({'envs': n, 'skipped': 'out of memory: %s' % str(e)[:80]})
    if 'step' not in skip:
        line['step'] = bench_step(65536, a.iters, a.warmup)
    if 'facade' not in skip:
        line['facade'] = bench_facade(a.facade_steps)
    _emit(line, a.out)


def _emit(line, out):
    s = json.dumps(line)
    print(s)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write(s + '\n')


if __name__ == '__main__':
    main()
