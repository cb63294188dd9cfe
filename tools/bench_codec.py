#!/usr/bin/env python3
"""Cost of the JPEG encoder (libigw_codec.so) next to the ray caster that feeds it, on one MI355X; prints one JSON line
and writes it to --out.  Every figure is the median of --repeats HIP-event windows of --iters launches after warm-up,
with the min - max spread; render and encode run in the same process on the same frames:

  pov       65,536 envs x 64 x 64 RGB of a stepped rt20 batch: igw_render_pov, then igw_jpeg_encode of those frames
  episodes  --episodes x (--steps + 1) logged frames (default 4,096 x 251): igw_render_episodes, then the encode
  views     64 grids x 512 x 512 look-at views: igw_render_views, then the encode

Per shape: ms per launch of both, frames / s, the bytes in (raw RGB) and out (the sum of the streams' sizes), their
ratio, and encode / render.  The kernel's VGPRs, LDS and scratch are read from the code object inside the library.

    python tools/bench_codec.py [--quality 90] [--out profiles/r11_codec_bench.json]

A profiler's kernel trace belongs in a run of its own (rocprofv3 --kernel-trace --stats -- python tools/bench_codec.py
--shapes pov --repeats 1).
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_render as BR  # noqa: E402


def _median(fn, iters, warmup, repeats):
    ms = [BR._time(fn, iters, warmup if k == 0 else 1) / 1e3 for k in range(repeats)]
    return {'ms_per_launch_median': round(float(np.median(ms)), 4), 'ms_per_launch_min': round(min(ms), 4),
            'ms_per_launch_max': round(max(ms), 4), 'repeats': repeats, 'iters': iters}


def _encode_side(frames, quality, iters, warmup, repeats):
    """The encode of `frames` (device uint8 [n, H, W, 3]) into preallocated slots of the default stride."""
    from gridworld_amd import codec as K
    n, H, W, _ = frames.shape
    buf = torch.empty((n, K.default_stride(W, H)), dtype=torch.uint8, device=frames.device)
    sizes = torch.empty((n,), dtype=torch.int32, device=frames.device)
    run = lambda: K.encode_jpeg(frames, quality, out=(buf, sizes), check_sizes=False)  # noqa: E731
    res = _median(run, iters, warmup, repeats)
    s = sizes.cpu().numpy().astype(np.int64)
    raw = int(n) * H * W * 3
    res.update(stride=int(buf.shape[1]), streams_that_did_not_fit=int((s < 0).sum()), bytes_in=raw,
               bytes_out=int(np.abs(s).sum()), largest_stream=int(np.abs(s).max()),
               bytes_out_over_in=round(float(np.abs(s).sum()) / raw, 4))
    return res


def _shape(name, frames, render, quality, iters, warmup, repeats):
    r = _median(render, iters, warmup, repeats)
    e = _encode_side(frames, quality, iters, warmup, repeats)
    n = int(frames.shape[0])
    r['frames_per_s'] = round(n / (r['ms_per_launch_median'] * 1e-3), 1)
    e['frames_per_s'] = round(n / (e['ms_per_launch_median'] * 1e-3), 1)
    return {'shape': name, 'frames': n, 'size': [int(frames.shape[2]), int(frames.shape[1])], 'render': r, 'encode': e,
            'encode_over_render': round(e['ms_per_launch_median'] / r['ms_per_launch_median'], 3)}


def bench_pov(n, quality, iters, warmup, repeats):
    env = BR._batch(n)
    acts = env.fill_actions(60, seed=3)
    for t in range(60):
        env.step_walking_ptr(acts[t])
    frames = torch.empty((n, 64, 64, 3), dtype=torch.uint8, device='cuda')
    res = _shape('pov', frames, lambda: env.render_pov(out=frames), quality, iters, warmup, repeats)
    res['envs'] = n
    return res


def bench_episodes(n, steps, quality, iters, warmup, repeats):
    env, rec, a = BR._logged_episodes(n, steps)
    frames = torch.empty((n * (steps + 1), 64, 64, 3), dtype=torch.uint8, device='cuda')
    res = _shape('episodes', frames, BR._episodes_call(env, rec, a, n, steps, frames), quality, iters, warmup, repeats)
    res.update(episodes=n, steps=steps)
    return res


def bench_views(quality, iters, warmup, repeats):
    import gridworld_amd as G
    from gridworld_amd import workloads
    grids = workloads.rt20(64, seed=4).to('cuda')
    poses = np.stack([np.array([*e, *G.look_at(e, (0, 1, 0))]) for e in
                      ((9 * np.cos(k), 4 + k % 3, 9 * np.sin(k)) for k in range(64))])
    frames = torch.empty((64, 512, 512, 3), dtype=torch.uint8, device='cuda')
    p = torch.from_numpy(poses).to('cuda')
    return _shape('views', frames, lambda: G.render_views(grids, p, size=(512, 512), out=frames), quality, iters,
                  warmup, repeats)


def code_object():
    """VGPRs, SGPRs, LDS and scratch of igw_jpeg_encode_kernel, from the gfx950 code object inside the library."""
    from gridworld_amd import codec as K
    llvm = '/opt/rocm/lib/llvm/bin'
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, 'fat.bin'), os.path.join(d, 'dev.co')
        try:
            subprocess.check_call([f'{llvm}/llvm-objcopy', '--dump-section', '.hip_fatbin=' + fat, K.LIB])
            subprocess.check_call([f'{llvm}/clang-offload-bundler', '--type=o', '--input=' + fat, '--output=' + co,
                                   '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--unbundle'])
            notes = subprocess.check_output([f'{llvm}/llvm-readelf', '--notes', co], text=True)
        except (OSError, subprocess.CalledProcessError) as e:
            return {'error': str(e)}
    kern = [b for b in notes.split('- .agpr_count:')[1:] if 'igw_jpeg_encode_kernel' in b][0]
    val = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, kern).group(1))  # noqa: E731
    return {'vgpr_count': val('vgpr_count'), 'sgpr_count': val('sgpr_count'), 'lds_bytes': val('group_segment_fixed_size'),
            'scratch_bytes': val('private_segment_fixed_size'), 'vgpr_spill_count': val('vgpr_spill_count'),
            'sgpr_spill_count': val('sgpr_spill_count')}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--shapes', default='pov,episodes,views')
    ap.add_argument('--envs', type=int, default=65536)
    ap.add_argument('--episodes', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=250)
    ap.add_argument('--quality', type=int, default=90)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--git-commit', default=None, help='the commit to stamp (default: git rev-parse HEAD)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from gridworld_amd import codec as K, render as R
    line = {'tool': 'tools/bench_codec.py', 'codec_build_id': K.build_id(), 'render_build_id': R.build_id(),
            'git_commit': a.git_commit or BR._git_commit(), 'device': torch.cuda.get_device_name(0),
            'quality': a.quality, 'code_object': code_object(), 'shapes': []}
    for name in a.shapes.split(','):
        if name == 'pov':
            res = bench_pov(a.envs, a.quality, a.iters, a.warmup, a.repeats)
        elif name == 'episodes':
            res = bench_episodes(a.episodes, a.steps, a.quality, a.iters, a.warmup, a.repeats)
        elif name == 'views':
            res = bench_views(a.quality, a.iters, a.warmup, a.repeats)
        else:
            raise SystemExit(f'unknown shape {name!r}')
        line['shapes'].append(res)
        torch.cuda.empty_cache()
    BR._emit(line, a.out)


if __name__ == '__main__':
    main()
