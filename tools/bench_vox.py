#!/usr/bin/env python3
"""Cost of the voxel observation (igw_vox_obs) on one MI355X; prints one JSON line and writes it
to --out.  The batch is a stepped rt20 batch of 4,096 and of 65,536 envs.  Per spec three variants are measured
ALTERNATELY in one process (a, b, c, a, b, ... --repeats times each), every figure the median of its HIP-event windows
of --iters calls with the min - max spread:

  vox_obs   env.vox_obs(spec, out=..., restart=env.done): one launch, shifted in place
  today     the torch composition a user writes today for the same tensor (today() below: the fewest kernels we found --
            per one-hot plane one broadcast compare and one converting copy into the output's channels, the target rows
            by one gather of the user-target table, the agent's cells by one scatter_add, the agent's frame by one
            padded gather with a per-env index, the stack by one cat on the previous stack; the restart rule is left
            out of it, which favours it).  Checked equal to tests/vox_model.py once per spec, on the first 64 envs.
  step      env.step() alone, for scale

--lib PATH[,PATH] adds `vox_obs_other0` (and 1): the same call through other builds of libigw_vox.so (the A/B arms
-DIGW_VOX_NT_STORES=0 / 2 of the non-temporal stores, say), alternating with the rest.

    python tools/bench_vox.py [--lib other/libigw_vox.so] [--out profiles/r18_vox_bench.json]
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

HBM_PEAK = 8.0e12
BASE = dict(planes=(('grid', 'onehot'), ('target', 'onehot')), agent=True)
SPECS = {'world_u8_k1': dict(BASE),
         'world_f16_k1': dict(BASE, dtype='float16'),
         'world_f16_k4': dict(BASE, dtype='float16', stack=4),
         'ego5_f16_k1': dict(BASE, dtype='float16', frame='ego', radius=5)}
AHEAD = ((0, -1), (1, 0), (0, 1), (-1, 0))
RIGHT = ((1, 0), (0, 1), (-1, 0), (0, -1))


def _spread(us):
    return {'us_per_call_median': round(float(np.median(us)), 2), 'us_per_call_min': round(min(us), 2),
            'us_per_call_max': round(max(us), 2), 'repeats': len(us)}


class Today:
    """The torch composition for grid + target one-hot + agent; everything that does not depend on the state is made
    once, here."""

    def __init__(self, env, spec):
        n, dev = env.num_envs, env.device
        self.env, self.spec, self.n = env, spec, n
        self.cls = torch.arange(1, 7, dtype=torch.int8, device=dev).view(1, 6, 1, 1, 1)
        self.world = torch.empty((n, spec.channels, 9, 11, 11), dtype=spec.dtype, device=dev)
        self.off = torch.tensor([5, 1, 5], dtype=torch.int64, device=dev)
        self.dy = torch.tensor([0, -1], dtype=torch.int64, device=dev)
        self.ahead = torch.tensor(AHEAD, dtype=torch.int64, device=dev)
        self.right = torch.tensor(RIGHT, dtype=torch.int64, device=dev)
        s = spec.size
        self.s = (spec.radius - torch.arange(s, device=dev)).view(1, s, 1)
        self.t = (torch.arange(s, device=dev) - spec.radius).view(1, 1, s)
        self.prev = None

    def planes(self):
        env, n, w = self.env, self.n, self.world
        pose = env.agent_buf.view(torch.float64)
        target = torch.as_strided(env.user_target[env.env_task.long()], (n, 1, 9, 11, 11), (1104, 0, 121, 11, 1))
        w[:, 0:6].copy_(env.grid.unsqueeze(1) == self.cls)
        w[:, 6:12].copy_(target == self.cls)
        h = torch.round(pose[:, :3]).long() + self.off                    # (torch.round is round-half-even)
        y = h[:, 1:2] + self.dy                                            # [n, 2]: head and feet
        ok = ((h[:, 0:1] >= 0) & (h[:, 0:1] <= 10) & (h[:, 2:3] >= 0) & (h[:, 2:3] <= 10) & (y >= 0) & (y <= 8))
        cell = (y * 121 + h[:, 0:1] * 11 + h[:, 2:3]).clamp_(0, 1088)
        body = w[:, 12].view(n, 1089)
        body.zero_()
        body.scatter_add_(1, cell, ok.to(w.dtype))       # (a cell outside adds 0 to the cell it was clamped to)
        if self.spec.frame == 'world':
            return w
        q = (torch.floor((pose[:, 3] + 45.0) / 90.0) % 4).long()
        f, r = self.ahead[q], self.right[q]
        x = h[:, 0].view(n, 1, 1) + self.s * f[:, 0].view(n, 1, 1) + self.t * r[:, 0].view(n, 1, 1)
        z = h[:, 2].view(n, 1, 1) + self.s * f[:, 1].view(n, 1, 1) + self.t * r[:, 1].view(n, 1, 1)
        inside = (x >= 0) & (x <= 10) & (z >= 0) & (z <= 10)
        idx = torch.where(inside, x * 11 + z, torch.full_like(x, 121))
        c, s = self.spec.channels, self.spec.size
        padded = torch.nn.functional.pad(w.view(n, c, 9, 121), (0, 1))
        return padded.gather(3, idx.view(n, 1, 1, s * s).expand(n, c, 9, s * s)).view(n, c, 9, s, s)

    def __call__(self):
        new = self.planes()
        k, c = self.spec.stack, self.spec.channels
        if k == 1:
            self.prev = new
        elif self.prev is None:
            self.prev = new.repeat(1, k, 1, 1, 1)
        else:
            self.prev = torch.cat([self.prev[:, c:], new], 1)
        return self.prev


def check_today(env, spec):
    """today()'s newest slot equals the model on the first 64 envs."""
    import vox_model as VM
    got = Today(env, spec)()[:64, -spec.channels:].cpu()
    src = {'target': env.user_target[env.env_task.long()][:64, :1089].cpu().numpy()}
    one = type(spec)(planes=spec.planes, agent=spec.agent, frame=spec.frame, radius=spec.radius, dtype=spec.dtype)
    want = VM.observe(VM.planes(env.grid[:64].cpu().numpy(), env.internals()[:64, :4], src, one), None, None, one)
    assert torch.equal(VM.bits(got.contiguous()), VM.bits(want)), f'today() differs from the model for {spec}'
    kernel = env.vox_obs(one)[:64].cpu()
    assert torch.equal(VM.bits(kernel), VM.bits(want)), f'vox_obs differs from the model for {spec}'


def _other_library(path):
    """Another build of the library, typed as the binding types its own."""
    import ctypes
    from gridworld_amd import vox as X
    lib = ctypes.CDLL(os.path.abspath(path))
    for name, (res, args) in X.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def bench_spec(env, acts, name, iters, warmup, repeats, other=None):
    from gridworld_amd import VoxSpec, vox as X
    spec = VoxSpec(**SPECS[name])
    n = env.num_envs
    check_today(env, spec)
    out = env.vox_obs(spec)
    today = Today(env, spec)
    step = {'t': 0}

    def one_step():
        env.step(acts[step['t'] % len(acts)])
        step['t'] += 1

    def through(lib):
        def call():
            mine, X.BINDING.lib = X.BINDING.lib, lib
            try:
                env.vox_obs(spec, out=out, restart=env.done)
            finally:
                X.BINDING.lib = mine
        return call
    variants = {'vox_obs': (lambda: env.vox_obs(spec, out=out, restart=env.done), iters), 'today': (today, iters),
                'step': (one_step, 10 * iters)}
    for k, lib in enumerate(other or ()):
        variants['vox_obs_other%d' % k] = (through(lib), iters)
    us = {k: [] for k in variants}
    for r in range(repeats):
        for k, (fn, its) in variants.items():
            us[k].append(BR._time(fn, its, warmup if r == 0 else 1))
    res = {k: _spread(v) for k, v in us.items()}
    med = lambda k: res[k]['us_per_call_median']  # noqa: E731
    nbytes = int(np.prod(spec.shape(n))) * out.element_size()
    res.update(spec_name=name, spec=repr(spec), envs=n, bytes_written_per_call=nbytes,
               bytes_moved_by_the_shift=2 * (spec.stack - 1) * (nbytes // spec.stack),
               write_bound_us_at_8TBps=round(nbytes / HBM_PEAK * 1e6, 2),
               achieved_store_TBps=round(nbytes / (med('vox_obs') * 1e-6) / 1e12, 3),
               share_of_8TBps=round(nbytes / (med('vox_obs') * 1e-6) / HBM_PEAK, 3),
               today_over_vox_obs=round(med('today') / med('vox_obs'), 2),
               vox_obs_beats_today_with_spreads_apart=res['vox_obs']['us_per_call_max'] < res['today']['us_per_call_min'],
               vox_obs_over_step=round(med('vox_obs') / med('step'), 2))
    for k in range(len(other or ())):
        res['other%d_over_vox_obs' % k] = round(med('vox_obs_other%d' % k) / med('vox_obs'), 3)
    del out, today
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--specs', default=','.join(SPECS))
    ap.add_argument('--envs', default='4096,65536')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--git-commit', default=None, help='the commit to stamp (default: git rev-parse HEAD)')
    ap.add_argument('--lib', default=None, help='other builds of libigw_vox.so to measure beside the package\'s, comma-separated')
    ap.add_argument('--note', default=None, help='a remark to keep with the result (an A/B arm, say)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_vox.py needs a GPU')
    from gridworld_amd import VecGridWorld, vox as X, workloads
    line = {'tool': 'tools/bench_vox.py', 'vox_build_id': X.build_id(), 'git_commit': a.git_commit or BR._git_commit(),
            'device': torch.cuda.get_device_name(0), 'iters': a.iters, 'results': []}
    if a.note:
        line['note'] = a.note
    other = None
    if a.lib:
        X.load()
        other = [_other_library(path) for path in a.lib.split(',')]
        line['other_vox_build_ids'] = [lib.igw_vox_build_id().decode() for lib in other]
    for n in (int(v) for v in a.envs.split(',')):
        env = VecGridWorld(n, size_reward=False, autoreset=True)
        env.set_tasks(workloads.rt20(n, seed=1).numpy())
        env.reset()
        acts = env.fill_actions(60, seed=3)
        for t in range(60):
            env.step_walking_ptr(acts[t])
        for name in a.specs.split(','):
            if name not in SPECS:
                raise SystemExit(f'unknown spec {name!r}; the specs are {list(SPECS)}')
            line['results'].append(bench_spec(env, acts, name, a.iters, a.warmup, max(1, a.repeats), other))
        del env
        torch.cuda.empty_cache()
    BR._emit(line, a.out)


if __name__ == '__main__':
    main()
