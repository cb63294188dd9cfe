"""CPU side of the recall query: libigw_recall.so as a cross-compiled artefact -- its exports, its
code object, its argument checks --, the host-side checks of gridworld_amd/recall.py and of env.recall, and the numpy
model the GPU test leans on (tests/recall_model.py on tests/recall_cases.py), pinned to the stepped CPU oracle and counted
for coverage.  The GPU comparison is tests/test_gpu_recall.py."""
import ctypes
import math
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from gridworld_amd import recall as _feature  # noqa: F401  (without the query nothing in this file can run)

import recall_cases as RCC
import recall_model as RCM
import relabel_cases as RC
import vox_model as VM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = '/opt/rocm/lib/llvm/bin'
E, T = RCC.E, RCC.T


def _declared():
    src = open(os.path.join(ROOT, 'include', 'igw_recall.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(igw_[a-z0-9_]+)\s*\(', src)))


# ---- the library -------------------------------------------------------------------------------------------------------
def test_recall_library_cross_compiles_and_exports_its_declared_symbols():
    from gridworld_amd import recall as R
    lib = R.build()
    assert os.path.exists(lib) and os.path.basename(lib) == 'libigw_recall.so'
    L = R.load()
    assert sorted(R.EXPORTS) == _declared()
    assert {'igw_recall_version', 'igw_recall_build_id', 'igw_recall_last_error', 'igw_recall'} == set(R.EXPORTS)
    for name in _declared():
        assert hasattr(L, name)
    assert L.igw_recall_version() == R.VERSION == 1
    assert R.build_id() == R.source_hash() == R.built_id()
    assert not R.is_stale()
    syms = subprocess.check_output([os.path.join(LLVM, 'llvm-readelf'), '--dyn-syms', '-W', lib], text=True)
    exported = [ln.split()[-1] for ln in syms.splitlines() if ' GLOBAL ' in ln and ' UND ' not in ln]
    assert sorted(s for s in exported if s.startswith('igw_')) == _declared()   # exactly the declared symbols
    header = open(os.path.join(ROOT, 'include', 'igw_recall.h')).read()
    assert ctypes.sizeof(R.Spec) == int(re.search(r'IGW_RECALL_SPEC_BYTES (\d+)', header).group(1)) == 64
    assert ctypes.sizeof(R.Plane) == 8 and R.Spec.num_planes.offset == 32 and R.Spec.scale.offset == 56


def test_recall_sources_are_in_no_other_library():
    """The recall library's files enter no other library's build id and no other library's files enter its own, but for
    csrc/igw_voxel.h, igw_voxel_table.h and igw_voxel_stage.h, which are vox's and recall's and no other library's; it is
    built with the step library's flags, and the package-level build knows it."""
    from gridworld_amd import aim as A, build as B, codec as K, goal as G, peek as P, peek_dict as PD, query as Q, \
        recall as R, relabel as RL, render as RD, vox as X, worth as W
    srcs = [os.path.basename(s) for s in B.SOURCES + B.HEADERS + RD.SOURCES + RD.HEADERS + RD.OBS_SOURCES + RD.OBS_HEADERS +
            Q.SOURCES + Q.HEADERS + K.LIBRARY.sources + K.LIBRARY.headers]
    for m in (G, A, P, PD, W, RL):
        srcs += [os.path.basename(s) for s in m.LIBRARY.sources + m.LIBRARY.headers]
    mine = [os.path.basename(s) for s in R.SOURCES + R.HEADERS]
    shared = ['igw_voxel.h', 'igw_voxel_stage.h', 'igw_voxel_table.h']
    assert sorted(mine) == ['igw_recall.h', 'igw_recall.hip'] + shared and not set(srcs) & set(mine)
    assert {os.path.basename(s) for s in X.LIBRARY.sources + X.LIBRARY.headers} & set(mine) == set(shared)
    assert R.LIBRARY.flags == () and os.path.basename(R.LIB) == 'libigw_recall.so'
    markers = [m.LIBRARY.marker for m in (G, A, P, PD, X, W, Q, RL)]
    assert R.LIBRARY.marker == b'igw-recall-build-id:' and R.LIBRARY.marker not in markers
    text = open(R.SOURCES[0]).read()
    assert re.findall(r'#include "([^"]+)"', text) == ['../../../include/igw_recall.h', '../igw_voxel.h', '../igw_voxel_table.h',
                                                        '../igw_voxel_stage.h']
    text += ''.join(open(os.path.join(os.path.dirname(R.SOURCES[0]), '..', h)).read() for h in shared)
    assert 'asm' not in re.sub(r'//.*', '', text)                               # no inline assembly
    assert 'recall' in open(os.path.join(ROOT, 'gridworld_amd', 'build.py')).read().split("if __name__ == '__main__':")[1]
    assert 'hip_recall.build(force=True)' in open(os.path.join(ROOT, '__graft_entry__.py')).read()


def test_recall_code_object_has_no_scratch_and_no_spills(tmp_path):
    """The notes of the gfx950 code object inside the library, read as tests/test_vox_cpu.py reads the vox's."""
    from gridworld_amd import recall as R
    fat, co = str(tmp_path / 'fat.bin'), str(tmp_path / 'dev.co')
    subprocess.check_call([os.path.join(LLVM, 'llvm-objcopy'), '--dump-section', '.hip_fatbin=' + fat, R.build()])
    subprocess.check_call([os.path.join(LLVM, 'clang-offload-bundler'), '--type=o',
                           '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--input=' + fat, '--output=' + co, '--unbundle'])
    notes = subprocess.check_output([os.path.join(LLVM, 'llvm-readelf'), '--notes', co], text=True)
    kern = [b for b in notes.split('- .agpr_count:')[1:] if 'igw_recall_kernel' in b]
    assert len(kern) == 4                                    # one kernel per element type
    for k in kern:
        val = lambda key: int(re.search(r'\.%s:\s+(\d+)' % key, k).group(1))  # noqa: E731
        print('%s: %d VGPRs, %d SGPRs (%d parked in vector lanes), %d B of LDS' % (
            re.search(r'\.name:\s+(\S+)', k).group(1), val('vgpr_count'), val('sgpr_count'), val('sgpr_spill_count'),
            val('group_segment_fixed_size')))
        # No byte of scratch and no vector register spilled: nothing the kernel keeps ever goes to memory.  As in the vox
        # kernel, a few scalar registers (lane masks and kernel arguments that are live across the walk over the change
        # words) are parked in the lanes of one vector register and fetched back outside the staging and store loops; that count is
        # bounded.
        assert val('private_segment_fixed_size') == 0
        assert val('vgpr_spill_count') == 0 and val('sgpr_spill_count') <= 16
        assert re.search(r'\.uses_dynamic_stack:\s+false', k)
        # (derived from the register file and the LDS size, not measured: 512 registers per lane and SIMD / 64 = eight
        # wavefronts per SIMD = eight workgroups of 256 per compute unit, and 160 KB of LDS / 32 KB = five)
        assert val('vgpr_count') <= 64
        assert val('group_segment_fixed_size') <= 32 * 1024
        assert re.search(r'\.max_flat_workgroup_size:\s+256', k)


# ---- the arguments -----------------------------------------------------------------------------------------------------
def test_recall_rejects_bad_arguments_without_a_device():
    from gridworld_amd import recall as R
    L = R.load()
    buf = (ctypes.c_uint8 * 32768)()
    p16 = (ctypes.addressof(buf) + 15) & ~15
    nan, inf = float('nan'), float('inf')
    ptrs = ('records', 'first', 'length', 'start_grid', 'init_pose', 'episode', 'step')
    outs = ('obs', 'next_obs', 'record', 'valid')
    ok = dict({k: p16 for k in ptrs + outs}, n_records=4, E=1, L=4, B=1, goal=None, goal_stride=0, n_goal_rows=0,
              goal_index=None)

    def call(null_spec=False, planes=((R.GRID, 0),), **kw):
        a = dict(ok)
        s = R.Spec()
        for k, pl in enumerate(planes):
            s.planes[k] = R.Plane(*pl)
        f = dict(num_planes=len(planes), agent_plane=1, frame=0, radius=5, dtype=0, stack=1, scale=1.0, bias=0.0)
        for k, v in kw.items():
            (f if k in f else a)[k] = v
        for k, v in f.items():
            setattr(s, k, v)
        return L.igw_recall(a['records'], a['n_records'], a['first'], a['length'], a['start_grid'], a['init_pose'], a['E'],
                            a['L'], a['episode'], a['step'], a['B'], a['goal'], a['goal_stride'], a['n_goal_rows'],
                            a['goal_index'], None if null_spec else ctypes.byref(s), *[a[k] for k in outs], None)

    with_goal = dict(goal=p16 + 1, goal_stride=1089, n_goal_rows=1)
    assert call(B=0) == 0 and call(B=0, planes=((R.GOAL, 1),), **with_goal) == 0
    bad = [{k: None} for k in ptrs] + \
        [dict(null_spec=True), dict({k: None for k in outs}), dict(B=-1), dict(E=-1), dict(n_records=-1), dict(L=0), dict(L=-2),
         dict(num_planes=0), dict(num_planes=5), dict(planes=((2, 0),)), dict(planes=((-1, 0),)), dict(planes=((0, 2),)),
         dict(planes=((0, -1),)), dict(frame=2), dict(frame=-1), dict(dtype=4), dict(dtype=-1),
         dict(frame=1, radius=0), dict(frame=1, radius=11), dict(stack=0), dict(stack=9),
         dict(dtype=1, scale=nan), dict(dtype=1, scale=inf), dict(dtype=3, bias=nan), dict(dtype=2, bias=-inf),
         dict(scale=2.0), dict(bias=1.0),
         dict(planes=((R.GOAL, 0),)), dict(planes=((R.GRID, 0), (R.GOAL, 1))),              # a goal plane without goal
         dict(goal=p16, goal_stride=1088, n_goal_rows=1), dict(goal=p16, goal_stride=0, n_goal_rows=1),
         dict(goal=p16, goal_stride=1089, n_goal_rows=-1),
         dict(start_grid=p16 + 8), dict(first=p16 + 4), dict(init_pose=p16 + 4), dict(records=p16 + 2), dict(length=p16 + 2),
         dict(episode=p16 + 2), dict(step=p16 + 1), dict(goal_index=p16 + 4, **with_goal),
         dict(dtype=1, obs=p16 + 1), dict(dtype=2, next_obs=p16 + 1), dict(dtype=3, obs=p16 + 2), dict(dtype=3, next_obs=p16 + 2)]
    for kw in bad:
        assert call(**dict(dict(B=0), **kw)) == -1, kw        # checked before B == 0 returns: nothing is launched here
        assert L.igw_recall_last_error().startswith(b'igw_recall: '), kw
    # a radius is looked at with EGO only; record and valid take any address; a single output is enough.  (More than
    # 2^31 - 1 blocks cannot be asked for: a block is a sample, and B is an int32.)
    assert call(B=0, radius=0) == 0 and call(B=0, record=p16 + 1, valid=p16 + 3) == 0
    assert call(B=0, obs=None, next_obs=None, record=None) == 0 and call(B=0, dtype=3, scale=0.5, bias=-1.0) == 0


def test_recall_host_side_checks_sampler_and_views():
    import gridworld_amd as G
    from gridworld_amd import recall as R
    assert G.recall is R and callable(G.recall)
    assert R.OUTPUTS == ('obs', 'next_obs', 'record', 'valid') and R.DEFAULT == ('obs', 'next_obs', 'record')
    assert R.check_outputs(('valid', 'obs')) == ('obs', 'valid') and R.check_outputs('record') == ('record',)
    for names in ((), ('observation',), ('obs', 'reward')):
        with pytest.raises(ValueError):
            R.check_outputs(names)
    # the spec: a VoxSpec whose planes are the grid's and the goal's
    spec, s = R.spec_of(dict(planes=(('target', 'occ'), ('grid', 'onehot')), frame='ego', radius=3, dtype='bfloat16', stack=5,
                             scale=0.5, bias=-1.0))
    assert [(s.planes[k].source, s.planes[k].encoding) for k in range(2)] == [(R.GOAL, 1), (R.GRID, 0)]
    assert (s.num_planes, s.agent_plane, s.frame, s.radius, s.dtype, s.stack, s.scale, s.bias) == (2, 1, 1, 3, 2, 5, 0.5, -1.0)
    assert R.needs_goal(spec) and not R.needs_goal(G.VoxSpec(planes=(('grid', 'occ'),)))
    assert G.vox_channel_names(spec) == ['target'] + ['grid:%d' % k for k in range(1, 7)] + ['agent']
    for planes in ((('want', 'onehot'),), (('grid', 'occ'), ('todo', 'occ'))):
        with pytest.raises(ValueError, match='goal query'):
            R.spec_of(G.VoxSpec(planes=planes))
    for x in (None, 'world', dict(stack=9)):
        with pytest.raises(ValueError):
            R.spec_of(x)
    # goal rows at one stride
    wide = torch.zeros((3, 4, 1104), dtype=torch.int8)
    view = torch.as_strided(wide, (3, 4, 9, 11, 11), (4 * 1104, 1104, 121, 11, 1))
    assert R.goal_rows(view) == (wide.data_ptr(), 1104, 12) and R.goal_rows(wide) == (wide.data_ptr(), 1104, 12)
    odd = torch.zeros(5 * 1089 + 1, dtype=torch.int8)[1:].view(5, 1089)
    assert R.goal_rows(odd) == (odd.data_ptr(), 1089, 5) and odd.data_ptr() % 2 == 1
    assert R.goal_rows(view[1:2, 2:3]) == (view[1, 2].data_ptr(), 1089, 1)
    for t in (view[:, :2], view.to(torch.int32), wide[..., :1000], view.permute(0, 1, 2, 4, 3), np.zeros((2, 1104), np.int8),
              torch.zeros(1089, dtype=torch.int8)):
        with pytest.raises(ValueError):
            R.goal_rows(t)
    # launch(): everything is looked at before the device is
    cpu = torch.device('cpu')
    rec = torch.zeros((2, 2, 8, 64), dtype=torch.uint8)
    ok = dict(records=rec, first=torch.tensor([0, 16]), length=torch.tensor([8, 8], dtype=torch.int32),
              starts=torch.zeros((2, 1104), dtype=torch.int8), init_pose=torch.zeros((2, 5), dtype=torch.float64),
              episode=torch.zeros(3, dtype=torch.int32), step=torch.ones(3, dtype=torch.int32), spec=G.VoxSpec(), goal=wide[:, 0],
              goal_index=None, cap=8, names=('obs',), out=None, dev=cpu, stream=None)
    with pytest.raises(ValueError, match='device tensor'):
        G.recall(rec, ok['first'], ok['length'], ok['starts'], ok['init_pose'], ok['episode'], ok['step'], G.VoxSpec())
    bad = [dict(records=rec[..., :32]), dict(records=rec.to(torch.int8)), dict(first=ok['first'].to(torch.int32)),
           dict(length=ok['length'].long()), dict(starts=ok['starts'][:, :1089]), dict(init_pose=ok['init_pose'].float()),
           dict(init_pose=ok['init_pose'][:, :4]), dict(episode=ok['episode'].long()), dict(step=ok['step'][:2]), dict(cap=0),
           dict(goal=None), dict(goal=wide.to(torch.int16)), dict(goal_index=torch.zeros(3, dtype=torch.int32)),
           dict(goal_index=torch.zeros(2, dtype=torch.int64)), dict(names=()), dict(names=('nope',)), dict(space='swimming'),
           dict(spec=G.VoxSpec(planes=(('todo', 'occ'),))), dict(out={'valid': torch.zeros(3, dtype=torch.uint8)}),
           dict(out={'obs': torch.zeros((3, 13, 9, 11, 12), dtype=torch.uint8)}),
           dict(out={'obs': torch.zeros((3, 13, 9, 11, 11), dtype=torch.float16)})]
    for kw in bad:
        with pytest.raises(ValueError):
            R.launch(**dict(ok, **kw))
    with pytest.raises(ValueError):
        R.launch(**dict(ok, spec=G.VoxSpec(planes=(('grid', 'occ'),)), goal=None, goal_index=torch.zeros(3, dtype=torch.int64)))
    # the sampler: seeded, in range, a step no episode of no steps holds
    length = torch.tensor([0, 1, 2, 48, 250, 7], dtype=torch.int32)
    e, t = R.sample(length, 4096, seed=5)
    assert e.dtype == t.dtype == torch.int32 and tuple(e.shape) == tuple(t.shape) == (4096,)
    assert int(e.min()) == 0 and int(e.max()) == 5 and (t >= 1).all()
    n = length[e.long()]
    assert (t[n > 0] <= n[n > 0]).all() and (t[n == 0] == 1).all() and int((n == 0).sum()) >= 20
    assert set(t[e == 2].tolist()) == {1, 2} and len(set(t[e == 4].tolist())) > 200
    e2, t2 = R.sample(length, 4096, seed=5)
    assert torch.equal(e, e2) and torch.equal(t, t2) and not torch.equal(e, R.sample(length, 4096, seed=6)[0])
    assert tuple(R.sample(length, 0)[0].shape) == (0,)
    # the views of a record (include/igw.h's layout)
    r = np.zeros((2, 64), np.uint8)
    r[:, 0:20] = np.arange(10, dtype=np.float32).view(np.uint8).reshape(2, 20)
    r[:, 20:24] = np.array([0.5, -0.1], np.float32).view(np.uint8).reshape(2, 4)
    r[:, 28:40] = np.arange(12, dtype=np.int16).view(np.uint8).reshape(2, 12)
    r[:, 42], r[:, 43] = (1, 0), (0, 2 | 3 << 2 | 1 << 5)
    r[:, 44:48] = np.array([17, 3], np.int32).view(np.uint8).reshape(2, 4)
    d = R.decode(torch.from_numpy(r))
    assert d['action'].tolist() == [17, 3] and d['reward'].tolist() == [0.5, np.float32(-0.1)] and d['done'].tolist() == [1, 0]
    assert d['inventory'].tolist() == [list(range(6)), list(range(6, 12))] and d['agent_pos'][1].tolist() == [5, 6, 7, 8, 9]
    assert d['action'].data_ptr() == torch.from_numpy(r).data_ptr() + 44                 # views, not copies
    fl, wd = R.decode(torch.from_numpy(r), 'flying'), R.decode(torch.from_numpy(r), 'walking_dict')
    assert tuple(fl['movement'].shape) == (2, 3) and tuple(fl['camera'].shape) == (2, 2) and 'action' not in fl
    assert fl['camera'].data_ptr() == torch.from_numpy(r).data_ptr() + 56
    assert tuple(wd['buttons'].shape) == (2, 8) and wd['camera'].data_ptr() == torch.from_numpy(r).data_ptr() + 52
    with pytest.raises(ValueError):
        R.decode(torch.from_numpy(r), 'swimming')


class _Stub:
    """What _Rows.recall looks at before it touches a device."""

    def __new__(cls, n=4, traj=None):
        from gridworld_amd import vec_env as V

        class Rows(V._Rows):
            def __del__(self):
                pass
        r = Rows()
        r.num_envs, r.flying, r.walk_dict, r.device = n, False, False, torch.device('cpu')
        r.cfg = types.SimpleNamespace(size_reward=0)
        r._stream = lambda: None
        r._traj = traj
        return r


def test_env_recall_raises_value_error_before_it_touches_a_device():
    import gridworld_amd as G
    env = _Stub()
    for spec in (dict(stack=9), dict(planes=(('depth', 'occ'),)), 'world', None):
        with pytest.raises(ValueError):
            env.recall(spec, batch=4)
    with pytest.raises(ValueError, match='goal query'):
        env.recall(G.VoxSpec(planes=(('grid', 'occ'), ('want', 'onehot'))), batch=4)
    for outputs in ((), ('reward',), 'observations'):
        with pytest.raises(ValueError):
            env.recall(G.VoxSpec(), batch=4, outputs=outputs)
    with pytest.raises(ValueError, match='episode log'):
        env.recall(G.VoxSpec(planes=(('grid', 'occ'),)), batch=4)
    logged = _Stub(traj=(None, None, 0, 8))
    with pytest.raises(ValueError, match='is logged'):
        logged.recall(G.VoxSpec(planes=(('grid', 'occ'),)), batch=4)
    logged = _Stub(traj=(None, None, 2, 8))
    grid = G.VoxSpec(planes=(('grid', 'occ'),))
    for kw in (dict(), dict(batch=-1), dict(batch=2.5), dict(batch=True), dict(episode=[0]), dict(step=[1]),
               dict(batch=4, goals='final'), dict(batch=4, goals=3), dict(batch=4, goals={'reward': None}),
               dict(batch=4, goal=[0, 0, 0, 0]), dict(batch=4, goals='own', goal=[0, 0, 0, 0])):
        with pytest.raises(ValueError, match='recall'):
            logged.recall(grid, **kw)
    with pytest.raises(ValueError, match="'target' plane"):
        logged.recall(G.VoxSpec(), batch=4)


# ---- the model -----------------------------------------------------------------------------------------------------------
def test_the_model_rebuilds_the_oracles_grid_at_every_entry():
    """The log's change words (relabel_cases.words_of) applied to the start give the oracle's grid at every entry, every
    case and env; the words through a record buffer and back are the words."""
    for name in RCC.cases():
        b = RCC.base(name)
        rec = RCC.records_of(b['change'], b['pos'])
        assert np.array_equal(RCM.words_of_records(rec).reshape(E, T), b['change'])
        for i in range(E):
            assert np.array_equal(RCM.entry_grids(b['starts'][i], b['change'][i]), b['grids'][:, i]), (name, i)
            assert np.array_equal(RCM.entry_pose(rec[i * T:(i + 1) * T], b['init'][i], 0), b['init'][i, :4])
            assert np.array_equal(RCM.entry_pose(rec[i * T:(i + 1) * T], b['init'][i], T),
                                  b['pos'][i, T - 1, [0, 1, 2, 4]].astype(np.float64))


def test_the_slots_are_what_a_live_stack_shows_before_and_after_the_step():
    """obs / next_obs of (e, t) against tests/vox_model.py's own stack rule -- filled at the reset, shifted by every step
    -- fed the log's entries: the two formulations of "slot j holds entry max(0, t - K + j)" agree."""
    import gridworld_amd as G
    assert RCM.slots(1, 4) == ([0, 0, 0, 0], [0, 0, 0, 1]) and RCM.slots(3, 4) == ([0, 0, 1, 2], [0, 1, 2, 3])
    assert RCM.slots(9, 4) == ([5, 6, 7, 8], [6, 7, 8, 9]) and RCM.slots(5, 1) == ([4], [5])
    name = 'init_pose'
    b = RCC.base(name)
    rows = [3, 17]
    spec = G.VoxSpec(planes=(('grid', 'onehot'), ('target', 'occ')), frame='ego', radius=2, dtype=torch.float16, stack=3,
                     scale=1 / 3, bias=-0.1)
    goal = RCC.cases()[name]['targets'].reshape(E, -1).astype(np.int8)
    episode, step = RCC.pairs()
    keep = np.isin(episode, rows)
    rec = RCC.records_of(b['change'], b['pos'])
    want = RCM.recall(rec, np.arange(E) * T, np.full(E, T), b['starts'], b['init'], episode[keep], step[keep], spec, goal=goal)
    assert want['valid'].all() and want['obs'].dtype is torch.float16
    assert tuple(want['obs'].shape) == (2 * T, 3 * 8, 9, 5, 5)
    pose = RCC.log_pose(b)
    for k, i in enumerate(rows):
        stack = None
        for s in range(T + 1):
            new = VM.planes(b['grids'][s, i][None], pose[i, s][None], {'target': goal[i][None]}, spec)
            prev, stack = stack, VM.observe(new, stack, None, spec)
            if s >= 1:
                assert torch.equal(VM.bits(want['next_obs'][k * T + s - 1]), VM.bits(stack[0])), (i, s)
                assert torch.equal(VM.bits(want['obs'][k * T + s - 1]), VM.bits(prev[0])), (i, s)
                assert np.array_equal(want['record'][k * T + s - 1], rec[i * T + s - 1])


def test_the_model_pads_what_the_contract_calls_padding():
    import gridworld_amd as G
    b = RCC.base('towers')
    rec = RCC.records_of(b['change'], b['pos'])
    spec = G.VoxSpec(planes=(('grid', 'occ'), ('target', 'occ')), dtype=torch.float32, scale=2.0, bias=0.25, stack=2)
    goal = np.zeros((5, 1089), np.int8)
    first = np.array([0, T, -1, E * T - 10, 2 * T])
    length = np.array([T, 0, 5, 11, 100])               # in the buffer, empty, before it, behind it, clamped to L = T
    #                     ok  e<0  e>=E  t=0  t>len  empty  first<0  behind  goal<0  goal>=rows  ok (clamped)  t > L
    episode = np.array([0,  -1,  5,    0,   0,     1,     2,       3,      0,      0,          4,            4])
    step = np.array([T,   1,   1,    0,   T + 1, 1,     1,       1,      1,      1,          T,            T + 1])
    index = np.array([4,   0,   0,    0,   0,     0,     0,       0,      -1,     5,          0,            0])
    want = RCM.recall(rec, first, length, b['starts'][:5], b['init'][:5], episode, step, spec, goal=goal, goal_index=index, L=T)
    assert want['valid'].tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0]
    pad = want['valid'] == 0
    assert (want['obs'][pad] == 0.25).all() and (want['next_obs'][pad] == 0.25).all() and not want['record'][pad].any()
    assert (want['obs'][~pad] == 2.25).any() and np.array_equal(want['record'][0], rec[T - 1])


# ---- coverage ------------------------------------------------------------------------------------------------------------
def test_the_cases_cover_what_the_gpu_comparison_has_to_tell_apart():
    """The floors of RCC.FLOORS, counted on the oracle-side arrays alone over the eight cases' 12,288 samples (12,544
    entries); each floor is the count itself.  The walking cases never leave the grid, so `a head cell outside the grid`
    is 0 here: the hand-written records of tests/test_gpu_recall.py hold those poses and count them there.  The live
    float64 state and the log's float32 pose round to different head cells on 3 entries, all in `select_only`."""
    total = {}
    for name in RCC.cases():
        for k, v in RCC.coverage(RCC.base(name)).items():
            total[k] = total.get(k, 0) + v
    for k, v in total.items():
        print('%-48s %6d   (floor %d)' % (k, v, RCC.FLOORS[k]))
    assert set(total) == set(RCC.FLOORS)
    for k, floor in RCC.FLOORS.items():
        assert total[k] >= floor, (k, total[k])
        assert floor >= 20 or k in RCC.NOT_IN_THE_CASES, k
    assert total['live and logged head cells differ'] == 3      # 0.024 % of the entries
    assert math.isclose(3 / (8 * E * (T + 1)), 0.00024, rel_tol=0.01)
