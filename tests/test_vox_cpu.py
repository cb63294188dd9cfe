"""CPU side of the voxel observation: libigw_vox.so as a cross-compiled artefact -- its exports,
its code object, its argument checks --, VoxSpec and vox_channel_names, the ValueErrors of VecGridWorld / vox_obs
without a device, the model's self-check against a naive version and the coverage of the oracle cases the GPU test
compares on.  The GPU comparison is tests/test_gpu_vox.py."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import vox_cases as VC
import vox_model as VM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = '/opt/rocm/lib/llvm/bin'


def _declared():
    src = open(os.path.join(ROOT, 'include', 'igw_vox.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(igw_[a-z0-9_]+)\s*\(', src)))


# ---- the library -------------------------------------------------------------------------------------------------------
def test_vox_library_cross_compiles_and_exports_its_declared_symbols():
    from gridworld_amd import vox as X
    lib = X.build()
    assert os.path.exists(lib) and os.path.basename(lib) == 'libigw_vox.so'
    L = X.load()
    assert sorted(X.EXPORTS) == _declared()
    assert {'igw_vox_version', 'igw_vox_build_id', 'igw_vox_last_error', 'igw_vox_obs'} == set(X.EXPORTS)
    for name in _declared():
        assert hasattr(L, name)
    assert L.igw_vox_version() == X.VERSION == 1
    assert X.build_id() == X.source_hash() == X.built_id()
    assert not X.is_stale()
    header = open(os.path.join(ROOT, 'include', 'igw_vox.h')).read()
    assert ctypes.sizeof(X.Spec) == int(re.search(r'IGW_VOX_SPEC_BYTES (\d+)', header).group(1)) == 192
    assert ctypes.sizeof(X.Source) == 32 and X.Spec.data.offset == 168


def test_vox_sources_are_in_no_other_library():
    """The vox library's files enter no other library's build id and no other library's files enter its own, but for
    csrc/igw_voxel.h, igw_voxel_table.h and igw_voxel_stage.h, which are vox's and recall's and no other library's; it is
    built with the step library's flags."""
    from gridworld_amd import aim as A, build as B, codec as K, goal as G, peek as P, query as Q, recall as RC, render as R, \
        vox as X
    others = B.SOURCES + B.HEADERS + R.SOURCES + R.HEADERS + R.OBS_SOURCES + R.OBS_HEADERS + Q.SOURCES + Q.HEADERS + \
        K.LIBRARY.sources + K.LIBRARY.headers + G.SOURCES + G.HEADERS + A.SOURCES + A.HEADERS + P.SOURCES + P.HEADERS
    srcs = {os.path.basename(s) for s in others}
    mine = [os.path.basename(s) for s in X.SOURCES + X.HEADERS]
    shared = ['igw_voxel.h', 'igw_voxel_stage.h', 'igw_voxel_table.h']
    assert sorted(mine) == ['igw_vox.h', 'igw_vox.hip'] + shared
    assert not srcs & set(mine)
    assert {os.path.basename(s) for s in RC.SOURCES + RC.HEADERS} & set(mine) == set(shared)
    assert X.LIBRARY.flags == () and os.path.basename(X.LIB) == 'libigw_vox.so'
    assert X.LIBRARY.marker == b'igw-vox-build-id:'
    assert X.LIBRARY.marker not in (Q.LIBRARY.marker, G.LIBRARY.marker, A.LIBRARY.marker, P.LIBRARY.marker,
                                    B.STEP.marker, R.LIBRARY.marker, R.OBS_LIBRARY.marker)
    text = open(X.SOURCES[0]).read()
    assert re.findall(r'#include "([^"]+)"', text) == ['../../../include/igw_vox.h', '../igw_voxel.h', '../igw_voxel_table.h',
                                                        '../igw_voxel_stage.h']


def test_vox_code_object_has_no_scratch_and_no_vector_spills(tmp_path):
    """The notes of the gfx950 code object inside the library, read as tests/test_peek_cpu.py reads the peek's."""
    from gridworld_amd import vox as X
    fat, co = str(tmp_path / 'fat.bin'), str(tmp_path / 'dev.co')
    subprocess.check_call([os.path.join(LLVM, 'llvm-objcopy'), '--dump-section', '.hip_fatbin=' + fat, X.build()])
    subprocess.check_call([os.path.join(LLVM, 'clang-offload-bundler'), '--type=o',
                           '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--input=' + fat, '--output=' + co, '--unbundle'])
    notes = subprocess.check_output([os.path.join(LLVM, 'llvm-readelf'), '--notes', co], text=True)
    kern = [b for b in notes.split('- .agpr_count:')[1:] if 'igw_vox_kernel' in b]
    assert len(kern) == 1
    val = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, kern[0]).group(1))  # noqa: E731
    print('igw_vox_kernel: %d VGPRs, %d SGPRs (%d spilled to vector lanes), %d B of LDS' % (
        val('vgpr_count'), val('sgpr_count'), val('sgpr_spill_count'), val('group_segment_fixed_size')))
    assert val('private_segment_fixed_size') == 0
    assert val('vgpr_spill_count') == 0
    assert re.search(r'\.uses_dynamic_stack:\s+false', kern[0])
    # (derived from the register file and the LDS size, not measured: 512 registers per lane and SIMD / 128 = four
    # wavefronts per SIMD = four workgroups of 256 per compute unit, and 160 KB of LDS / 40 KB = four as well)
    assert val('vgpr_count') <= 128
    assert val('group_segment_fixed_size') <= 40 * 1024
    assert re.search(r'\.max_flat_workgroup_size:\s+256', kern[0])


# ---- the arguments -----------------------------------------------------------------------------------------------------
def test_vox_rejects_bad_arguments_without_a_device():
    from gridworld_amd import vox as X
    L = X.load()
    buf = (ctypes.c_uint8 * 16384)()
    p16 = (ctypes.addressof(buf) + 15) & ~15
    nan, inf = float('nan'), float('inf')

    def call(agent=p16, aux=p16, n=1, null_spec=False, sources=((p16, None, 1104, 0, 0),), **kw):
        s = X.Spec()
        for k, src in enumerate(sources):
            s.sources[k] = X.Source(*src)
        f = dict(num_sources=len(sources), agent_plane=1, frame=X.WORLD, radius=5, dtype=0, stack=1, fill=0, scale=1.0,
                 bias=0.0, data=p16, restart=None, restart_stride=0)
        f.update(kw)
        for k, v in f.items():
            setattr(s, k, v)
        return L.igw_vox_obs(agent, aux, n, None if null_spec else ctypes.byref(s), None)

    src = lambda **kw: (tuple({**dict(rows=p16, add=None, stride=1104, by_task=0, enc=0), **kw}.values()),)  # noqa: E731
    bad = [dict(agent=None), dict(aux=None), dict(null_spec=True), dict(data=None), dict(n=-1),
           dict(num_sources=0), dict(num_sources=5), dict(sources=src(rows=None)), dict(sources=src(stride=1088)),
           dict(sources=src() + src(stride=0)), dict(sources=src(enc=2)), dict(sources=src(enc=-1)),
           dict(frame=2), dict(frame=-1), dict(dtype=4), dict(dtype=-1),
           dict(frame=X.EGO, radius=0), dict(frame=X.EGO, radius=11), dict(stack=0), dict(stack=9),
           dict(dtype=1, scale=nan), dict(dtype=1, scale=inf), dict(dtype=3, bias=nan), dict(dtype=2, bias=-inf),
           dict(scale=2.0), dict(bias=1.0),
           dict(dtype=1, data=p16 + 1), dict(dtype=2, data=p16 + 1), dict(dtype=3, data=p16 + 2),
           dict(restart=p16, restart_stride=0), dict(restart=p16, restart_stride=-64)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert L.igw_vox_last_error().startswith(b'igw_vox_obs: '), kw
    # nothing is launched for n == 0 (`data` may then be NULL); the checks come first all the same.  A radius is looked
    # at with EGO only.  (More than 2^31 - 1 blocks cannot be asked for: a block is an env, and n is an int32.)
    assert call(n=0) == 0 and call(n=0, data=None) == 0 and call(n=0, radius=0, sources=src() * 4) == 0
    assert call(n=0, stack=9) == -1 and call(n=0, agent=None) == -1 and call(n=0, num_sources=0) == -1


# ---- VoxSpec -------------------------------------------------------------------------------------------------------------
def test_voxspec_validates_on_construction_and_describes_its_tensor():
    import gridworld_amd as G
    s = G.VoxSpec()
    assert (s.channels, s.size, s.shape(7)) == (13, 11, (7, 13, 9, 11, 11)) and s.dtype is torch.uint8
    assert G.vox_channel_names(s) == ['grid:%d' % k for k in range(1, 7)] + ['target:%d' % k for k in range(1, 7)] + ['agent']
    s = G.VoxSpec(planes=(('grid', 'occ'), ('todo', 'onehot'), ('grid', 'onehot'), ('want', 'occ')), agent=False,
                  frame='ego', radius=10, dtype='float16', stack=8, scale=1 / 3, bias=-0.1)
    assert (s.channels, s.size, s.shape(2)) == (14, 21, (2, 112, 9, 21, 21)) and s.dtype is torch.float16
    assert s.needs() == ('want', 'todo')
    names = G.vox_channel_names(s)
    assert names[0] == 'grid' and names[1:7] == ['todo:%d' % k for k in range(1, 7)] and names[-1] == 'want'
    assert len(names) == s.channels
    assert G.vox_channel_names(dict(planes=(('todo', 'occ'),))) == ['todo', 'agent']
    assert G.VoxSpec.of(s) is s and G.VoxSpec.of(dict(stack=3, frame='ego', radius=1)).shape(1) == (1, 39, 9, 3, 3)
    assert repr(G.VoxSpec(stack=2)).startswith('VoxSpec(planes=') and 'stack=2' in repr(G.VoxSpec(stack=2))
    bad = [dict(planes=()), dict(planes=(('grid', 'onehot'),) * 2), dict(planes=(('grid', 'occ'),) * 5),
           dict(planes=(('grid', 'onehot'), ('grid', 'occ'), ('target', 'onehot'), ('target', 'occ'), ('want', 'occ'))),
           dict(planes=(('pov', 'onehot'),)), dict(planes=(('grid', 'rgb'),)), dict(planes='grid'), dict(planes=(('grid',),)),
           dict(frame='camera'), dict(radius=0), dict(radius=11), dict(radius=2.5), dict(radius=True),
           dict(dtype=torch.int8), dict(dtype='float64'), dict(stack=0), dict(stack=9), dict(stack=1.5),
           dict(dtype=torch.float16, scale=float('nan')), dict(dtype=torch.float32, bias=float('inf')),
           dict(dtype=torch.float32, scale=1e39), dict(scale=2.0), dict(bias=0.5)]
    for kw in bad:
        with pytest.raises(ValueError):
            G.VoxSpec(**kw)
    for x in (None, 3, 'world', ('grid',)):
        with pytest.raises(ValueError):
            G.VoxSpec.of(x)


class _Stub:
    """What _Rows.vox_obs looks at before it touches a device."""

    def __new__(cls, n=4):
        from gridworld_amd import vec_env as V

        class Rows(V._Rows):
            def __del__(self):
                pass
        r = Rows()
        r.num_envs, r.flying, r.walk_dict, r.device = n, False, False, torch.device('cpu')
        r.cfg = types.SimpleNamespace(size_reward=0)
        r._stream = lambda: None
        return r


def test_vox_obs_raises_value_error_before_it_touches_a_device():
    import gridworld_amd as G
    env = _Stub()
    for spec in (dict(stack=9), dict(planes=(('depth', 'occ'),)), 'world', None):
        with pytest.raises(ValueError):
            env.vox_obs(spec)
    wants = G.VoxSpec(planes=(('grid', 'occ'), ('want', 'onehot'), ('todo', 'occ')))
    for goal in (None, {}, {'want': torch.zeros((4, 9, 11, 11), dtype=torch.int8)}):
        with pytest.raises(ValueError, match='goal'):
            env.vox_obs(wants, goal=goal)
    # the constructor: a bad spec, and planes of a goal query it was not asked to run -- before it looks for a device
    for kw in (dict(vox_obs=dict(stack=0)), dict(vox_obs='world'), dict(vox_obs=wants), dict(vox_obs=wants, goal=True),
               dict(vox_obs=wants, goal=('want', 'gain')), dict(vox_obs=dict(planes=(('todo', 'occ'),)), goal=('want',))):
        with pytest.raises(ValueError):
            G.VecGridWorld(4, **kw)


def test_rows_of_takes_dense_cells_at_any_row_stride():
    from gridworld_amd import vox as X
    wide = torch.zeros((4, 1104), dtype=torch.int8)
    view = torch.as_strided(wide, (4, 9, 11, 11), (1104, 121, 11, 1))
    assert X.rows_of('x', view, 4) == (wide.data_ptr(), 1104)
    dense = torch.zeros(4 * 1089 + 1, dtype=torch.int8)[1:].view(4, 9, 11, 11)
    assert X.rows_of('x', dense, 4) == (dense.data_ptr(), 1089)
    assert X.rows_of('x', wide, 4) == (wide.data_ptr(), 1104)
    for t in (view[:3], view.to(torch.int32), view.permute(0, 1, 3, 2), wide[:, :1000], np.zeros((4, 9, 11, 11), np.int8)):
        with pytest.raises(ValueError):
            X.rows_of('x', t, 4)


# ---- the model -----------------------------------------------------------------------------------------------------------
def test_model_equals_the_naive_version_in_every_quadrant():
    from gridworld_amd import vox as X
    rng = np.random.RandomState(3)
    n = 16
    mk = lambda lo, hi, p: (rng.randint(lo, hi, (n, 9, 11, 11)) * (rng.uniform(size=(n, 9, 11, 11)) < p)).astype(np.int8)  # noqa: E731
    grid, src = mk(1, 7, 0.2), dict(target=mk(1, 8, 0.2), want=mk(-6, 7, 0.3), todo=mk(-6, 7, 0.1))
    pose = np.stack([rng.choice(VC.XZ + (0.0, -3.0, 4.49), n), rng.choice(VC.YS + (0.0, 3.0), n),
                     rng.choice(VC.XZ + (0.0, 2.0), n), np.resize(np.array(VC.FLY_YAWS + (90.0, 180.0, 270.0, -90.0)), n)], 1)
    assert sorted(set(VM.quadrant(pose[:, 3]).tolist())) == [0, 1, 2, 3]
    assert VM.quadrant([0, 44.99, 45, 315, 360, -45, -45.5, 404.5, 99999]).tolist() == [0, 0, 1, 0, 0, 0, 3, 0, 3]
    # the add is a binary64 add: the double below 45 plus 45 is a tie that rounds to 90.0, so it already reads as
    # quadrant 1; the double below 135 plus 45 is exact and stays in quadrant 1
    assert np.nextafter(45.0, 0.0) + 45.0 == 90.0 and np.nextafter(135.0, 0.0) + 45.0 < 180.0
    assert VM.quadrant([np.nextafter(45.0, 0.0), np.nextafter(135.0, 0.0), 135.0]).tolist() == [1, 1, 2]
    planes4 = (('grid', 'onehot'), ('target', 'occ'), ('want', 'onehot'), ('todo', 'occ'))
    specs = [X.VoxSpec(planes=planes4)] + [X.VoxSpec(planes=planes4, frame='ego', radius=r) for r in (1, 5, 10)] + \
        [X.VoxSpec(planes=(('todo', 'onehot'), ('grid', 'occ')), agent=False, frame='ego', radius=5)]
    for spec in specs:
        a, b = VM.planes(grid, pose, src, spec), VM.naive_planes(grid, pose, src, spec)
        assert a.shape == spec.shape(n)[:1] + (spec.channels,) + spec.shape(n)[2:] and a.dtype == np.uint8
        assert np.array_equal(a, b), spec
        assert a.any() and set(np.unique(a).tolist()) == {0, 1}
    # the agent's two cells sit in the window's centre column, and the sight vector of yaw 90 (+x) is the way up
    ego = X.VoxSpec(planes=(('grid', 'occ'),), frame='ego', radius=2)
    g = np.zeros((1, 9, 11, 11), np.int8)
    g[0, 0, 7, 5] = 3                                  # two cells towards +x of the agent at the origin
    x = VM.planes(g, np.array([[0.0, 0.0, 0.0, 90.0]]), {}, ego)
    assert x[0, 1, :, 2, 2].tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 0] and x[0, 1].sum() == 2
    assert x[0, 0, 0, 0, 2] == 1 and x[0, 0].sum() == 1
    x = VM.planes(g, np.array([[0.0, 0.0, 0.0, 0.0]]), {}, ego)      # facing -z: +x is two cells to the right
    assert x[0, 0, 0, 2, 4] == 1 and x[0, 0].sum() == 1


def test_model_observe_shifts_fills_and_rounds_twice():
    from gridworld_amd import vox as X
    new = lambda v: np.full((3, 2, 9, 3, 3), v, np.uint8)  # noqa: E731
    spec = X.VoxSpec(planes=(('grid', 'occ'),), frame='ego', radius=1, stack=3)
    a = VM.observe(new(1), None, None, spec)
    assert a.shape == (3, 6, 9, 3, 3) and a.dtype is torch.uint8 and bool((a == 1).all())
    b = VM.observe(new(0), a, np.array([0, 255, 0], np.uint8), spec)
    assert b[0, :4].eq(1).all() and b[0, 4:].eq(0).all() and b[1].eq(0).all() and torch.equal(b[0], b[2])
    assert VM.observe(new(0), a, None, spec, fill=True).eq(0).all()
    f16 = X.VoxSpec(dtype=torch.float16, scale=1 / 3, bias=-0.1)
    v = VM.observe(np.ones((1, 13, 9, 11, 11), np.uint8), None, None, f16)
    want = np.float16(np.float32(np.float32(1.0) * np.float32(1 / 3)) + np.float32(-0.1))
    assert v.dtype is torch.float16 and VM.bits(v).unique().tolist() == [int(want.view(np.int16))]


# ---- coverage ------------------------------------------------------------------------------------------------------------
def test_cases_cover_what_the_gpu_comparison_has_to_tell_apart():
    """The floors of VC.FLOORS, counted on the oracle-side arrays: over every case, and the first seven over the directed
    table alone.  Counted (all cases / the directed tables alone): quadrant 0 1,639 / 392, 1 395 / 294, 2 140 / 98, 3 246 /
    196; a half-integer x or z 916 / 900; the head outside in x / z 661 / 660, in y 490 / 490; a `want` row with a negative
    id 1,172 / 980; a `target` row that differs from the table's 1,556 / 980."""
    truths = VC.all_truths()
    assert list(truths) == list(VC.MC.cases()) + ['recolour', 'flying', 'directed_walking', 'directed_flying']
    assert len(VC.directed_poses(False)) == 8 * 49 and len(VC.directed_poses(True)) == 12 * 49
    total, directed = {}, {}
    for name, truth in truths.items():
        for k, v in VC.coverage(truth).items():
            total[k] = total.get(k, 0) + v
            if name.startswith('directed'):
                directed[k] = directed.get(k, 0) + v
    for k in VC.FLOORS:
        print('%-36s %6d   directed alone %6d   (floor %d)' % (k, total[k], directed[k], VC.FLOORS[k]))
    for k, floor in VC.FLOORS.items():
        assert total[k] >= floor, (k, total[k])
    for k in VC.DIRECTED_FLOORS:
        assert directed[k] >= VC.FLOORS[k], (k, directed[k])
    # the directed poses arrive in the oracle's records as they were set
    for flying in (False, True):
        assert np.array_equal(VC.directed_truth(flying)['pose'][0], VC.directed_poses(flying)[:, :4])
    assert (VC.walking_truth('recolour')['target'] != VC.walking_truth('recolour')['table']).any()
