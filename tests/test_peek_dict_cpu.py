"""CPU side of the peek query of the flying and walking Dict spaces: libigw_peek_dict.so as a
cross-compiled artefact -- its exports and constants, its code object's resources, its argument checks --, the
ValueErrors of VecGridWorld.peek_dict on a stub without a device, and the census of the oracle truth the GPU test
compares against.  The GPU comparison is tests/test_gpu_peek_dict.py."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

import peek_dict_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = '/opt/rocm/lib/llvm/bin'


def _header(name='igw_peek_dict.h', comments=False):
    src = open(os.path.join(ROOT, 'include', name)).read()
    return src if comments else re.sub(r'/\*.*?\*/', '', src, flags=re.S)


def _declared():
    return sorted(set(re.findall(r'\b(igw_[a-z0-9_]+)\s*\(', _header())))


# ---- the library -------------------------------------------------------------------------------------------------------
def test_library_cross_compiles_and_exports_its_declared_symbols():
    from gridworld_amd import peek_dict as D
    lib = D.build()
    assert os.path.exists(lib) and os.path.basename(lib) == 'libigw_peek_dict.so'
    L = D.load()
    assert sorted(D.EXPORTS) == _declared()
    assert {'igw_peek_dict_version', 'igw_peek_dict_build_id', 'igw_peek_dict_last_error', 'igw_peek_flying',
            'igw_peek_walking_dict'} == set(D.EXPORTS)
    for name in _declared():
        assert hasattr(L, name)
    assert L.igw_peek_dict_version() == D.VERSION == 1
    assert D.build_id() == D.source_hash() == D.built_id()
    assert not D.is_stale()


def test_constants_match_the_headers():
    from gridworld_amd import peek as P, peek_dict as D
    mine, peeks = _header(), _header('igw_peek.h')
    const = lambda src, name: int(re.search(r'#define\s+%s\s+(-?\d+)' % name, src).group(1))  # noqa: E731
    assert const(mine, 'IGW_PEEK_DICT_VERSION') == D.VERSION
    assert const(mine, 'IGW_PEEK_DICT_MAX_H') == D.MAX_H == const(peeks, 'IGW_PEEK_MAX_H') == P.MAX_H
    assert const(mine, 'IGW_PEEK_DICT_MAX_K') == D.MAX_K == const(peeks, 'IGW_PEEK_MAX_K') == P.MAX_K
    assert const(mine, 'IGW_PEEK_DICT_POSE') == const(peeks, 'IGW_PEEK_POSE') == 5
    assert const(mine, 'IGW_PEEK_DICT_BUTTONS') == 8
    assert D.OUTPUTS == P.OUTPUTS
    # the action arguments are the step's own, in its order (vec_env._SPACES)
    from gridworld_amd import _lib, vec_env as V
    for space, mode in (('flying', _lib.FLYING), ('walking_dict', _lib.WALKING_DICT)):
        step = [(k, str(dt).replace('torch.', ''), shape) for k, dt, shape in V._SPACES[mode].buffers]
        assert list(D.SPACES[space][1]) == step
        assert [(k, np.dtype(dt).name, shape) for k, dt, shape in DC.FIELDS[space]] == step
    # the header states the rule for every kind of invalid action the census knows
    text = ' '.join(_header(comments=True).split())
    for phrase in ('a movement component that is not finite', 'a camera component that is not finite or beyond',
                   'inventory outside 0..6, a hotbar byte above 6', 'placement outside 0..2'):
        assert phrase in text, phrase


def test_sources_are_in_no_other_library():
    """The library's files enter no other library's build id, no other library's kernels enter its own, it is built with
    the step library's flags and includes igw_device.h (and through it igw_trig.h) as it is."""
    from gridworld_amd import aim as A, build as B, codec as K, goal as G, peek as P, peek_dict as D, query as Q, render as R, vox as X
    others = B.SOURCES + B.HEADERS + R.SOURCES + R.HEADERS + R.OBS_SOURCES + R.OBS_HEADERS + Q.SOURCES + Q.HEADERS + \
        K.LIBRARY.sources + K.LIBRARY.headers + G.SOURCES + G.HEADERS + A.SOURCES + A.HEADERS + P.SOURCES + P.HEADERS + \
        X.LIBRARY.sources + X.LIBRARY.headers
    srcs = [os.path.basename(s) for s in others]
    assert 'igw_peek_dict.hip' not in srcs and 'igw_peek_dict.h' not in srcs
    mine = [os.path.basename(s) for s in D.SOURCES + D.HEADERS]
    assert [s for s in mine if s.endswith('.hip')] == ['igw_peek_dict.hip']
    assert D.LIBRARY.flags == () and D.LIBRARY.marker == b'igw-peek-dict-build-id:'
    assert D.LIBRARY.marker not in (P.LIBRARY.marker, Q.LIBRARY.marker, G.LIBRARY.marker, A.LIBRARY.marker, B.STEP.marker)
    assert P.LIBRARY.marker not in open(D.build(), 'rb').read()   # (... nor is it a prefix that built_id could find there)
    # the library's own files: its .hip file, the headers under csrc/peek/ and igw_vote.h
    own = [s for s in D.SOURCES + D.HEADERS
           if os.path.basename(os.path.dirname(s)) in ('peek', 'peek_dict') or os.path.basename(s) == 'igw_vote.h']
    assert sorted(os.path.basename(s) for s in own) == ['igw_peek_body.h', 'igw_peek_core.h', 'igw_peek_dict.hip', 'igw_vote.h']
    assert not {'igw_peek_body.h', 'igw_peek_core.h', 'igw_vote.h'} & {os.path.basename(s) for s in B.SOURCES + B.HEADERS}
    text = ''.join(open(s).read() for s in own)
    assert '#include "../igw_device.h"' in text and 'igw_trig.h' in open(os.path.join(D.CSRC, 'igw_device.h')).read()
    for name in ('igw_sincos', 'dd_two_prod', 'igw_atan2_accurate'):
        assert not re.search(r'\b%s\s*\([^;{]*\)\s*\{' % name, text), name   # the trig is included, not copied
    for name in ('parse_flying', 'parse_walking_dict', 'world_act_pre', 'world_act_post', 'finish_break', 'world_update',
                 'syn_size_delta', 'finish_step'):
        assert re.search(r'\b%s(<[A-Z]+>)?\(' % name, text), name   # restated here, not moved out of the step library


def _kernels(tmp_path):
    """name -> the notes block of each kernel of the gfx950 code object inside the library."""
    from gridworld_amd import peek_dict as D
    fat, co = str(tmp_path / 'fat.bin'), str(tmp_path / 'dev.co')
    subprocess.check_call([os.path.join(LLVM, 'llvm-objcopy'), '--dump-section', '.hip_fatbin=' + fat, D.build()])
    subprocess.check_call([os.path.join(LLVM, 'clang-offload-bundler'), '--type=o',
                           '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--input=' + fat, '--output=' + co, '--unbundle'])
    notes = subprocess.check_output([os.path.join(LLVM, 'llvm-readelf'), '--notes', co], text=True)
    blocks = [b for b in notes.split('- .agpr_count:')[1:] if 'igw_peek_dict_kernel' in b]
    return {('flying' if 'ILb1E' in b else 'walking_dict'): b for b in blocks}


def test_code_object_resources_are_the_ones_design_md_quotes(tmp_path):
    """VGPRs, LDS bytes, scratch bytes and waves per SIMD of both kernels, read from the code object's notes; the line
    DESIGN.md section 15 quotes for each is rebuilt from them.  Waves per SIMD are derived, not measured: 512 registers
    per lane and SIMD in granules of 8, 160 KiB of LDS per compute unit, four SIMDs, workgroups of four wavefronts."""
    kern = _kernels(tmp_path)
    assert sorted(kern) == ['flying', 'walking_dict']
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    for space, block in kern.items():
        val = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, block).group(1))  # noqa: E731
        alloc = -(-(val('vgpr_count') + int(re.match(r'\s*(\d+)', block).group(1))) // 8) * 8
        waves = min(8, 512 // alloc, (160 * 1024 // val('group_segment_fixed_size')) * 4 // 4)
        line = '`igw_peek_dict_kernel` (%s): %d VGPRs, %d B of LDS, %d B of scratch, %d SGPRs spilled to vector lanes, %d waves per SIMD' % (
            space.replace('_', ' '), val('vgpr_count'), val('group_segment_fixed_size'), val('private_segment_fixed_size'),
            val('sgpr_spill_count'), waves)
        print(line)
        assert line in design, line
        assert val('vgpr_spill_count') == 0 and re.search(r'\.uses_dynamic_stack:\s+false', block)
        assert (val('private_segment_fixed_size') == 0) == ('It does not spill to scratch' in design)
        assert re.search(r'\.max_flat_workgroup_size:\s+256', block)


# ---- the arguments -----------------------------------------------------------------------------------------------------
STATE = ('grid', 'occ', 'hist', 'aux', 'agent', 'task_target', 'task_start', 'task_meta', 'task_index')
OUT = ('reward', 'ends', 'change', 'pose', 'ret')
ACTS = {'flying': ('movement', 'camera', 'inventory', 'placement'), 'walking_dict': ('buttons', 'camera')}


@pytest.mark.parametrize('space', DC.SPACES)
def test_entries_reject_bad_arguments_without_a_device(space):
    from gridworld_amd import peek_dict as D
    L = D.load()
    entry = getattr(L, D.SPACES[space][0])
    buf = (ctypes.c_uint8 * 16384)()
    p16 = (ctypes.addressof(buf) + 15) & ~15
    acts = ACTS[space]
    ok = dict({k: p16 for k in STATE + OUT + acts}, n=1, K=4, H=3, per_env=0, right=1.0, wrong=0.1, max_steps=250,
              select=1, gamma=1.0)

    def call(**kw):
        a = dict(ok, **kw)
        return entry(*[a[k] for k in STATE], a['n'], a['K'], a['H'], *[a[k] for k in acts], a['per_env'], a['right'],
                     a['wrong'], a['max_steps'], a['select'], a['gamma'], *[a[k] for k in OUT], None)
    odd = [dict(buttons=p16 + 4), dict(camera=p16 + 2)] if space == 'walking_dict' else [{k: p16 + 2} for k in acts]
    bad = [{k: None} for k in STATE] + [{k: p16 + 8} for k in STATE] + [{k: None} for k in acts] + odd + \
        [{k: None for k in OUT}] + [{k: p16 + 1} for k in OUT] + [dict(reward=p16 + 2), dict(pose=p16 + 2), dict(ret=p16 + 2)] + \
        [dict(n=-1), dict(K=0), dict(K=4097), dict(H=0), dict(H=33), dict(max_steps=0), dict(max_steps=65535),
         dict(gamma=float('inf')), dict(gamma=float('nan')), dict(n=1 << 30, K=4096)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert L.igw_peek_dict_last_error().startswith(b'igw_peek_dict: '), kw
    # nothing is launched for n == 0, whatever subset of the outputs is asked for; the checks come first all the same
    assert call(n=0) == 0 and call(n=0, reward=None, change=None, pose=None) == 0 and call(n=0, ends=p16 + 2, K=4096, H=32) == 0
    assert call(n=0, K=0) == -1 and call(n=0, **{k: None for k in OUT}) == -1 and call(n=0, grid=None) == -1
    assert call(n=0, camera=None) == -1


class _Stub:
    """What _Rows.peek_dict looks at before it touches a device."""

    def __new__(cls, n=4, **kw):
        import torch
        from gridworld_amd import vec_env as V

        class Rows(V._Rows):
            def __del__(self):
                pass
        r = Rows()
        r.num_envs, r.flying, r.walk_dict, r.device = n, True, False, torch.device('cpu')
        r.cfg = types.SimpleNamespace(size_reward=0)
        for k, v in kw.items():
            setattr(r, k, v)
        r._stream = lambda: None
        return r


def _zeros(space, lead):
    return {k: np.zeros(tuple(lead) + shape, dt) for k, dt, shape in DC.FIELDS[space]}


def test_peek_dict_raises_value_error_before_it_touches_a_device():
    import torch
    fly_ok, dict_ok = _zeros('flying', (4, 3)), _zeros('walking_dict', (4, 3))
    with pytest.raises(ValueError, match=r'env\.peek'):
        _Stub(flying=False).peek_dict(fly_ok)                                    # the Discrete(18) space
    for kw, a in ((dict(cfg=types.SimpleNamespace(size_reward=1)), fly_ok),
                  (dict(flying=False, walk_dict=True, cfg=types.SimpleNamespace(size_reward=1)), dict_ok)):
        with pytest.raises(ValueError, match='size_reward'):
            _Stub(**kw).peek_dict(a)
    for space, env in (('flying', _Stub()), ('walking_dict', _Stub(flying=False, walk_dict=True))):
        ok = _zeros(space, (4, 3))
        keys = list(ok)
        other = dict_ok if space == 'flying' else fly_ok
        bad = [other, {k: v for k, v in ok.items() if k != keys[0]}, dict(ok, extra=ok['camera']), ok['camera'], None, [ok]]
        bad += [dict(ok, camera=np.zeros((4, 2, 2), np.float32)), dict(ok, camera=np.zeros((3, 3, 2), np.float32)),   # leading shapes
                dict(ok, camera=np.zeros((4, 4, 3, 2), np.float32)), dict(ok, camera=np.zeros((4, 3, 3), np.float32)),
                dict(ok, camera=np.zeros((4, 3), np.float32)), dict(ok, camera=torch.zeros((4, 3, 1, 2)))]
        bad += [_zeros(space, lead) for lead in ((3,), (2, 2, 2, 2), (5, 4, 3), (3, 4, 3), (4, 33), (4, 0), (0, 3), (4097, 2),
                                                 (4, 4, 33), (4, 0, 3))]
        for actions in bad:
            with pytest.raises(ValueError):
                env.peek_dict(actions)
        for outputs in ((), ('gain',), ('ret', 'want')):
            with pytest.raises(ValueError):
                env.peek_dict(ok, outputs=outputs)
    # env.peek keeps raising for these spaces
    for kw in (dict(), dict(flying=False, walk_dict=True)):
        with pytest.raises(ValueError, match='Discrete'):
            _Stub(**kw).peek(np.zeros((4, 3), np.int32))


def test_device_actions_cast_floats_plainly_and_keep_wide_ids_invalid():
    """What peek_dict hands the kernel for entries that are not device tensors of the ABI dtypes already (on the CPU
    device): movement and camera of any dtype, nested lists included, are the plain float32 cast env.step() makes of
    them; only the id fields keep a value too wide for them invalid instead of wrapping into the valid range."""
    import torch
    from gridworld_amd import peek_dict as D
    cpu = torch.device('cpu')
    cam = np.array([[[45, -30], [-5, 5], [7, -1], [2000000, 0]]], np.int64)
    mv = np.array([[[7, -1, 0], [1, 0, -9], [0, 0, 1], [-1, 1, 0]]], np.int64)
    inv, pl = np.array([[7, -1, (1 << 32) + 3, 6]], np.int64), np.array([[3, (1 << 32) + 1, 2, -1]], np.int64)
    ints = dict(movement=mv, camera=cam, inventory=inv, placement=pl)
    floats = dict(ints, movement=mv.astype(np.float32), camera=cam.astype(np.float32))
    for acts in (ints, floats, {k: torch.from_numpy(v) for k, v in ints.items()}, {k: v.tolist() for k, v in ints.items()},
                 dict(ints, camera=cam.astype(np.float64), movement=mv.astype(np.int16))):
        assert D.shape_of('flying', acts, 9) == (1, 4, False)
        m, c, i, p = D.device_actions('flying', acts, cpu)
        assert m.dtype == c.dtype == torch.float32 and i.dtype == p.dtype == torch.int32
        assert m.tolist() == mv.tolist() and c.tolist() == cam.tolist()
        assert i.tolist() == [[-1, -1, -1, 6]] and p.tolist() == [[3, -1, 2, -1]]
    ready = D.device_actions('flying', ints, cpu)
    again = D.device_actions('flying', dict(zip(ints, ready)), cpu)
    assert all(a is b for a, b in zip(ready, again))                      # what already fits is passed on as it is
    b = np.array([[[256, 0, -1, 0, 1, 0, 2, 300], [0, 0, 0, 0, 0, 0, 0, -2], [1, 1, 0, 0, 0, 0, 1, 6]]], np.int64)
    for acts in (dict(buttons=b, camera=cam[:, :3]), dict(buttons=b.tolist(), camera=cam[:, :3].tolist())):
        assert D.shape_of('walking_dict', acts, 9) == (1, 3, False)
        bb, c = D.device_actions('walking_dict', acts, cpu)
        assert bb.dtype == torch.uint8 and c.dtype == torch.float32 and c.tolist() == cam[:, :3].tolist()
        assert bb.tolist() == [[[1, 0, 1, 0, 1, 0, 1, 255], [0, 0, 0, 0, 0, 0, 0, 255], [1, 1, 0, 0, 0, 0, 1, 6]]]
    with pytest.raises(ValueError):
        D.shape_of('flying', dict(ints, camera=[[[1, 2], [3]]]), 9)        # a ragged list


def test_sanitise_is_the_headers_rule():
    a = DC.pack('flying', [[DC.fly(mv=(DC.NAN, -1, DC.INF), cam=(2e6, -5), inv=7, pl=3), DC.fly(mv=(0.5, 0, 0), cam=(1e6, DC.NAN), inv=6, pl=2),
                            DC.fly(inv=-1, pl=-1, cam=(-DC.INF, -1e6))]])
    s = DC.sanitise('flying', a)
    assert s['movement'][0].tolist() == [[0, -1, 0], [0.5, 0, 0], [0, 0, 0]] and s['camera'][0].tolist() == [[0, -5], [1e6, 0], [0, -1e6]]
    assert s['inventory'][0].tolist() == [0, 6, 0] and s['placement'][0].tolist() == [0, 2, 0]
    b = DC.pack('walking_dict', [[DC.btn(fwd=1, hotbar=7, cam=(DC.NAN, 3)), DC.btn(use=1, hotbar=6, cam=(-2e6, 3)), DC.btn(hotbar=255)]])
    s = DC.sanitise('walking_dict', b)
    assert s['buttons'][0].tolist() == [[1, 0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 1, 6], [0] * 8]
    assert s['camera'][0].tolist() == [[0, 3], [0, 3], [0, 0]]
    assert np.isnan(a['movement'][0, 0, 0]) and b['buttons'][0, 0, 7] == 7   # the inputs are not touched
    d = DC.from_discrete('walking_dict', np.arange(-1, 19))
    assert d['buttons'][1:19].sum(0).tolist() == [1, 1, 1, 1, 1, 1, 1, 21] and not d['buttons'][[0, 1, 19]].any()
    f = DC.from_discrete('flying', np.arange(-1, 19))
    assert f['placement'].tolist() == [0] * 17 + [2, 1, 0] and f['inventory'][7:13].tolist() == [1, 2, 3, 4, 5, 6]


# ---- census --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('space', DC.SPACES)
def test_truth_covers_what_the_gpu_comparison_has_to_tell_apart(space):
    """Over the space's whole case set (eight cases, three checkpoints, the three candidate sets) each situation occurs --
    the floor is peek_cases' FLOOR = 20 candidates (env, k), far above the "at least once" that would do -- so that a
    kernel that never changes a cell, never ends or forgets its own blocks cannot pass the GPU comparison.  Counted on
    the oracle's truth alone.  Measured, flying, 67,584 candidates: a place 41,071; a break 20,651; an end by completion
    955; an end by max_steps 5,920; executed steps with a camera that is not finite 2,199, beyond the limit 1,466, a
    movement that is not finite 2,997, an inventory outside 0..6 2,932, a placement outside 0..2 2,932; directed
    candidates whose future depends on their own block 1,930, of them with another position (a collision) 495.  Walking
    Dict, 72,960 candidates: 43,934; 24,913; 809; 6,592; camera 2,199 and 1,466, a hotbar byte above 6 2,997; own block
    3,499, collisions 1,355."""
    assert list(DC.cases(space)) == list(DC.PC.cases()) and 'short' in DC.cases(space)
    first = DC.FIELDS[space][0][0]
    assert DC.candidates(space, 'random')[first].shape[:3] == (DC.E, 70, 16)
    assert DC.candidates(space, 'shared')[first].shape[:2] == (3, 1)
    assert DC.candidates(space, 'directed')[first].shape[:2] == (len(DC.directed_names(space)), 32)
    cam = np.abs(DC.candidates(space, 'random')['camera'])
    assert cam[:, 0::2].max() <= 5 < cam[:, 1::2].max() <= 90
    got, own, hit = {}, 0, 0
    for name in DC.cases(space):
        for tc in DC.CHECKPOINTS:
            for cset in DC.SETS:
                for k, v in DC.census(space, name, tc, cset).items():
                    got[k] = got.get(k, 0) + v
            own += DC.own_block_hits(space, name, tc)
            hit += DC.own_block_collisions(space, name, tc)
    got['a future that depends on its own block'], got['a collision with its own block'] = own, hit
    for k, v in got.items():
        print('%-45s %d' % (k, v))
    kinds = 5 if space == 'flying' else 3
    assert len(got) == 5 + kinds + 2
    for k, v in got.items():
        assert v >= DC.PC.FLOOR, (k, v)
    # what the directed sequences were written for happens where they were written for it
    names = DC.directed_names(space)
    col = names.index
    d0 = DC.truth(space, 'looking_down', 0, 'directed')
    change, pose = d0['change'].astype(np.int32), d0['pose']
    assert (DC.truth(space, 'short', 12, 'directed')['ends'] == DC.SHORT_STEPS - 12).all()           # the step limit
    nothing = col('nothing' if space == 'flying' else 'discrete_nothing')
    assert (change[:, nothing] == -1).all() and (d0['ends'][:, nothing] == 0).all()
    done = DC.truth(space, 'appendix_b', 0, 'directed')['ends'][:, col('complete_side' if space == 'flying' else 'discrete_complete_side')]
    assert ((done > 0) & (done < 32)).all()                                                          # completed mid-sequence
    empty = DC.truth(space, 'empty_inventory', 0, 'directed')['change'][:, col('same_colour')]
    none = np.arange(DC.E) % 6 == 0                                                                  # no block of colour 1
    assert ((empty >> 11) != 1)[none].all() and ((empty >> 11) == 1).any(-1)[~none].all()
    if space == 'flying':
        pb = change[:, col('place_break')]
        assert (pb[:, 1] >= 2048).all() and (pb[:, 2] == (pb[:, 1] & 0x7ff)).all()                   # placed, then the same cell broken
        assert (pose[:, col('from_above'), 1] > 0.5).all() and (change[:, col('from_above')] >= 2048).any(-1).all()
        assert (np.abs(pose[:, col('leave_x'), 0]) <= 7).all() and (np.abs(pose[:, col('leave_x'), 0]) > 6).all()   # the gate
        assert (pose[:, col('leave_up'), 1] < 10).all() and (pose[:, col('leave_up'), 1] > 9).all()
        assert (np.abs(pose[:, col('leave_z'), 2]) <= 7).all()
        assert (pose[:, col('pitch_clamp'), 3] == -54.5).all()                                       # 90 - 280 clamps to -90, + 35.5
        assert ((pose[:, col('yaw_wrap'), 4] >= 0) & (pose[:, col('yaw_wrap'), 4] <= 360)).all()
        sel = change[:, col('select')]
        with_select = DC.cases(space)['looking_down']['kw'].get('select_and_place', True)
        assert with_select and (sel[:, 1] >= 2048).all() and (sel[:, 2] >> 11 == 3).all() and (sel[:, 3] >> 11 == 4).all()
        off = DC.truth(space, 'select_only', 0, 'directed')['change'].astype(np.int32)[:, col('select')]
        assert (sel[:, 7] >> 11 == 2).all()                                                          # ... and cancels the break
        # without select_and_place a hotbar change alone places nothing and a break beside it stays a break
        assert (off[:, 1] >= 2048).all() and (off[:, 2] == -1).all() and (off[:, 5] >> 11 == 5).all()
        assert (off[:, 6] == (off[:, 5] & 0x7ff)).all() and (off[:, 7] == -1).all()
    else:
        assert (change[:, col('attack_use'), 1] == -1).all() and (change[:, col('attack_use'), 2] >= 2048).all()
        au = change[:, col('attack_use')]
        assert (au[:, 3] == -1).all() and (au[:, 4] == (au[:, 2] & 0x7ff)).all()                     # a no-op again, then the break alone
        assert (au[:, 5] >> 11 == 2).all() and (au[:, 7] >> 11 == 3).all()                           # the hotbar byte places and cancels the break
        assert (change[:, col('hotbar_use'), 1] >> 11 == 5).all()
        two = pose[:, col('two_buttons')]
        assert (two[:, 0] != 0).all() and (two[:, 2] != 0).all()                                     # moved along both axes
        assert (pose[:, col('fractional'), 4] % 5 != 0).all()
