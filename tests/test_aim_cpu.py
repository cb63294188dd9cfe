"""CPU side of the aim query: libigw_aim.so as a cross-compiled artefact -- its exports, its code
object, its argument checks --, aim_decode / aim_action on CPU tensors, the model of tests/aim_cases.py against the
oracle probe, and the coverage of the truth the GPU test compares against.  The GPU comparison is
tests/test_gpu_aim.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import aim_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = '/opt/rocm/lib/llvm/bin'


def _declared():
    src = open(os.path.join(ROOT, 'include', 'igw_aim.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(igw_[a-z0-9_]+)\s*\(', src)))


# ---- the library -------------------------------------------------------------------------------------------------------
def test_aim_library_cross_compiles_and_exports_its_declared_symbols():
    from gridworld_amd import aim as A
    lib = A.build()
    assert os.path.exists(lib) and os.path.basename(lib) == 'libigw_aim.so'
    L = A.load()
    assert sorted(A.EXPORTS) == _declared()
    assert {'igw_aim_version', 'igw_aim_build_id', 'igw_aim_last_error', 'igw_aim'} == set(A.EXPORTS)
    for name in _declared():
        assert hasattr(L, name)
    assert L.igw_aim_version() == A.VERSION == 1
    assert A.build_id() == A.source_hash() == A.built_id()
    assert not A.is_stale()


def test_aim_sources_are_in_no_other_library():
    """The aim library's files enter no other library's build id, no other library's kernels enter its own, and it is
    built with the step library's flags."""
    from gridworld_amd import aim as A, build as B, codec as K, goal as G, query as Q, render as R
    others = B.SOURCES + B.HEADERS + R.SOURCES + R.HEADERS + R.OBS_SOURCES + R.OBS_HEADERS + Q.SOURCES + Q.HEADERS + \
        K.LIBRARY.sources + K.LIBRARY.headers + G.SOURCES + G.HEADERS
    srcs = [os.path.basename(s) for s in others]
    assert 'igw_aim.hip' not in srcs and 'igw_aim.h' not in srcs
    mine = [os.path.basename(s) for s in A.SOURCES + A.HEADERS]
    assert [s for s in mine if s.endswith('.hip')] == ['igw_aim.hip']
    assert not {os.path.basename(s) for s in others if s.endswith('.hip')} & set(mine)
    assert A.LIBRARY.flags == () and os.path.basename(A.LIB) == 'libigw_aim.so'
    assert A.LIBRARY.marker == b'igw-aim-build-id:'
    assert A.LIBRARY.marker not in (Q.LIBRARY.marker, G.LIBRARY.marker, B.STEP.marker)
    text = open(A.SOURCES[0]).read()
    assert '#include "../igw_device.h"' in text


def test_aim_code_object_has_no_scratch_and_no_spills(tmp_path):
    """The notes of the gfx950 code object inside the library, read as tests/test_goal_cpu.py reads the goal's."""
    from gridworld_amd import aim as A
    fat, co = str(tmp_path / 'fat.bin'), str(tmp_path / 'dev.co')
    subprocess.check_call([os.path.join(LLVM, 'llvm-objcopy'), '--dump-section', '.hip_fatbin=' + fat, A.build()])
    subprocess.check_call([os.path.join(LLVM, 'clang-offload-bundler'), '--type=o',
                           '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--input=' + fat, '--output=' + co, '--unbundle'])
    notes = subprocess.check_output([os.path.join(LLVM, 'llvm-readelf'), '--notes', co], text=True)
    kern = [b for b in notes.split('- .agpr_count:')[1:] if 'igw_aim_kernel' in b]
    assert len(kern) == 1
    val = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, kern[0]).group(1))  # noqa: E731
    print('igw_aim_kernel: %d VGPRs, %d SGPRs, %d B of LDS' % (val('vgpr_count'), val('sgpr_count'),
                                                               val('group_segment_fixed_size')))
    assert val('private_segment_fixed_size') == 0
    assert val('vgpr_spill_count') == 0 and val('sgpr_spill_count') == 0
    assert re.search(r'\.uses_dynamic_stack:\s+false', kern[0])
    assert val('vgpr_count') <= 128
    assert val('group_segment_fixed_size') <= 64 * 1024
    assert re.search(r'\.max_flat_workgroup_size:\s+256', kern[0])


# ---- the arguments -----------------------------------------------------------------------------------------------------
def test_aim_rejects_bad_arguments_without_a_device():
    from gridworld_amd import aim as A
    L = A.load()
    buf = (ctypes.c_uint8 * 16384)()
    p16 = (ctypes.addressof(buf) + 15) & ~15
    ok = dict(agent=p16, occ=p16, n=1, max_turns=72, place=p16, brk=p16)

    def call(**kw):
        a = dict(ok, **kw)
        return L.igw_aim(a['agent'], a['occ'], a['n'], a['max_turns'], a['place'], a['brk'], None)
    bad = [dict(agent=None), dict(occ=None), dict(place=None, brk=None)] + \
        [{k: p16 + 8} for k in ('agent', 'occ', 'place', 'brk')] + [dict(place=p16 + 4), dict(brk=None, place=p16 + 1)] + \
        [dict(n=-1), dict(max_turns=-1), dict(max_turns=73)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert L.igw_aim_last_error().startswith(b'igw_aim: '), kw
    assert call(n=0) == 0 and call(n=0, place=None) == 0 and call(n=0, brk=None, max_turns=0) == 0   # nothing is launched
    assert call(n=0, place=None, brk=None) == -1 and call(n=0, max_turns=73) == -1


def test_launch_raises_value_error_before_it_touches_a_device():
    from gridworld_amd import aim as A
    with pytest.raises(ValueError):
        A.launch(None, None, 4, 73, True, True, None, None, None)
    with pytest.raises(ValueError):
        A.launch(None, None, 4, -1, True, True, None, None, None)
    with pytest.raises(ValueError):
        A.launch(None, None, 4, 72, False, False, None, None, None)


# ---- aim_decode / aim_action ---------------------------------------------------------------------------------------------
def test_aim_decode_and_aim_action_on_hand_written_codes():
    import torch
    import gridworld_amd as G
    code = AC.code_of
    cases = [(-1, (-1, 0, 0), 0), (code(0, 0), (0, 0, 0), None), (code(-3, 2), (5, -3, 2), 12), (code(4, -1), (5, 4, -1), 13),
             (code(0, -2), (2, 0, -2), 14), (code(0, 36), (36, 0, 36), 15), (code(-36, -36), (72, -36, -36), 12),
             (code(35, 36), (71, 35, 36), 13), (code(1, 1), (2, 1, 1), 13), (code(-1, -1), (2, -1, -1), 12)]
    codes = torch.tensor([c for c, _, _ in cases], dtype=torch.int32)
    turns, di, dj = G.aim_decode(codes)
    assert turns.tolist() == [w[0] for _, w, _ in cases]
    assert di.tolist() == [w[1] for _, w, _ in cases] and dj.tolist() == [w[2] for _, w, _ in cases]
    assert turns.dtype == di.dtype == dj.dtype == torch.int32
    # one env per case: the code sits in cell 7 + k of a plane that is -1 elsewhere
    n = len(cases)
    base = torch.full((n, AC.ROW), -1, dtype=torch.int32)
    plane = torch.as_strided(base, (n, 9, 11, 11), (AC.ROW, 121, 11, 1))
    cells = torch.arange(n) + 7
    base[torch.arange(n), cells] = codes
    for kind, last in (('place', 17), ('break', 16)):
        got = G.aim_action(plane, cells, kind=kind)
        assert got.dtype == torch.int32 and tuple(got.shape) == (n,)
        assert got.tolist() == [last if a is None else a for _, _, a in cases], kind
    assert G.aim_action(plane, cells.to(torch.int32)).tolist() == G.aim_action(plane, cells).tolist()
    assert G.aim_action(plane, torch.full((n,), -1)).tolist() == [0] * n           # no cell asked for
    assert G.aim_action(plane, cells + 1).tolist() == [0] * n                      # a cell nothing reaches
    assert G.aim_action(base[:, :AC.CELLS], cells).tolist() == G.aim_action(plane, cells).tolist()
    with pytest.raises(ValueError):
        G.aim_action(plane, cells, kind='look')


# ---- model = probe -------------------------------------------------------------------------------------------------------
def _differ(grid, pose, max_turns):
    m = AC.model(grid, pose, max_turns)
    place, brk = AC.probe(grid, pose, max_turns)
    return int((place != m['place']).sum()), int((brk != m['brk']).sum()), int((place >= 0).sum()), int((brk >= 0).sum())


FULL = (('directed', 0, 1), ('directed', 2, 5), ('towers', 2, 3), ('init_pose', 1, 20))


@pytest.mark.parametrize('name,c,e', FULL)
def test_model_equals_probe_over_the_full_window(name, c, e):
    grids, poses, _ = AC.states(name)
    dp, db, np_, nb = _differ(grids[c, e], poses[c, e], 72)
    print(f'{name} checkpoint {AC.CHECKPOINTS[c]} env {e}: {np_} place cells, {nb} break cells; cells that differ: '
          f'{dp} place, {db} break')
    assert np_ + nb > 0 and dp == 0 and db == 0


@pytest.mark.parametrize('name', ['directed', 'towers'])
def test_model_equals_probe_on_every_state_at_six_turns(name):
    grids, poses, _ = AC.states(name)
    bad = cells = 0
    for c in range(grids.shape[0]):
        for e in range(grids.shape[1]):
            dp, db, np_, nb = _differ(grids[c, e], poses[c, e], 6)
            bad, cells = bad + dp + db, cells + np_ + nb
    print(f'{name}: {grids.shape[0] * grids.shape[1]} states, {cells} reachable cells, {bad} differ')
    assert cells > 0 and bad == 0


# ---- coverage ------------------------------------------------------------------------------------------------------------
def test_truth_covers_what_the_gpu_comparison_has_to_tell_apart():
    """The floors that keep the GPU comparison from passing on constants (conditions; measured counts are printed)."""
    assert list(AC.cases()) == list(AC.MC.cases()) + ['directed']
    got = dict.fromkeys(('states', 'place cells', 'break cells', 'states with a place cell at turns 0',
                         'place cells on level 1 or above', 'directions refused by the overlap',
                         'directions refused by the build zone', 'states with no place cell',
                         'states with a winner at di = -36', 'cells whose tie the rule resolves'), 0)
    for name, c, e, grid, pose in AC.all_states():
        m = AC.model(grid, pose, 72)
        place, brk = m['place'], m['brk']
        got['states'] += 1
        got['place cells'] += int((place >= 0).sum())
        got['break cells'] += int((brk >= 0).sum())
        got['states with a place cell at turns 0'] += int((place == AC.code_of(0, 0)).any())
        got['place cells on level 1 or above'] += int((place[121:] >= 0).sum())
        got['directions refused by the overlap'] += int(m['overlap'].sum())
        got['directions refused by the build zone'] += int(m['off_zone'].sum())
        got['states with no place cell'] += int(not (place >= 0).any())
        won = np.concatenate([place[place >= 0], brk[brk >= 0]])
        got['states with a winner at di = -36'] += int(((won & 0xff) == 0).any())
        # a tie: a second direction with the winner's cell and the winner's turns
        for cells, plane in ((m['place_cell'], place), (m['break_cell'], brk)):
            ok = cells >= 0
            same = (m['codes'][ok] >> 16) == (plane[cells[ok]] >> 16)
            got['cells whose tie the rule resolves'] += int((np.bincount(cells[ok][same], minlength=AC.CELLS) >= 2).sum())
    for k, v in got.items():
        print('%-45s %d' % (k, v))
    floors = {'states': 6 * 3 * 32 + 3 * 8, 'place cells': 2000, 'break cells': 150,
              'states with a place cell at turns 0': 100, 'place cells on level 1 or above': 200,
              'directions refused by the overlap': 20, 'directions refused by the build zone': 20,
              'states with no place cell': 5, 'states with a winner at di = -36': 30,
              'cells whose tie the rule resolves': 100}
    for k, v in floors.items():
        assert got[k] >= v, (k, got[k], v)
