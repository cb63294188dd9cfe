"""CPU side of the goal query: libigw_goal.so as a cross-compiled artefact -- its exports, its code
object, its argument checks -- and the coverage of the oracle truth the GPU test compares against
(tests/goal_cases.py).  The GPU comparison is tests/test_gpu_goal.py."""
import ctypes
import os
import re
import subprocess

import numpy as np

import goal_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = '/opt/rocm/lib/llvm/bin'


def _declared():
    src = open(os.path.join(ROOT, 'include', 'igw_goal.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(igw_[a-z0-9_]+)\s*\(', src)))


def test_goal_library_cross_compiles_and_exports_its_declared_symbols():
    from gridworld_amd import goal as G
    lib = G.build()
    assert os.path.exists(lib) and os.path.basename(lib) == 'libigw_goal.so'
    L = G.load()
    assert sorted(G.EXPORTS) == _declared()
    assert {'igw_goal_version', 'igw_goal_build_id', 'igw_goal_last_error', 'igw_goal'} == set(G.EXPORTS)
    for name in _declared():
        assert hasattr(L, name)
    assert L.igw_goal_version() == G.VERSION == 1
    assert G.build_id() == G.source_hash() == G.built_id()
    assert not G.is_stale()


def test_goal_sources_are_in_no_other_library():
    """The goal library's files enter no other library's build id, and it is built with the step library's flags."""
    from gridworld_amd import build as B, codec as K, goal as G, query as Q, render as R
    srcs = [os.path.basename(s) for s in B.SOURCES + B.HEADERS + R.SOURCES + R.HEADERS + R.OBS_SOURCES + R.OBS_HEADERS +
            Q.SOURCES + Q.HEADERS + K.LIBRARY.sources + K.LIBRARY.headers]
    assert 'igw_goal.hip' not in srcs and 'igw_goal.h' not in srcs
    assert G.LIBRARY.flags == () and os.path.basename(G.LIB) == 'libigw_goal.so'
    assert G.LIBRARY.marker == b'igw-goal-build-id:' and G.LIBRARY.marker != Q.LIBRARY.marker


def test_goal_code_object_has_no_scratch_and_no_spills(tmp_path):
    """The notes of the gfx950 code object inside the library, read as tests/test_query_cpu.py reads the query's."""
    from gridworld_amd import goal as G
    fat, co = str(tmp_path / 'fat.bin'), str(tmp_path / 'dev.co')
    subprocess.check_call([os.path.join(LLVM, 'llvm-objcopy'), '--dump-section', '.hip_fatbin=' + fat, G.build()])
    subprocess.check_call([os.path.join(LLVM, 'clang-offload-bundler'), '--type=o',
                           '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--input=' + fat, '--output=' + co, '--unbundle'])
    notes = subprocess.check_output([os.path.join(LLVM, 'llvm-readelf'), '--notes', co], text=True)
    kern = [b for b in notes.split('- .agpr_count:')[1:] if 'igw_goal_kernel' in b]
    assert len(kern) == 1
    val = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, kern[0]).group(1))  # noqa: E731
    print('igw_goal_kernel: %d VGPRs, %d SGPRs, %d B of LDS' % (val('vgpr_count'), val('sgpr_count'),
                                                                val('group_segment_fixed_size')))
    assert val('private_segment_fixed_size') == 0
    assert val('vgpr_spill_count') == 0 and val('sgpr_spill_count') == 0
    assert re.search(r'\.uses_dynamic_stack:\s+false', kern[0])
    assert val('vgpr_count') <= 128
    assert val('group_segment_fixed_size') <= 80 * 1024   # two blocks per CU at the least (160 KiB of LDS)
    assert re.search(r'\.max_flat_workgroup_size:\s+256', kern[0])


def test_goal_rejects_bad_arguments_without_a_device():
    from gridworld_amd import goal as G
    L = G.load()
    buf = (ctypes.c_uint8 * 8192)()
    p16 = (ctypes.addressof(buf) + 15) & ~15
    state = ('grid', 'hist', 'aux', 'agent', 'task_target', 'task_start', 'task_meta', 'task_index')
    ok = dict({k: p16 for k in state + ('mask', 'look') + G.OUTPUTS}, n=1, max_steps=250)

    def call(**kw):
        a = dict(ok, **kw)
        return L.igw_goal(*[a[k] for k in state], a['n'], 1.0, 0.1, a['max_steps'], 1, a['mask'], a['look'],
                          *[a[k] for k in G.OUTPUTS], None)
    bad = [{k: None} for k in state] + [{k: p16 + 8} for k in state] + \
        [dict(n=-1), dict(align=p16 + 2), dict(fit=p16 + 4), dict(want=p16 + 8), dict(todo=p16 + 4), dict(gain=p16 + 2),
         dict(look=p16 + 1), dict(mask=None), dict(look=None), dict(mask=None, gain=None), dict(look=None, ends=None),
         dict(max_steps=0), dict(max_steps=65535)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert L.igw_goal_last_error().startswith(b'igw_goal: ')
    none = {k: None for k in G.OUTPUTS}
    assert call(n=0) == 0 and call(n=0, **none) == 0                 # a no-op: nothing is launched
    assert call(n=0, mask=None, look=None, gain=None, ends=None) == 0   # mask and look go with gain and ends only


def test_goal_world_names_the_block_ids_wanted():
    import torch
    import gridworld_amd as G
    want = torch.tensor([[0, 2, 1, -1, 3, -2]], dtype=torch.int8)
    start = torch.tensor([[0, 0, 1, 1, 4, 1]], dtype=torch.int8)
    assert G.goal_world(want, start).tolist() == [[0, 2, 2, 0, -1, -1]]
    assert G.goal_world(want, start).dtype == torch.int8


def _all(names, key):
    return np.concatenate([GC.truth(n)[key] for n in names])


def test_oracle_truth_covers_what_the_gpu_comparison_has_to_tell_apart():
    """The floors that keep the GPU comparison from passing on constants (conditions; measured counts are printed)."""
    six = list(GC.MC.cases())
    assert len(six) == 6 and list(GC.cases()) == six + ['recolour']
    fit, align = _all(six, 'fit').reshape(-1, 4), _all(six, 'align').reshape(-1, 3)
    assert len(fit) == 6 * len(GC.CHECKPOINTS) * GC.E == 1152
    cols = [p for p in GC.PROBES]
    gain, ends, changed = _all(six, 'gain')[..., cols].reshape(-1), _all(six, 'ends')[..., cols].reshape(-1), \
        _all(six, 'changed').reshape(-1)
    assert len(gain) == 9216
    rs, ws = np.float32(GC.RIGHT), np.float32(GC.WRONG)
    got = {'live max_int > 0': int((fit[:, 0] > 0).sum()), 'align != 0': int(align.any(1).sum()),
           'rot 1': int((align[:, 2] == 1).sum()), 'rot 2': int((align[:, 2] == 2).sum()),
           'rot 3': int((align[:, 2] == 3).sum()),
           '+right': int((gain == rs).sum()), '-right': int((gain == -rs).sum()),
           '+wrong': int((gain == ws).sum()), '-wrong': int((gain == -ws).sum()),
           'changed, gain 0': int((changed & (gain == 0)).sum()), 'ends by completion': int((ends == 1).sum()),
           'cached != live (six cases)': int((fit[:, 0] != fit[:, 3]).sum())}
    r = GC.truth('recolour')
    rc = r['gain'][..., cols]
    got['recolour: cached != live'] = int((r['fit'][..., 0] != r['fit'][..., 3]).sum())
    got['recolour: reward differs from the live maximum\'s'] = int((r['changed'] & (rc != r['live'])).sum())
    for k, v in got.items():
        print('%-50s %d' % (k, v))
    floors = {'live max_int > 0': 200, 'align != 0': 200, 'rot 1': 5, 'rot 2': 5, 'rot 3': 5, '+right': 100, '-right': 100,
              '+wrong': 100, '-wrong': 100, 'changed, gain 0': 10, 'ends by completion': 20,
              'recolour: cached != live': 20, 'recolour: reward differs from the live maximum\'s': 20}
    for k, v in floors.items():
        assert got[k] >= v, (k, got[k], v)
    # what the truth is made of holds together
    for name in GC.cases():
        t = GC.truth(name)
        assert (t['fit'][..., 0] <= t['fit'][..., 1]).all() and (t['fit'][..., 0] <= t['fit'][..., 2]).all()
        assert ((t['want'] != 0).sum((2, 3, 4)) <= t['fit'][..., 1]).all()
        assert (np.where(t['todo'] != 0, t['want'], 0) == t['todo']).all()
        idle = [a for a in range(18) if a not in GC.PROBES]
        assert (t['gain'][..., idle] == 0).all()
    # the script of `recolour` does what it says: env 0 at step 25 has placed over the broken block and turned away;
    # the placing probes are paid from the cached 0, the break probe has nothing to break
    assert r['fit'][4, 0].tolist() == [1, 3, 1, 0]
    assert r['gain'][4, 0, [6, 7, 8, 9, 10, 11, 17]].tolist() == [2, 1, 2, 1, 1, 1, 1] and r['gain'][4, 0, 16] == 0
