"""CPU side of the action mask: libigw_query.so as a cross-compiled artefact -- its exports, its
code object, its argument checks -- and the coverage of the oracle truth the GPU test compares against
(tests/mask_cases.py).  The GPU comparison is tests/test_gpu_action_mask.py."""
import ctypes
import os
import re
import subprocess

import numpy as np

import mask_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = '/opt/rocm/lib/llvm/bin'


def _declared():
    src = open(os.path.join(ROOT, 'include', 'igw_query.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(igw_[a-z0-9_]+)\s*\(', src)))


def test_query_library_cross_compiles_and_exports_its_declared_symbols():
    from gridworld_amd import query as Q
    lib = Q.build()
    assert os.path.exists(lib) and os.path.basename(lib) == 'libigw_query.so'
    L = Q.load()
    assert sorted(Q.EXPORTS) == _declared()
    assert {'igw_query_version', 'igw_query_build_id', 'igw_action_mask'} <= set(Q.EXPORTS)
    for name in _declared():
        assert hasattr(L, name)
    assert L.igw_query_version() == Q.VERSION == 1
    assert Q.build_id() == Q.source_hash() == Q.built_id()
    assert not Q.is_stale()


def test_query_code_object_has_no_scratch_and_no_spills(tmp_path):
    """The notes of the gfx950 code object inside the library, read as tests/render_checks.py reads the renderer's."""
    from gridworld_amd import query as Q
    fat, co = str(tmp_path / 'fat.bin'), str(tmp_path / 'dev.co')
    subprocess.check_call([os.path.join(LLVM, 'llvm-objcopy'), '--dump-section', '.hip_fatbin=' + fat, Q.build()])
    subprocess.check_call([os.path.join(LLVM, 'clang-offload-bundler'), '--type=o',
                           '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--input=' + fat, '--output=' + co, '--unbundle'])
    notes = subprocess.check_output([os.path.join(LLVM, 'llvm-readelf'), '--notes', co], text=True)
    kern = [b for b in notes.split('- .agpr_count:')[1:] if 'igw_action_mask_kernel' in b]
    assert len(kern) == 1
    val = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, kern[0]).group(1))  # noqa: E731
    print('igw_action_mask_kernel: %d VGPRs, %d SGPRs, %d B of LDS' % (val('vgpr_count'), val('sgpr_count'),
                                                                       val('group_segment_fixed_size')))
    assert val('private_segment_fixed_size') == 0
    assert val('vgpr_spill_count') == 0 and val('sgpr_spill_count') == 0
    assert re.search(r'\.uses_dynamic_stack:\s+false', kern[0])
    assert val('vgpr_count') <= 128                       # four wavefronts per SIMD at the least
    assert val('group_segment_fixed_size') <= 32 * 1024   # five blocks per CU at the least
    assert re.search(r'\.max_flat_workgroup_size:\s+256', kern[0])


def test_action_mask_rejects_bad_arguments_without_a_device():
    from gridworld_amd import query as Q
    L = Q.load()
    buf = (ctypes.c_uint8 * 4096)()
    p16 = (ctypes.addressof(buf) + 15) & ~15
    ok = dict(agent=p16, occ=p16, n=1, mask=p16, look=p16, actions=p16)

    def call(**kw):
        a = dict(ok, **kw)
        return L.igw_action_mask(a['agent'], a['occ'], a['n'], 1, a['mask'], a['look'], a['actions'], 0, 0, 0, None)
    for bad in (dict(agent=None), dict(occ=None), dict(mask=None), dict(n=-1), dict(agent=p16 + 8), dict(occ=p16 + 4),
                dict(look=p16 + 1), dict(actions=p16 + 2)):
        assert call(**bad) == -1, bad
        assert L.igw_query_last_error().startswith(b'igw_action_mask: ')
    assert call(n=0) == 0 and call(n=0, look=None, actions=None) == 0   # a no-op: nothing is launched


def test_query_sources_are_in_no_other_library():
    """The query library's files enter no other library's build id."""
    from gridworld_amd import build as B, render as R
    srcs = [os.path.basename(s) for s in B.SOURCES + B.HEADERS + R.SOURCES + R.HEADERS + R.OBS_SOURCES + R.OBS_HEADERS]
    assert 'igw_query.hip' not in srcs and 'igw_query.h' not in srcs


def test_action_names():
    import gridworld_amd as G
    assert len(G.action_mask_names) == 18 and len(set(G.action_mask_names)) == 18
    assert [G.action_mask_names[a] for a in (0, 5, 16, 17)] == ['noop', 'jump', 'break', 'place']


def test_oracle_truth_covers_both_values_of_every_conditional_bit():
    """The floor that keeps the GPU comparison from passing on constant masks: over all cases, each conditional bit is
    0 in at least 20 (env, checkpoint) pairs and 1 in at least 20, and both `look` cells exist in at least 20."""
    masks, looks = zip(*(MC.truth(name) for name in MC.cases()))
    m, lk = np.concatenate(masks).reshape(-1, 18), np.concatenate(looks).reshape(-1, 2)
    assert len(m) == len(MC.cases()) * len(MC.CHECKPOINTS) * MC.E
    ones, zeros = m.sum(0), (1 - m).sum(0)
    print('pairs with the bit set:  ', ones.tolist())
    print('pairs with the bit clear:', zeros.tolist())
    print('pairs with a break / place cell:', (lk >= 0).sum(0).tolist())
    assert (m[:, [0, 1, 2, 3, 4, 12, 13]] == 1).all()
    for b in MC.CONDITIONAL:
        assert ones[b] >= MC.FLOOR and zeros[b] >= MC.FLOOR, b
    assert ((lk >= 0).sum(0) >= MC.FLOOR).all()
    assert ((lk[:, 0] >= 0) == (m[:, 16] == 1)).all() and ((lk[:, 1] >= 0) == (m[:, 17] == 1)).all()
    # the cases do what their names say
    t = {name: MC.truth(name)[0] for name in MC.cases()}
    colour = 1 + np.arange(MC.E) % 6
    first = t['empty_inventory'][0]                    # at reset: the colour of the starting grid cannot be placed ...
    assert not first[np.arange(MC.E), 5 + colour].any()
    looking = t['empty_inventory'][3]                  # ... where the others can
    rows = looking[:, 6:12].any(1)
    assert rows.sum() >= 8 and not looking[rows, 5 + colour[rows]].any()
    assert (looking[rows, 6:12].sum(1) >= 4).all()
    assert (t['select_only'][:, :, 6:12].sum(2) == 5).all()                     # all but the active colour
    assert not t['init_pose'][:, :8, 14].any() and not t['init_pose'][:, 8:16, 15].any()
    b = t['appendix_b']                                # env 0 runs the script from step 0: at step 12 it can place
    assert b[3, 0, 17] == 1 and b[3, 0, 16] == 0
