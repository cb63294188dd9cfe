"""CPU side of the peek query: libigw_peek.so as a cross-compiled artefact -- its exports, its code
object, its argument checks --, the ValueErrors of VecGridWorld.peek on a stub without a device, peek_decode / peek_best
on CPU tensors, and the coverage of the oracle truth the GPU test compares against.  The GPU comparison is
tests/test_gpu_peek.py."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

import peek_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = '/opt/rocm/lib/llvm/bin'


def _declared():
    src = open(os.path.join(ROOT, 'include', 'igw_peek.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(igw_[a-z0-9_]+)\s*\(', src)))


# ---- the library -------------------------------------------------------------------------------------------------------
def test_peek_library_cross_compiles_and_exports_its_declared_symbols():
    from gridworld_amd import peek as P
    lib = P.build()
    assert os.path.exists(lib) and os.path.basename(lib) == 'libigw_peek.so'
    L = P.load()
    assert sorted(P.EXPORTS) == _declared()
    assert {'igw_peek_version', 'igw_peek_build_id', 'igw_peek_last_error', 'igw_peek'} == set(P.EXPORTS)
    for name in _declared():
        assert hasattr(L, name)
    assert L.igw_peek_version() == P.VERSION == 1
    assert P.build_id() == P.source_hash() == P.built_id()
    assert not P.is_stale()


def test_peek_sources_are_in_no_other_library():
    """The peek library's files enter no other library's build id, no other library's kernels enter its own, it is built
    with the step library's flags and includes igw_device.h as it is."""
    from gridworld_amd import aim as A, build as B, codec as K, goal as G, peek as P, query as Q, render as R
    others = B.SOURCES + B.HEADERS + R.SOURCES + R.HEADERS + R.OBS_SOURCES + R.OBS_HEADERS + Q.SOURCES + Q.HEADERS + \
        K.LIBRARY.sources + K.LIBRARY.headers + G.SOURCES + G.HEADERS + A.SOURCES + A.HEADERS
    srcs = [os.path.basename(s) for s in others]
    assert 'igw_peek.hip' not in srcs and 'igw_peek.h' not in srcs
    mine = [os.path.basename(s) for s in P.SOURCES + P.HEADERS]
    assert [s for s in mine if s.endswith('.hip')] == ['igw_peek.hip']
    assert not {os.path.basename(s) for s in others if s.endswith('.hip')} & set(mine)
    assert P.LIBRARY.flags == () and os.path.basename(P.LIB) == 'libigw_peek.so'
    assert P.LIBRARY.marker == b'igw-peek-build-id:'
    assert P.LIBRARY.marker not in (Q.LIBRARY.marker, G.LIBRARY.marker, A.LIBRARY.marker, B.STEP.marker)
    # the library's own files: its .hip file, the headers under csrc/peek/ and igw_vote.h
    own = [s for s in P.SOURCES + P.HEADERS if os.path.basename(os.path.dirname(s)) == 'peek' or os.path.basename(s) == 'igw_vote.h']
    assert sorted(os.path.basename(s) for s in own) == ['igw_peek.hip', 'igw_peek_body.h', 'igw_peek_core.h', 'igw_vote.h']
    text = ''.join(open(s).read() for s in own)
    assert '#include "../igw_device.h"' in text
    for name in ('parse_walking_discrete', 'world_act_pre', 'world_act_post', 'finish_break', 'world_update',
                 'syn_size_delta', 'finish_step'):
        assert re.search(r'\b%s\(' % name, text), name   # restated here, not moved out of the step library
    assert not {'igw_peek_body.h', 'igw_peek_core.h', 'igw_vote.h'} & {os.path.basename(s) for s in B.SOURCES + B.HEADERS}


def test_peek_code_object_has_no_scratch_and_no_vector_spills(tmp_path):
    """The notes of the gfx950 code object inside the library, read as tests/test_aim_cpu.py reads the aim's."""
    from gridworld_amd import peek as P
    fat, co = str(tmp_path / 'fat.bin'), str(tmp_path / 'dev.co')
    subprocess.check_call([os.path.join(LLVM, 'llvm-objcopy'), '--dump-section', '.hip_fatbin=' + fat, P.build()])
    subprocess.check_call([os.path.join(LLVM, 'clang-offload-bundler'), '--type=o',
                           '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--input=' + fat, '--output=' + co, '--unbundle'])
    notes = subprocess.check_output([os.path.join(LLVM, 'llvm-readelf'), '--notes', co], text=True)
    kern = [b for b in notes.split('- .agpr_count:')[1:] if 'igw_peek_kernel' in b]
    assert len(kern) == 1
    val = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, kern[0]).group(1))  # noqa: E731
    print('igw_peek_kernel: %d VGPRs, %d SGPRs (%d spilled to vector lanes), %d B of LDS' % (
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
STATE = ('grid', 'occ', 'hist', 'aux', 'agent', 'task_target', 'task_start', 'task_meta', 'task_index')
OUT = ('reward', 'ends', 'change', 'pose', 'ret')


def test_peek_rejects_bad_arguments_without_a_device():
    from gridworld_amd import peek as P
    L = P.load()
    buf = (ctypes.c_uint8 * 16384)()
    p16 = (ctypes.addressof(buf) + 15) & ~15
    ok = dict({k: p16 for k in STATE + OUT}, n=1, K=4, H=3, actions=p16, per_env=0, right=1.0, wrong=0.1, max_steps=250,
              select=1, gamma=1.0)

    def call(**kw):
        a = dict(ok, **kw)
        return L.igw_peek(*[a[k] for k in STATE], a['n'], a['K'], a['H'], a['actions'], a['per_env'], a['right'],
                          a['wrong'], a['max_steps'], a['select'], a['gamma'], *[a[k] for k in OUT], None)
    bad = [{k: None} for k in STATE] + [{k: p16 + 8} for k in STATE] + [dict(actions=None), dict(actions=p16 + 2)] + \
        [{k: None for k in OUT}] + [{k: p16 + 1} for k in OUT] + [dict(reward=p16 + 2), dict(pose=p16 + 2), dict(ret=p16 + 2)] + \
        [dict(n=-1), dict(K=0), dict(K=4097), dict(H=0), dict(H=33), dict(max_steps=0), dict(max_steps=65535),
         dict(gamma=float('inf')), dict(gamma=float('nan')), dict(n=1 << 30, K=4096)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert L.igw_peek_last_error().startswith(b'igw_peek: '), kw
    # nothing is launched for n == 0, whatever subset of the outputs is asked for; the checks come first all the same
    assert call(n=0) == 0 and call(n=0, reward=None, change=None, pose=None) == 0 and call(n=0, ends=p16 + 2, K=4096, H=32) == 0
    assert call(n=0, K=0) == -1 and call(n=0, **{k: None for k in OUT}) == -1 and call(n=0, grid=None) == -1


class _Stub:
    """What _Rows.peek looks at before it touches a device."""

    def __new__(cls, n=4, **kw):
        import torch
        from gridworld_amd import vec_env as V

        class Rows(V._Rows):
            def __del__(self):
                pass
        r = Rows()
        r.num_envs, r.flying, r.walk_dict, r.device = n, False, False, torch.device('cpu')
        r.cfg = types.SimpleNamespace(size_reward=0)
        for k, v in kw.items():
            setattr(r, k, v)
        r._stream = lambda: None
        return r


def test_peek_raises_value_error_before_it_touches_a_device():
    import torch
    ok = np.zeros((4, 3), np.int32)
    for kw in (dict(flying=True), dict(walk_dict=True), dict(cfg=types.SimpleNamespace(size_reward=1))):
        with pytest.raises(ValueError):
            _Stub(**kw).peek(ok)
    env = _Stub()
    for actions in (np.zeros(3, np.int32), np.zeros((2, 2, 2, 2), np.int32), np.zeros((5, 4, 3), np.int32),
                    np.zeros((3, 4, 3), np.int32), np.zeros((4, 33), np.int32), np.zeros((4, 0), np.int32),
                    np.zeros((0, 3), np.int32), np.zeros((4097, 2), np.int32), np.zeros((4, 3), np.float32),
                    torch.zeros((4, 3)), torch.zeros((4, 3), dtype=torch.bool), torch.zeros((4, 4, 33), dtype=torch.int64)):
        with pytest.raises(ValueError):
            env.peek(actions)
    for outputs in ((), ('gain',), ('ret', 'want')):
        with pytest.raises(ValueError):
            env.peek(ok, outputs=outputs)


# ---- peek_decode / peek_best -----------------------------------------------------------------------------------------------
def test_peek_decode_and_peek_best_on_hand_written_values():
    import torch
    import gridworld_amd as G
    codes = torch.tensor([[-1, 0, 1088, (6 << 11) | 1088], [(1 << 11) | 5, 5, -1, (3 << 11)]], dtype=torch.int16)
    cell, colour = G.peek_decode(codes)
    assert cell.tolist() == [[-1, 0, 1088, 1088], [5, 5, -1, 0]] and colour.tolist() == [[-1, 0, 0, 6], [1, 0, -1, 3]]
    assert cell.dtype == colour.dtype == torch.int32 and cell.shape == codes.shape
    cell_np, _ = G.peek_decode(codes.numpy())
    assert cell_np.tolist() == cell.tolist()
    ret = torch.tensor([[0.0, 1.5, 1.5, -2.0], [-1.0, -1.0, -3.0, -1.0], [0.0, -0.0, 0.0, 0.0], [1.0, 2.0, 3.0, 4.0]])
    best = G.peek_best(ret)
    assert best.tolist() == [1, 0, 0, 3] and best.dtype == torch.int64
    assert G.peek_best(ret[:, :1]).tolist() == [0, 0, 0, 0]
    nan = float('nan')
    odd = torch.tensor([[nan, nan, nan], [nan, -5.0, nan], [nan, float('inf'), float('inf')], [-float('inf'), nan, -float('inf')]])
    assert G.peek_best(odd).tolist() == [0, 1, 1, 0]       # a NaN ranks below every number; always an index below K


def test_reward64_and_returns_follow_the_header():
    r32 = np.array([0.0, 0.1, -0.1, 1.0, -2.0, 3.0], np.float32)
    r64 = PC.reward64(r32)
    assert r64.tolist() == [0.0, 1 * 0.1, -1 * 0.1, 1.0, -2.0, 3.0] and r64.dtype == np.float64
    assert np.array_equal(r64.astype(np.float32), r32)
    with pytest.raises(KeyError):
        PC.reward64(np.array([0.25], np.float32))
    x = PC.returns(np.array([[0.1, 0.1, 1.0]]), 0.97)
    assert x.dtype == np.float32 and x[0] == np.float32((0.0 + 1.0 * 0.1) + 0.97 * 0.1 + (0.97 * 0.97) * 1.0)


# ---- coverage ------------------------------------------------------------------------------------------------------------
def test_truth_covers_what_the_gpu_comparison_has_to_tell_apart():
    """The floors that keep the GPU comparison from passing on a kernel that forgets its own changes: at least FLOOR = 20
    candidates (env, k) in each situation, counted on the oracle's truth of the `random` and `directed` sets alone (tree2,
    82,944 more candidates per checkpoint, adds to every count but the step limit's and the own-block one).  Measured, all cases and checkpoints, random +
    directed, 64,512 candidates: a place 36,901; a break 32,960; two or more changes 33,612; a cell changed again 29,141;
    an unpaid change, then a paid placement 1,665; an end by completion 574; an end by max_steps 5,824; more than 2
    sub-steps 2,913; right > 0 23,600; right < 0 18,449; wrong > 0 17,947; wrong < 0 25,201; a collision with or a ray
    hit on its own block (directed against `ghost`) 2,185."""
    assert list(PC.cases()) == list(PC.MC.cases()) + ['recolour', 'short']
    assert PC.candidates('tree2').shape == (324, 2) and len({tuple(r) for r in PC.candidates('tree2').tolist()}) == 324
    assert PC.candidates('random').shape == (PC.E, 70, 16) and PC.candidates('directed').shape == (len(PC.DIRECTED), 32)
    assert {18, -1} <= set(PC.candidates('directed').reshape(-1).tolist())
    got, own = {}, 0
    for name in PC.cases():
        for tc in PC.CHECKPOINTS:
            for cset in ('random', 'directed'):
                for k, v in PC.coverage(name, tc, cset).items():
                    got[k] = got.get(k, 0) + v
            own += PC.own_block_hits(name, tc)
    got['a collision with or a ray hit on its own block'] = own
    for k, v in got.items():
        print('%-50s %d' % (k, v))
    assert got['candidates'] == 8 * 3 * PC.E * (70 + len(PC.DIRECTED))
    for k, v in got.items():
        assert v >= PC.FLOOR, (k, v)
    # what the directed sequences were written for happens where they were written for it
    d0 = PC.truth('looking_down', 0, 'directed')
    col = lambda n: PC.DIRECTED_NAMES.index(n)  # noqa: E731
    change = d0['change'].astype(np.int32)
    pb = change[:, col('place_break')]
    assert (pb[:, 9] >= 2048).all() and (pb[:, 10] == (pb[:, 9] & 0x7ff)).all()        # placed, then the same cell broken
    assert (d0['drop'][:, col('jump')] > 0.3).any(-1).all()                      # a fall faster than 5 per second
    assert (change[:, col('no_ops'), [0, 1, 4, 7, 14, 16]] == -1).all()
    done = PC.truth('appendix_b', 0, 'directed')['ends'][:, col('complete_side')]
    assert ((done > 0) & (done < 32)).all()                                            # the target completed mid-sequence
    short = PC.truth('short', 12, 'directed')['ends']
    assert (short == PC.SHORT_STEPS - 12).all()                                        # ... and the step limit
    rec = PC.truth('recolour', 0, 'directed')
    r, c = rec['reward'][:, col('recolour')], rec['change'][:, col('recolour')]
    assert ((c[:, :14] >= 0) & (r[:, :14] == 0)).any(-1).all()                         # a change with wrong == 0 ...
    assert ((c[:, 14:] >= 2048) & (r[:, 14:] != 0)).any(-1).all()                      # ... and a paid placement after it
