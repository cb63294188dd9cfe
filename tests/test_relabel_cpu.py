"""CPU side of the relabel query: libigw_relabel.so as a cross-compiled artefact -- its exports, its
code object, its argument checks --, the host-side checks of gridworld_amd/relabel.py, and the numpy model the GPU test
leans on (tests/relabel_model.py on tests/relabel_cases.py), pinned to the stepped CPU oracle and counted for coverage.
The GPU comparison is tests/test_gpu_relabel.py."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from gridworld_amd import relabel as _feature  # noqa: F401  (without the query nothing in this file can run)

import relabel_cases as RC
import relabel_model as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = '/opt/rocm/lib/llvm/bin'


def _declared():
    src = open(os.path.join(ROOT, 'include', 'igw_relabel.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(igw_[a-z0-9_]+)\s*\(', src)))


def test_relabel_library_cross_compiles_and_exports_its_declared_symbols():
    from gridworld_amd import relabel as R
    lib = R.build()
    assert os.path.exists(lib) and os.path.basename(lib) == 'libigw_relabel.so'
    L = R.load()
    assert sorted(R.EXPORTS) == _declared()
    assert {'igw_relabel_version', 'igw_relabel_build_id', 'igw_relabel_last_error', 'igw_relabel'} == set(R.EXPORTS)
    for name in _declared():
        assert hasattr(L, name)
    assert L.igw_relabel_version() == R.VERSION == 1
    assert R.build_id() == R.source_hash() == R.built_id()
    assert not R.is_stale()
    syms = subprocess.check_output([os.path.join(LLVM, 'llvm-readelf'), '--dyn-syms', '-W', lib], text=True)
    exported = [ln.split()[-1] for ln in syms.splitlines() if ' GLOBAL ' in ln and ' UND ' not in ln]
    assert sorted(s for s in exported if s.startswith('igw_')) == _declared()   # exactly the declared symbols


def test_relabel_sources_are_in_no_other_library():
    """The relabel library's files enter no other library's build id, it is built with the step library's flags, and the
    package-level build knows it."""
    from gridworld_amd import aim as A, build as B, codec as K, goal as G, peek as P, peek_dict as PD, query as Q, \
        relabel as R, render as RD, vox as X, worth as W
    srcs = [os.path.basename(s) for s in B.SOURCES + B.HEADERS + RD.SOURCES + RD.HEADERS + RD.OBS_SOURCES + RD.OBS_HEADERS +
            Q.SOURCES + Q.HEADERS + K.LIBRARY.sources + K.LIBRARY.headers]
    for m in (G, A, P, PD, X, W):
        srcs += [os.path.basename(s) for s in m.LIBRARY.sources + m.LIBRARY.headers]
    assert 'igw_relabel.hip' not in srcs and 'igw_relabel.h' not in srcs
    assert R.LIBRARY.flags == () and os.path.basename(R.LIB) == 'libigw_relabel.so'
    markers = [m.LIBRARY.marker for m in (G, A, P, PD, X, W, Q)]
    assert R.LIBRARY.marker == b'igw-relabel-build-id:' and R.LIBRARY.marker not in markers
    assert 'relabel' in open(os.path.join(ROOT, 'gridworld_amd', 'build.py')).read().split("if __name__ == '__main__':")[1]
    assert 'hip_relabel.build(force=True)' in open(os.path.join(ROOT, '__graft_entry__.py')).read()


def test_relabel_code_object_has_no_scratch_and_no_spills(tmp_path):
    """The notes of the gfx950 code object inside the library, read as tests/test_worth_cpu.py reads the worth's."""
    from gridworld_amd import relabel as R
    fat, co = str(tmp_path / 'fat.bin'), str(tmp_path / 'dev.co')
    subprocess.check_call([os.path.join(LLVM, 'llvm-objcopy'), '--dump-section', '.hip_fatbin=' + fat, R.build()])
    subprocess.check_call([os.path.join(LLVM, 'clang-offload-bundler'), '--type=o',
                           '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--input=' + fat, '--output=' + co, '--unbundle'])
    notes = subprocess.check_output([os.path.join(LLVM, 'llvm-readelf'), '--notes', co], text=True)
    kern = [b for b in notes.split('- .agpr_count:')[1:] if 'igw_relabel_kernel' in b]
    assert len(kern) == 1
    val = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, kern[0]).group(1))  # noqa: E731
    print('igw_relabel_kernel: %d VGPRs, %d SGPRs, %d B of LDS' % (val('vgpr_count'), val('sgpr_count'),
                                                                   val('group_segment_fixed_size')))
    assert val('private_segment_fixed_size') == 0
    assert val('vgpr_spill_count') == 0 and val('sgpr_spill_count') == 0
    assert re.search(r'\.uses_dynamic_stack:\s+false', kern[0])
    assert val('vgpr_count') <= 64                          # eight wavefronts per SIMD as far as registers go
    assert val('group_segment_fixed_size') <= 32 * 1024     # five blocks per CU (160 KiB of LDS)
    assert re.search(r'\.max_flat_workgroup_size:\s+256', kern[0])


def test_relabel_rejects_bad_arguments_without_a_device():
    from gridworld_amd import relabel as R
    L = R.load()
    buf = (ctypes.c_uint8 * 32768)()
    p16 = (ctypes.addressof(buf) + 15) & ~15
    ins = ('records', 'first', 'length', 'start_grid', 'targets', 'at')
    outs = ('reward', 'done', 'progress', 'end', 'ret', 'target_size', 'target')
    ok = dict({k: p16 for k in ins + outs}, at=None, n_records=4, E=1, G=1, L=4, max_steps=250, gamma=1.0)

    def call(**kw):
        a = dict(ok, **kw)
        return L.igw_relabel(a['records'], a['n_records'], a['first'], a['length'], a['start_grid'], a['targets'], a['at'],
                             a['E'], a['G'], a['L'], 1.0, 0.1, a['max_steps'], a['gamma'], *[a[k] for k in outs], None)
    bad = [{k: None} for k in ('records', 'first', 'length', 'start_grid')] + \
        [dict(targets=None, at=None), dict(targets=p16, at=p16), dict({k: None for k in outs}),
         dict(start_grid=p16 + 8), dict(targets=p16 + 8), dict(target=p16 + 8), dict(first=p16 + 4), dict(records=p16 + 2),
         dict(length=p16 + 2), dict(targets=None, at=p16 + 2), dict(reward=p16 + 2), dict(end=p16 + 2), dict(ret=p16 + 2),
         dict(progress=p16 + 1), dict(target_size=p16 + 1),
         dict(E=-1), dict(n_records=-1), dict(G=0), dict(G=257), dict(L=0), dict(L=-3), dict(E=1 << 20, G=256, L=1 << 12),
         dict(max_steps=0), dict(max_steps=65535), dict(gamma=math.inf), dict(gamma=-math.inf), dict(gamma=math.nan)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert L.igw_relabel_last_error().startswith(b'igw_relabel: ')
    # E == 0 launches nothing, whatever the rest (still checked)
    assert call(E=0) == 0 and call(E=0, targets=None, at=p16) == 0 and call(E=0, done=p16 + 1, reward=None) == 0
    assert call(E=0, G=257) == -1 and call(E=0, **{k: None for k in outs}) == -1


def test_relabel_host_side_checks_and_future_entries():
    import torch
    import gridworld_amd as G
    from gridworld_amd import relabel as R
    assert G.relabel is R and callable(G.relabel) and G.relabel_future is R.relabel_future
    assert R.OUTPUTS == ('reward', 'done', 'progress', 'end', 'ret', 'target_size', 'target')
    assert R.check_outputs(('ret', 'reward')) == ('reward', 'ret') and R.check_outputs('end') == ('end',)
    for names in ((), ('rewards',), ('reward', 'word')):
        with pytest.raises(ValueError):
            R.check_outputs(names)
    cpu = torch.device('cpu')
    rec = torch.zeros((2, 2, 8, 64), dtype=torch.uint8)
    first, length = torch.tensor([0, 16]), torch.tensor([8, 8], dtype=torch.int32)
    starts = torch.zeros((2, 1104), dtype=torch.int8)
    at = torch.zeros((2, 3), dtype=torch.int32)
    tg = torch.zeros((2, 3, 1104), dtype=torch.int8)
    with pytest.raises(ValueError, match='device tensor'):
        G.relabel(rec, first, length, starts, at=at)       # the stateless form takes a device log
    ok = dict(records=rec, first=first, length=length, starts=starts, targets=None, at=at, pad=8,
              reward=(1.0, 0.1, 250), gamma=1.0, names=('reward',), out=None, dev=cpu, stream=None)
    bad = [dict(targets=tg), dict(at=None), dict(at=at.long()), dict(at=at[:1]), dict(at=torch.zeros((2, 0), dtype=torch.int32)),
           dict(at=torch.zeros((2, 257), dtype=torch.int32)), dict(at=None, targets=tg[:, :, :1089]),
           dict(at=None, targets=tg.to(torch.int32)), dict(records=rec[..., :32]), dict(records=rec.to(torch.int8)),
           dict(first=first.to(torch.int32)), dict(length=length.long()), dict(starts=starts[:, :1089]), dict(pad=0),
           dict(pad=1 << 40), dict(reward=(1.0, 0.1, 0)), dict(reward=(1.0, 0.1, 65535)), dict(gamma=float('nan')),
           dict(gamma=float('inf')), dict(names=()), dict(names=('nope',)), dict(out={'done': torch.zeros((2, 3, 8), dtype=torch.uint8)}),
           dict(out={'reward': torch.zeros((2, 3, 9))}), dict(out={'reward': torch.zeros((2, 3, 8), dtype=torch.float64)})]
    for kw in bad:
        with pytest.raises(ValueError):
            R.launch(**dict(ok, **kw))
    with pytest.raises(ValueError):
        R.grid_rows(np.zeros((2, 3, 1088), np.int8), cpu, (2, 3))
    assert tuple(R.grid_rows(np.ones((2, 3, 9, 11, 11), np.int64), cpu, (2, 3)).shape) == (2, 3, 1104)
    # HER's "future" entries: 1..length, 0 for an empty episode, the same for the same seed
    length = torch.tensor([0, 1, 2, 48, 250, 7], dtype=torch.int32)
    f = G.relabel_future(length, 64, seed=5)
    assert f.dtype == torch.int32 and tuple(f.shape) == (6, 64)
    assert (f[0] == 0).all() and (f[1:] >= 1).all() and (f <= length[:, None]).all()
    assert len(set(f[4].tolist())) > 32 and set(f[2].tolist()) == {1, 2}
    assert torch.equal(f, G.relabel_future(length, 64, seed=5)) and not torch.equal(f, G.relabel_future(length, 64, seed=6))
    for kw in (dict(length=length.float(), k=2), dict(length=length, k=0), dict(length=length[None], k=2)):
        with pytest.raises(ValueError):
            G.relabel_future(**kw)


def _model(name, max_steps=None):
    """The model's answers for the named case under every goal, from the base run's change words alone."""
    b, goals = RC.base(name), RC.goal_grids(name)
    ms = RC.cases()[name]['kw']['max_steps'] if max_steps is None else max_steps
    return [[RM.episode(b['starts'][i], b['change'][i], goals[i, g], RC.RIGHT, RC.WRONG, ms) for g in range(len(RC.GOALS))]
            for i in range(RC.E)]


@pytest.mark.parametrize('max_steps', [None, 20])
def test_the_model_equals_the_stepped_oracle(max_steps):
    """Reward (as a bit pattern), done and the cached max_int of every step, every case, env and goal."""
    for name in RC.cases():
        t, m = RC.truth(name, max_steps), _model(name, max_steps)
        for i in range(RC.E):
            for g, goal in enumerate(RC.GOALS):
                r, where = m[i][g], (name, i, goal, max_steps)
                assert np.array_equal(r['reward'].view(np.uint32), t['reward'][i, g].view(np.uint32)), where
                assert np.array_equal(r['done'], t['done'][i, g]), where
                assert np.array_equal(r['progress'], t['progress'][i, g]), where
                assert r['end'] == RC.end_of(t['done'][i, g]), where
        if max_steps == 20:
            assert (t['done'][:, :, 19] == 1).all()


def test_the_grid_sequence_does_not_depend_on_the_target():
    """What lets the log's change words stand for the episode under any target: the oracle builds the same grids,
    step for step, whatever it is paid for."""
    for name in RC.cases():
        b, t = RC.base(name), RC.truth(name)
        for g, goal in enumerate(RC.GOALS):
            assert np.array_equal(t['grids'][g], b['grids']), (name, goal)
        own = RC.GOALS.index('own')                            # ... and the base run is the `own` run
        assert np.array_equal(t['reward'][:, own].view(np.uint32), b['reward'].view(np.uint32))
        assert np.array_equal(t['done'][:, own], b['done'])
        # the words rebuild the grids
        for i in (0, 7, 31):
            assert np.array_equal(RM.grids_of(b['starts'][i], b['change'][i]), b['grids'][:, i])


def test_the_cases_cover_what_the_gpu_comparison_has_to_tell_apart():
    """Coverage floors on the oracle's truth alone, over all cases and goals (conditions; counts are printed)."""
    got = dict.fromkeys(('steps with reward > 0', 'steps with reward < 0', 'pairs that end before the last step',
                         'pairs never done', 'steps where done falls from 1 to 0', 'logged steps that recolour a cell in place',
                         'steps whose relabelled reward differs from the logged one'), 0)
    for name in RC.cases():
        b, t = RC.base(name), RC.truth(name)
        end = RC.end_of(t['done'])
        got['steps with reward > 0'] += int((t['reward'] > 0).sum())
        got['steps with reward < 0'] += int((t['reward'] < 0).sum())
        got['pairs that end before the last step'] += int(((end > 0) & (end < RC.T)).sum())
        got['pairs never done'] += int((end == 0).sum())
        got['steps where done falls from 1 to 0'] += int(((t['done'][..., :-1] == 1) & (t['done'][..., 1:] == 0)).sum())
        g = b['grids'].astype(np.int16)
        changed = (g[1:] != g[:-1]).any(2)                                     # [T, E]
        s = g - b['starts'][None].astype(np.int16)
        same_size = np.count_nonzero(s[1:], axis=2) == np.count_nonzero(s[:-1], axis=2)
        got['logged steps that recolour a cell in place'] += int((changed & same_size).sum())
        got['steps whose relabelled reward differs from the logged one'] += \
            int((t['reward'].view(np.uint32) != b['reward'].view(np.uint32)[:, None]).sum())
    for k, v in got.items():
        print('%-65s %d' % (k, v))
    for k, v in got.items():
        assert v >= 20, (k, v)
    # a step paid from a stale cache (right != 0 counted from a max_int that a recolouring in place had left behind the
    # live maximum).  `recolour` recolours 32 cells but its logged actions change no block count afterwards, so under
    # its own target nothing is paid from the stale value; `towers` under final, at24 and rolled is what reaches it.
    stale = {name: sum(r[g]['stale_paid'] for r in _model(name) for g in range(len(RC.GOALS))) for name in RC.cases()}
    print('%-65s %s' % ('steps paid from a stale cache', {k: v for k, v in stale.items() if v}))
    assert sum(stale.values()) >= 1
