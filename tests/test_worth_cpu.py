"""CPU side of the worth query: libigw_worth.so as a cross-compiled artefact -- its exports, its
code object, its argument checks --, worth_decode, and the numpy model the GPU test compares against
(tests/worth_model.py on tests/worth_cases.py), pinned to the CPU oracle twice and counted for coverage.  The GPU
comparison is tests/test_gpu_worth.py."""
import ctypes
import os
import re
import subprocess

import numpy as np

import goal_cases as GC
import worth_cases as WC
import worth_model as WM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = '/opt/rocm/lib/llvm/bin'


def _declared():
    src = open(os.path.join(ROOT, 'include', 'igw_worth.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(igw_[a-z0-9_]+)\s*\(', src)))


def test_worth_library_cross_compiles_and_exports_its_declared_symbols():
    from gridworld_amd import worth as W
    lib = W.build()
    assert os.path.exists(lib) and os.path.basename(lib) == 'libigw_worth.so'
    L = W.load()
    assert sorted(W.EXPORTS) == _declared()
    assert {'igw_worth_version', 'igw_worth_build_id', 'igw_worth_last_error', 'igw_worth'} == set(W.EXPORTS)
    for name in _declared():
        assert hasattr(L, name)
    assert L.igw_worth_version() == W.VERSION == 1
    assert W.build_id() == W.source_hash() == W.built_id()
    assert not W.is_stale()
    syms = subprocess.check_output([os.path.join(LLVM, 'llvm-readelf'), '--dyn-syms', '-W', lib], text=True)
    exported = [ln.split()[-1] for ln in syms.splitlines() if ' GLOBAL ' in ln and ' UND ' not in ln]
    assert sorted(s for s in exported if s.startswith('igw_')) == _declared()   # exactly the declared symbols


def test_worth_sources_are_in_no_other_library():
    """The worth library's files enter no other library's build id, and it is built with the step library's flags."""
    from gridworld_amd import aim as A, build as B, codec as K, goal as G, peek as P, peek_dict as PD, query as Q, \
        render as R, vox as X, worth as W
    srcs = [os.path.basename(s) for s in B.SOURCES + B.HEADERS + R.SOURCES + R.HEADERS + R.OBS_SOURCES + R.OBS_HEADERS +
            Q.SOURCES + Q.HEADERS + K.LIBRARY.sources + K.LIBRARY.headers]
    for m in (G, A, P, PD, X):
        srcs += [os.path.basename(s) for s in m.LIBRARY.sources + m.LIBRARY.headers]
    assert 'igw_worth.hip' not in srcs and 'igw_worth.h' not in srcs
    assert W.LIBRARY.flags == () and os.path.basename(W.LIB) == 'libigw_worth.so'
    markers = [m.LIBRARY.marker for m in (G, A, P, PD, X, Q)]
    assert W.LIBRARY.marker == b'igw-worth-build-id:' and W.LIBRARY.marker not in markers


def test_worth_code_object_has_no_scratch_and_no_spills(tmp_path):
    """The notes of the gfx950 code object inside the library, read as tests/test_goal_cpu.py reads the goal's."""
    from gridworld_amd import worth as W
    fat, co = str(tmp_path / 'fat.bin'), str(tmp_path / 'dev.co')
    subprocess.check_call([os.path.join(LLVM, 'llvm-objcopy'), '--dump-section', '.hip_fatbin=' + fat, W.build()])
    subprocess.check_call([os.path.join(LLVM, 'clang-offload-bundler'), '--type=o',
                           '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--input=' + fat, '--output=' + co, '--unbundle'])
    notes = subprocess.check_output([os.path.join(LLVM, 'llvm-readelf'), '--notes', co], text=True)
    kern = [b for b in notes.split('- .agpr_count:')[1:] if 'igw_worth_kernel' in b]
    assert len(kern) == 1
    val = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, kern[0]).group(1))  # noqa: E731
    print('igw_worth_kernel: %d VGPRs, %d SGPRs, %d B of LDS' % (val('vgpr_count'), val('sgpr_count'),
                                                                 val('group_segment_fixed_size')))
    assert val('private_segment_fixed_size') == 0
    assert val('vgpr_spill_count') == 0 and val('sgpr_spill_count') == 0
    assert re.search(r'\.uses_dynamic_stack:\s+false', kern[0])
    assert val('vgpr_count') <= 128
    assert val('group_segment_fixed_size') <= 32 * 1024   # five blocks per CU (160 KiB of LDS)
    assert re.search(r'\.max_flat_workgroup_size:\s+256', kern[0])


def test_worth_rejects_bad_arguments_without_a_device():
    from gridworld_amd import worth as W
    L = W.load()
    buf = (ctypes.c_uint8 * 32768)()
    p16 = (ctypes.addressof(buf) + 15) & ~15
    state = ('grid', 'hist', 'aux', 'agent', 'task_target', 'task_start', 'task_meta', 'task_index')
    ok = dict({k: p16 for k in state + ('allow', 'word', 'best')}, n=1, max_steps=250)

    def call(**kw):
        a = dict(ok, **kw)
        return L.igw_worth(*[a[k] for k in state], a['n'], a['max_steps'], a['allow'], 0, 1.0, 0.1, a['word'],
                           a['best'], None)
    bad = [{k: None} for k in state] + [{k: p16 + 8} for k in state] + \
        [dict(n=-1), dict(allow=p16 + 1), dict(allow=p16 + 8), dict(word=p16 + 2), dict(word=p16 + 8), dict(best=p16 + 4), dict(best=p16 + 8),
         dict(word=None, best=None), dict(n=0, word=None, best=None), dict(max_steps=0), dict(max_steps=65535)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert L.igw_worth_last_error().startswith(b'igw_worth: ')
    assert call(n=0) == 0 and call(n=0, word=None) == 0 and call(n=0, best=None, allow=None) == 0   # nothing is launched


def test_worth_decode_round_trips():
    import torch
    import gridworld_amd as G
    from gridworld_amd import worth as W
    assert G.worth_plane_names == ('break', 'place1', 'place2', 'place3', 'place4', 'place5', 'place6')
    right = np.array([0, 1, -1, 1089, -1089, 5, -7, 0, 0, 2047, -2048], np.int32)
    wrong = np.array([0, 1, -1, 1, -1, 0, 0, 1, -1, 0, 0], np.int32)
    ends = np.array([0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 1], bool)
    w = W.worth_encode(right, wrong, ends)
    assert w.dtype == np.int16 and (w >= 0).all() and np.array_equal(w, WM.encode(right, wrong, ends))
    word = np.concatenate([w, np.array([-1], np.int16)])
    for d in (G.worth_decode(word), {k: v.numpy() for k, v in G.worth_decode(torch.from_numpy(word)).items()}):
        assert d['right'].dtype == np.int16 and d['wrong'].dtype == np.int8 and d['gain'].dtype == np.float32
        assert d['ends'].dtype == np.bool_ and d['valid'].dtype == np.bool_
        assert np.array_equal(d['right'][:-1], right) and np.array_equal(d['wrong'][:-1], wrong)
        assert np.array_equal(d['ends'][:-1], ends) and d['valid'][:-1].all()
        assert not d['valid'][-1] and d['right'][-1] == 0 and d['wrong'][-1] == 0 and not d['ends'][-1]
        assert np.isnan(d['gain'][-1]) and not np.isnan(d['gain'][:-1]).any()
        want = np.where(right != 0, right * np.float64(1), wrong * np.float64(0.1)).astype(np.float32)
        assert np.array_equal(d['gain'][:-1].view(np.uint32), want.view(np.uint32))
    d = G.worth_decode(word, right_scale=0.3, wrong_scale=-0.7)
    want = np.where(right != 0, right * np.float64(0.3), wrong * np.float64(-0.7)).astype(np.float32)
    assert np.array_equal(d['gain'][:-1].view(np.uint32), want.view(np.uint32))
    mr, mw, me, mv = WM.decode(word)
    assert np.array_equal(mr, d['right']) and np.array_equal(mw, d['wrong']) and np.array_equal(me, d['ends'])
    assert np.array_equal(mv, d['valid'])


def test_the_model_pays_what_the_stepped_oracle_pays():
    """For every probe step of the oracle that changed the grid, the model's word at (that plane, that cell) decodes to
    the step's reward, as a bit pattern, and to its `done`: this carries the stale cache."""
    import gridworld_amd as G
    n = stale = 0
    for name in WC.cases():
        st, words = WC.states(name), WC.words(name)
        if name in GC.cases():   # the probes are the goal truth's
            t = GC.truth(name)
            cols = list(WC.PROBES)
            assert np.array_equal(t['gain'][..., cols].view(np.uint32), st['gain'].view(np.uint32))
            assert np.array_equal(t['changed'], st['cell'] >= 0)
        C, E, _ = st['cell'].shape
        for c in range(C):
            for i in range(E):
                for j in range(8):
                    cell, plane = int(st['cell'][c, i, j]), int(st['plane'][c, i, j])
                    if cell < 0:
                        continue
                    d = G.worth_decode(words[c, i, plane, cell:cell + 1], WC.RIGHT, WC.WRONG)
                    assert d['valid'][0], (name, c, i, j)
                    assert d['gain'].view(np.uint32)[0] == st['gain'][c, i, j:j + 1].view(np.uint32)[0], (name, c, i, j)
                    assert bool(d['ends'][0]) == bool(st['ends'][c, i, j]), (name, c, i, j)
                    n += 1
                    stale += int(WC.model(name)[c][i]['M'] != st['cached'][c, i])
    print(f'{n} probe steps changed the grid; {stale} of them on a stale cache')
    # the floors of tests/test_goal_cpu.py on the same probes: 100 each of +right, -right, +wrong, -wrong; 20 stale
    assert n >= 400 and stale >= 20


def _edited_max_int(case, name, c, i, plane, cell):
    from oracle import oracle as O
    start = WC.starts_of(case)[i].astype(np.int8)
    t = case['targets'][i].astype(np.int8) - start
    g = WC.states(name)['grid'][c, i].copy()
    g.reshape(-1)[cell] = plane
    return O.task_eval(t, g - start)['max_int']


def test_the_model_recounts_what_the_stateless_oracle_counts():
    """m' of the model equals oracle.task_eval(T, S edited)['max_int'] for every recounting edit of the rare kinds --
    every removing edit, every break that adds votes, every completion, every right < 0 -- and for a seeded random
    1,000 of the other recounting edits per case."""
    rng = np.random.RandomState(2024)
    for name, case in WC.cases().items():
        rare, rest = [], []
        for c, row in enumerate(WC.model(name)):
            for i, m in enumerate(row):
                recount = m['adds'] | m['removes']
                right = WM.decode(m['word'][:, :WM.CELLS])[0].reshape(7, 9, 11, 11)
                is_rare = recount & (m['removes'] | (m['adds'] & (np.arange(7) == 0)[:, None, None, None])
                                     | (m['mprime'] == m['target_size']) | (right < 0))
                for p, cell in zip(*np.nonzero(is_rare.reshape(7, -1))):
                    rare.append((c, i, p, cell))
                for p, cell in zip(*np.nonzero((recount & ~is_rare).reshape(7, -1))):
                    rest.append((c, i, p, cell))
        pick = [rest[k] for k in rng.choice(len(rest), 1000, replace=False)]
        for c, i, p, cell in rare + pick:
            want = _edited_max_int(case, name, c, i, int(p), int(cell))
            got = WC.model(name)[c][i]['mprime'].reshape(7, -1)[p, cell]
            assert got == want, (name, c, i, p, cell, got, want)
        print(f'{name}: {len(rare)} rare edits and 1,000 of {len(rest)} others recounted by the oracle')


def test_the_model_covers_what_the_gpu_comparison_has_to_tell_apart():
    """Coverage floors on the model's counts over all cases, envs and checkpoints (conditions; counts are printed)."""
    got = dict.fromkeys(('right > 0', 'right < 0', 'wrong == 0', 'ends by completion', 'a break that lowers the maximum',
                         'a break that touches a maximal bin while another keeps the maximum',
                         'an adding edit that touches bins without raising the maximum', 'a break that adds votes',
                         'a place that removes votes', 'a place that removes votes, right < 0',
                         'env-checkpoints whose cache is stale'), 0)
    for name in WC.cases():
        st = WC.states(name)
        for c, row in enumerate(WC.model(name)):
            for i, m in enumerate(row):
                right, wrong, _, valid = (a[:, :WM.CELLS].reshape(7, 9, 11, 11) for a in WM.decode(m['word']))
                mp, M = m['mprime'], m['M']
                got['right > 0'] += int((right > 0).sum())
                got['right < 0'] += int((right < 0).sum())
                got['wrong == 0'] += int((valid & (wrong == 0)).sum())
                got['ends by completion'] += int((valid & (mp == m['target_size'])).sum())
                got['a break that lowers the maximum'] += int((m['removes'][0] & (mp[0] < M)).sum())
                got['a break that touches a maximal bin while another keeps the maximum'] += \
                    int((m['removes'][0] & m['touched_max'][0] & (mp[0] == M)).sum())
                got['an adding edit that touches bins without raising the maximum'] += \
                    int((m['adds'] & m['touched'] & (mp == M)).sum())
                got['a break that adds votes'] += int(m['adds'][0].sum())
                got['a place that removes votes'] += int(m['removes'][1:].sum())
                got['a place that removes votes, right < 0'] += int((m['removes'][1:] & (right[1:] < 0)).sum())
                got['env-checkpoints whose cache is stale'] += int(M != st['cached'][c, i])
    for k, v in got.items():
        print('%-75s %d' % (k, v))
    for k, v in got.items():
        assert v >= 20, (k, v)
    # `unbuild` does what it says: once env 0 has broken its extra block (checkpoint 25) putting colour 1 back takes
    # the vote away and breaking the other extra block adds one
    m = WC.model('unbuild')[4][0]
    right = WM.decode(m['word'][:, :WM.CELLS])[0].reshape(7, 9, 11, 11)
    assert m['M'] == 1 and right[1, 0, 5, 4] == -1 and m['removes'][1, 0, 5, 4]
    assert right[0, 0, 5, 3] == 1 and m['adds'][0, 0, 5, 3]
