"""The code the query libraries share (csrc/igw_vote.h: the histogram vote; csrc/peek/igw_peek_core.h and igw_peek_body.h:
the peek kernel; csrc/igw_voxel.h, igw_voxel_table.h and igw_voxel_stage.h: the back end of the two voxel writers):
each shared function is defined once outside the step library, and every library that includes a shared header lists it
among its HEADERS, so that its build id and its staleness see the header.  No device."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'gridworld_amd', 'csrc')
STEP_ONLY = ('igw_kernels.hip', 'igw_device.h')      # the step library restates what it needs: nothing moves out of it
SHARED = {'igw_vote.h': os.path.join(CSRC, 'igw_vote.h'), 'igw_peek_core.h': os.path.join(CSRC, 'peek', 'igw_peek_core.h'),
          'igw_peek_body.h': os.path.join(CSRC, 'peek', 'igw_peek_body.h'), 'igw_voxel.h': os.path.join(CSRC, 'igw_voxel.h'),
          'igw_voxel_table.h': os.path.join(CSRC, 'igw_voxel_table.h'),
          'igw_voxel_stage.h': os.path.join(CSRC, 'igw_voxel_stage.h')}
VOXEL = {'igw_voxel.h', 'igw_voxel_table.h', 'igw_voxel_stage.h'}
PEEK = {'igw_vote.h', 'igw_peek_core.h', 'igw_peek_body.h'}
ONCE = ('class1', 'row_piece_max', 'vote_change', 'wave_sum_i32', 'world_act_pre', 'world_act_post', 'finish_break',
        'world_update', 'syn_size_delta', 'finish_step', 'elem_value', 'store16', 'pose_cell', 'write_slot')


def _code(path):
    """The file without its comments."""
    return re.sub(r'//[^\n]*|/\*.*?\*/', '', open(path).read(), flags=re.S)


def _libraries():
    from gridworld_amd import aim, build, codec, goal, peek, peek_dict, query, recall, relabel, render, vox, worth
    libs = {m.__name__.rsplit('.', 1)[1]: m.LIBRARY for m in (aim, codec, goal, peek, peek_dict, query, recall, relabel, render, vox, worth)}
    libs.update(render_obs=render.OBS_LIBRARY, step=build.STEP)
    return libs


def _included(path, seen=None):
    """Real paths of the files under csrc that `path` includes with quotes, directly or through them."""
    seen = set() if seen is None else seen
    for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', _code(path), flags=re.M):
        f = os.path.realpath(os.path.join(os.path.dirname(path), inc))
        if f.startswith(os.path.realpath(CSRC) + os.sep) and f not in seen:
            seen.add(f)
            _included(f, seen)
    return seen


def test_every_shared_function_is_defined_once_outside_the_step_library():
    files = [os.path.join(d, f) for d, _, fs in os.walk(CSRC) for f in fs if f not in STEP_ONLY]
    assert {os.path.basename(f) for f in SHARED.values()} <= {os.path.basename(f) for f in files}
    for name in ONCE:
        head = re.compile(r'\b%s\s*\([^;{]*\)\s*\{' % name)   # the function's head and the brace that opens its body
        where = [os.path.relpath(f, CSRC) for f in files for _ in head.findall(_code(f))]
        assert len(where) == 1 and os.path.basename(where[0]) in SHARED, (name, where)
    # ... and the step library keeps its own: the shared headers are no part of it
    from gridworld_amd import build as B
    assert not set(SHARED) & {os.path.basename(f) for f in B.SOURCES + B.HEADERS}
    assert not set(SHARED) & {os.path.basename(f) for f in _included(os.path.join(CSRC, 'igw_kernels.hip'))}


def test_the_voxel_channel_table_and_staging_loop_are_shared_text():
    """The channel table and the staging loop of vox and recall are statements in two files that both kernels include in
    their bodies: each file is included once by each kernel, and what marks the table (the six channels of a one-hot
    plane) and the loop (the ahead / right mapping of the agent's frame, the 0 / 1..6 / kOther classification, the agent's
    body) stands in those files and nowhere else under csrc."""
    files = [os.path.join(d, f) for d, _, fs in os.walk(CSRC) for f in fs]
    marks = {'igw_voxel_table.h': (r'tid\s*-\s*first\s*\+\s*1', r'match\s*=', r'ch_plane\s*\[\s*tid\s*\]\s*='),
             'igw_voxel_stage.h': (r'fr\.hx\s*\+\s*\w+\s*\*\s*fr\.fx', r'kOther\s*:\s*0', r'y\s*==\s*fr\.hy\s*-\s*1',
                                   r'\*\s*121\s*\+\s*x\s*\*\s*11\s*\+\s*z')}
    for name, pats in marks.items():
        for kernel in (os.path.join(CSRC, 'vox', 'igw_vox.hip'), os.path.join(CSRC, 'recall', 'igw_recall.hip')):
            included = re.findall(r'#include "\.\./(igw_voxel_(?:table|stage)\.h)"', _code(kernel))
            assert included.count(name) == 1, (kernel, name)
        for pat in pats:
            where = [os.path.basename(f) for f in files if re.search(pat, _code(f))]
            assert where == [name], (pat, where)


def _users():
    """library name -> the shared headers its sources include."""
    users = {}
    for name, lib in _libraries().items():
        inc = set().union(*[_included(lib.path(s)) for s in lib.sources])
        mine = {k for k, f in SHARED.items() if os.path.realpath(f) in inc}
        if mine:
            users[name] = mine
    return users


def test_a_library_lists_the_shared_headers_it_includes():
    users, libs = _users(), _libraries()
    assert users == {'goal': {'igw_vote.h'}, 'worth': {'igw_vote.h'}, 'relabel': {'igw_vote.h'},
                     'peek': PEEK, 'peek_dict': PEEK, 'vox': VOXEL, 'recall': VOXEL}
    for name, mine in users.items():
        listed = {os.path.realpath(libs[name].path(h)) for h in libs[name].headers}
        for k in mine:
            assert os.path.realpath(SHARED[k]) in listed, (name, k)
        # the build id keys files by base name: a shared header's is unique among the library's files
        names = [os.path.basename(f) for f in libs[name].sources + libs[name].headers]
        assert len(names) == len(set(names)), name


def test_a_touched_shared_header_makes_its_libraries_stale():
    libs = _libraries()
    for name, mine in _users().items():
        lib = libs[name]
        lib.build()
        assert not lib.is_stale(), name
        for k in sorted(mine):
            st = os.stat(SHARED[k])
            later = max(os.stat(lib.lib).st_mtime_ns, st.st_mtime_ns) + 10 ** 10
            try:
                os.utime(SHARED[k], ns=(st.st_atime_ns, later))
                assert lib.is_stale(), (name, k)
            finally:
                os.utime(SHARED[k], ns=(st.st_atime_ns, st.st_mtime_ns))
        assert not lib.is_stale(), name
        assert lib.built_id() == lib.source_hash()


QUERIES = ('query', 'goal', 'aim', 'peek', 'peek_dict', 'vox', 'worth', 'relabel', 'recall')


def test_every_query_module_describes_its_library_through_the_one_constructor():
    """What build.query fills in for the nine modules: the three symbols every library has, in front of the module's own
    entries; the library's names from the module's; and a staleness that sees the describing module and build.py."""
    import ctypes
    import importlib
    from gridworld_amd import build as B
    for name in QUERIES:
        m = importlib.import_module('gridworld_amd.' + name)
        sym = 'igw_' + name
        assert {os.path.realpath(d) for d in m.LIBRARY.deps} == {os.path.realpath(m.__file__), os.path.realpath(B.__file__)}
        assert list(m.SIGNATURES)[:3] == [sym + '_version', sym + '_build_id', sym + '_last_error'] and len(m.SIGNATURES) > 3
        assert [m.SIGNATURES[k] for k in list(m.SIGNATURES)[:3]] == [(ctypes.c_int, []), (ctypes.c_char_p, []),
                                                                     (ctypes.c_char_p, [])]
        assert m.EXPORTS == list(m.SIGNATURES) and m.SIGNATURES is m.BINDING.signatures
        assert m.BINDING.library is m.LIBRARY and m.BINDING.module == 'gridworld_amd.' + name
        assert issubclass(m.BINDING.error, RuntimeError) and m.BINDING.error.__module__ == m.__name__
        assert m.BINDING.what.startswith('igw_') and m.BINDING.what not in list(m.SIGNATURES)[:3]   # check()'s default entry
        assert m.LIB == m.LIBRARY.lib == os.path.join(os.path.dirname(m.__file__), 'lib%s.so' % sym)
        assert m.SOURCES == m.LIBRARY.sources == [os.path.join(CSRC, name, sym + '.hip')]
        assert m.HEADERS is m.LIBRARY.headers and os.path.basename(m.HEADERS[-1]) == sym + '.h'
        assert m.LIBRARY.marker == ('igw-%s-build-id:' % name.replace('_', '-')).encode()
        assert m.LIBRARY.define == 'IGW_%s_BUILD_ID' % name.upper()
        assert (m.build, m.source_hash, m.built_id, m.is_stale) == (m.LIBRARY.build, m.LIBRARY.source_hash,
                                                                    m.LIBRARY.built_id, m.LIBRARY.is_stale)
        assert (m.load, m.check, m.build_id) == (m.BINDING.load, m.BINDING.check, m.BINDING.build_id)
        device = [os.path.basename(h) for h in B.DEVICE_HEADERS]
        assert device == ['igw_device.h', 'igw_trig.h', 'igw_trig_lut.h', 'igw_trig_tables.h', 'igw.h']
        assert ([h for h in m.HEADERS if h in B.DEVICE_HEADERS] == B.DEVICE_HEADERS) == (name not in ('vox', 'recall'))
        assert all(os.path.exists(f) for f in m.SOURCES + m.HEADERS)


def test_a_newer_describing_module_or_build_py_makes_a_library_stale():
    from gridworld_amd import build as B, query as Q
    Q.build()
    assert not Q.is_stale()
    for f in (Q.__file__, B.__file__):
        st = os.stat(f)
        later = max(os.stat(Q.LIB).st_mtime_ns, st.st_mtime_ns) + 10 ** 10
        try:
            os.utime(f, ns=(st.st_atime_ns, later))
            assert Q.is_stale(), f
        finally:
            os.utime(f, ns=(st.st_atime_ns, st.st_mtime_ns))
    assert not Q.is_stale()
