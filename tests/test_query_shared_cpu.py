"""The code the query libraries share (csrc/igw_vote.h: the histogram vote; csrc/peek/igw_peek_core.h and igw_peek_body.h:
the peek kernel):
each shared function is defined once outside the step library, and every library that includes a shared header lists it
among its HEADERS, so that its build id and its staleness see the header.  No device."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'gridworld_amd', 'csrc')
STEP_ONLY = ('igw_kernels.hip', 'igw_device.h')      # the step library restates what it needs: nothing moves out of it
SHARED = {'igw_vote.h': os.path.join(CSRC, 'igw_vote.h'), 'igw_peek_core.h': os.path.join(CSRC, 'peek', 'igw_peek_core.h'),
          'igw_peek_body.h': os.path.join(CSRC, 'peek', 'igw_peek_body.h')}
ONCE = ('class1', 'row_piece_max', 'vote_change', 'wave_sum_i32', 'world_act_pre', 'world_act_post', 'finish_break',
        'world_update', 'syn_size_delta', 'finish_step')


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
                     'peek': set(SHARED), 'peek_dict': set(SHARED)}
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
