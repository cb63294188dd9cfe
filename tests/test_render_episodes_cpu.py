"""CPU side of the log frames (igw_render_episodes, include/igw_render.h): the entry point is declared, exported and
bound, checks its arguments like igw_render_pov, reports a missing device, and its kernel passes the code-object
gates of the pov kernel.  The GPU comparisons are tests/test_gpu_render_episodes.py."""
import os
import re
import subprocess

import pytest

from render_checks import LLVM, _buffers, _kernel_gates, _kernel_notes_and_asm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_render_episodes_is_declared_exported_and_bound():
    from gridworld_amd import render as R
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'igw_render.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+igw_render_episodes\s*\(', src)
    assert 'igw_render_episodes' in R.EXPORTS
    L = R.load()
    assert hasattr(L, 'igw_render_episodes') and len(L.igw_render_episodes.argtypes) == 17
    syms = subprocess.check_output([os.path.join(LLVM, 'llvm-readelf'), '--dyn-syms', R.LIB], text=True)
    assert re.search(r'FUNC\s+GLOBAL\s+DEFAULT\s+\d+\s+igw_render_episodes$', syms, flags=re.M)
    assert callable(R.render_episodes_into)
    assert L.igw_render_version() == 1


def test_render_episodes_code_object_gates(tmp_path):
    notes, asm = _kernel_notes_and_asm(tmp_path)
    kern, val, body = _kernel_gates(notes, asm, 'igw_render_episodes_kernel')
    assert 'igw_render_pov_kernel' not in kern                         # the pov kernel's test selects by that name
    # vector stores of the frame, the LDS replay table, the LDS bitmap build it shares with the views kernel
    assert 'global_store' in body and 'ds_max' in body and 'ds_or' in body


def test_render_episodes_rejects_bad_arguments_and_a_missing_device():
    import torch
    from gridworld_amd import render as R
    L = R.load()
    buf, p = _buffers()
    ok = dict(records=p, n_records=16, first=p, length=p, frame0=p, start=p, pose=p, m=2, max_length=5, atlas=p,
              side=128, out=p, n_frames=12, w=64, h=64, c=3)

    def call(**kw):
        a = dict(ok, **kw)
        return L.igw_render_episodes(a['records'], a['n_records'], a['first'], a['length'], a['frame0'], a['start'],
                                     a['pose'], a['m'], a['max_length'], a['atlas'], a['side'], a['out'],
                                     a['n_frames'], a['w'], a['h'], a['c'], None)
    bad = [dict(m=-1), dict(max_length=-1), dict(max_length=(1 << 24) + 1), dict(m=1 << 20, max_length=1 << 12),
           dict(n_records=-1), dict(n_frames=-1), dict(c=2), dict(c=5), dict(w=0), dict(h=0), dict(w=1025),
           dict(h=1025), dict(side=12), dict(side=264), dict(side=0), dict(start=p + 4), dict(records=p + 8),
           dict(first=p + 4), dict(frame0=p + 2), dict(pose=p + 4), dict(length=p + 2), dict(atlas=p + 1)]
    bad += [{k: 0} for k in ('records', 'first', 'length', 'frame0', 'start', 'pose', 'atlas', 'out')]
    for b in bad:
        assert call(**b) == -1, b
        assert L.igw_render_last_error().startswith(b'igw_render_episodes: ')
    # m == 0 reads nothing: null buffers are fine, and the call is a no-op
    nulls = dict(records=0, first=0, length=0, frame0=0, start=0, pose=0, atlas=0, out=0, m=0)
    if torch.cuda.is_available():
        assert call(**nulls) == 0
    else:
        assert call() == -2 and b'no CPU fallback' in L.igw_render_last_error()
        assert call(**nulls) == -2


@pytest.mark.parametrize('max_length', [1, 250])
def test_render_episodes_grid_fits_the_launch_limit(max_length):
    """m * (max_length + 1) blocks along x: the largest accepted product is 2^31 - 1."""
    from gridworld_amd import render as R
    L = R.load()
    buf, p = _buffers()
    m_max = (2 ** 31 - 1) // (max_length + 1)
    args = lambda m: (p, 0, p, p, p, p, p, m, max_length, p, 128, p, 0, 64, 64, 3, None)  # noqa: E731
    assert L.igw_render_episodes(*args(m_max + 1)) == -1
    assert b'2^31' in L.igw_render_last_error()
