"""CPU side of the first-person frame ("First-person frames"): the brute-force model of the contract on
analytic scenes, and the HIP renderer library as a cross-compiled artefact -- its code object, exports, argument
checks and the missing-device error.  The GPU comparison of kernel against model is tests/test_gpu_render.py."""
import glob
import json
import math
import os
import re

import numpy as np
import pytest

import pov_model as M
from render_checks import _buffers, _forbidden, _kernel_gates, _kernel_notes_and_asm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _atlas():
    from gridworld_amd import render as R
    return R.default_atlas()


# ---- the model on analytic scenes -------------------------------------------------------------------------------
def test_horizon_row_and_far_plane_cut_of_the_ground():
    empty = np.zeros((9, 11, 11), np.int8)
    # at the origin, level: the upper half is sky, the ground starts where its hit is inside the 37 x 37 quads
    r = M.render((0, 0, 0, 0, 0), empty, _atlas(), 64, 64)
    assert (r['face'][:32] == -1).all()
    b = 1 - (2 * np.arange(64) + 1) / 64
    first = int(np.argmax(1.5 / np.maximum(-b, 1e-12) <= 18.5))   # the centre column ends at z = -18.5
    assert (r['face'][:first, 32] == -1).all() and (r['face'][first:, 32] == M.GROUND).all()
    # from the corner (10, 10) towards the far corner the ground outruns the far plane: cut at depth 30
    r = M.render((10, 0, 10, -45, 0), empty, _atlas(), 64, 64)
    first = int(np.argmax(1.5 / np.maximum(-b, 1e-12) <= 30))
    assert first == 34
    for j in (31, 32):
        assert (r['face'][:first, j] == -1).all() and (r['face'][first:, j] == M.GROUND).all()
        assert r['t'][first, j] <= 30 and np.isinf(r['t'][first - 1, j])
    # white inside the build zone's footprint (ahead, around |x|, |z| <= 5.5), grey around it (under the eye)
    img = r['image']
    assert (img[63, 32] == (79, 81, 85)).all() and (img[first, 32] == 255).all()


# u / v of each face in the cell's unit coordinates and its sub-tile (column, row) in eighths
TABLE = {'top': (lambda l: l[2], lambda l: l[0], (0, 1)), 'bottom': (lambda l: l[0], lambda l: l[2], (1, 0)),
         'left': (lambda l: l[2], lambda l: l[1], (0, 0)), 'right': (lambda l: 1 - l[2], lambda l: l[1], (0, 0)),
         'front': (lambda l: l[0], lambda l: l[1], (1, 1)), 'back': (lambda l: 1 - l[0], lambda l: l[1], (1, 1))}
# a pose that looks at that face of the block centred at (0, 2, 0) from 1.2 away, and the face's plane
VIEWS = {'top': ((0.1, 3.7, -0.2, 0, -90), 1, 2.5), 'bottom': ((0.1, 0.3, -0.2, 0, 90), 1, 1.5),
         'left': ((-1.7, 2.1, -0.2, 90, 0), 0, -0.5), 'right': ((1.7, 2.1, 0.2, -90, 0), 0, 0.5),
         'front': ((0.1, 2.1, 1.7, 0, 0), 2, 0.5), 'back': ((-0.1, 2.1, -1.7, 180, 0), 2, -0.5)}


@pytest.mark.parametrize('face', list(TABLE))
def test_single_block_face_subtile_and_orientation_through_the_coded_atlas(face):
    atlas = M.coded_atlas(128)
    pose, axis, plane = VIEWS[face]
    W = H = 32
    for colour in range(1, 7):
        g = np.zeros((9, 11, 11), np.int8)
        g[3, 5, 5] = colour                               # world (0, 2, 0)
        r = M.render(pose, g, atlas, W, H)
        dec = M.decode(r['image'])
        d = M.rays(pose[3], pose[4], W, H)
        e = np.array(pose[:3], np.float64)
        t = (plane - e[axis]) / d[..., axis]
        p = e + t[..., None] * d
        loc = p - (np.array([0, 2, 0]) - 0.5)
        on = (loc >= 0).all(-1) & (loc <= 1).all(-1)
        assert on.sum() > 50, face
        uf, vf, (su, sv) = TABLE[face]
        tx, ty = M.TILES[colour]
        col = tx * 32 + su * 16 + np.clip(np.floor(uf(np.moveaxis(loc, -1, 0)) * 16), 0, 15)
        rowb = ty * 32 + sv * 16 + np.clip(np.floor(vf(np.moveaxis(loc, -1, 0)) * 16), 0, 15)
        c = on & M.clean(r)
        assert (r['face'][c] == M.FACE_NAMES.index(face)).all()
        assert (dec[..., 0][c] == col[c]).all() and (dec[..., 1][c] == rowb[c]).all(), (face, colour)
        # the face spans its sub-tile in both directions (a constant u or v would be a wrong orientation)
        assert len(np.unique(dec[c][:, 0])) >= 8 and len(np.unique(dec[c][:, 1])) >= 8


def _gl_rotate(angle, axis):
    """glRotatef's matrix (counter-clockwise by `angle` degrees about the normalised axis)."""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    c, s = math.cos(math.radians(angle)), math.sin(math.radians(angle))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return c * np.eye(3) + (1 - c) * np.outer(a, a) + s * K


def test_centre_ray_is_the_sight_vector_and_the_basis_is_the_gl_modelview():
    rng = np.random.RandomState(0)
    for _ in range(50):
        yaw, pitch = rng.uniform(-360, 360), rng.uniform(-90, 90)
        d = M.rays(yaw, pitch, 65, 65)[32, 32]
        m = math.cos(math.radians(pitch))       # World.get_sight_vector (core/world.py:145-160)
        sight = (math.cos(math.radians(yaw - 90)) * m, math.sin(math.radians(pitch)),
                 math.sin(math.radians(yaw - 90)) * m)
        np.testing.assert_allclose(d, sight, atol=1e-12)
        # render.py:107-110: glRotatef(yaw, 0, 1, 0); glRotatef(-pitch, cos yaw, 0, sin yaw): eye -z / +x / +y
        R = _gl_rotate(yaw, (0, 1, 0)) @ _gl_rotate(-pitch, (math.cos(math.radians(yaw)), 0,
                                                             math.sin(math.radians(yaw))))
        f, r, u = M.basis(yaw, pitch)
        np.testing.assert_allclose(R.T @ [0, 0, -1], f, atol=1e-12)
        np.testing.assert_allclose(R.T @ [1, 0, 0], r, atol=1e-12)
        np.testing.assert_allclose(R.T @ [0, 1, 0], u, atol=1e-12)


def _wall():
    g = np.zeros((9, 11, 11), np.int8)
    g[0:3, :, 4] = 3        # cells z = -1, x = -5..5, y = -1..1: the wall's front face is the plane z = -0.5
    return g


def test_near_plane_see_through_at_a_wall():
    g = _wall()
    W = H = 64
    # 0.25 from the wall the near plane cannot cut it: a frustum point at depth < 0.1 is within 0.1 * sqrt(3)
    for yaw in (60, 80, 100, 120):
        r = M.render((0, 0.5, -0.25, yaw, 0), g, _atlas(), W, H)
        assert not (r['face'] == -1).all()
        d = M.rays(yaw, 0, W, H)
        t = np.where(d[..., 2] < 0, 0.25 / -d[..., 2], np.inf)
        assert (t >= 0.1).all()
    # 0.12 from it at a grazing yaw the left edge of the frame is closer than the near plane: those pixels show the
    # wall's inside, never the clipped front face
    pose = (0.0, 0.5, -0.38, 60, 0)
    r = M.render(pose, g, _atlas(), W, H)
    d = M.rays(60, 0, W, H)
    t = np.where(d[..., 2] < 0, 0.12 / -d[..., 2], np.inf)
    clipped = t < 0.1
    assert clipped.sum() > 100
    assert (r['face'][clipped] != M.FACE_NAMES.index('front')).all()
    assert (r['t'][clipped] >= 0.1).all()
    # behind the clipped face the ray crosses the wall cell and leaves through its back (culled): sky and ground
    assert set(r['face'][clipped].tolist()) <= {-1, M.GROUND, M.FACE_NAMES.index('left')}
    assert M.GROUND in set(r['face'][clipped].tolist())
    assert (r['face'][~clipped & (d[..., 2] < -0.5)] == M.FACE_NAMES.index('front')).any()


def test_default_atlas_and_load_atlas(tmp_path):
    from gridworld_amd import render as R
    a = R.default_atlas()
    assert a.shape == (128, 128, 4) and a.dtype == np.uint8
    ref = np.load(os.path.join(ROOT, 'tests', 'golden', 'texture_atlas.npz'))['atlas']
    # one solid colour per tile: the colour at the centre of the reference's tile
    for tid, (tx, ty) in R.TILES.items():
        r0 = 128 - (ty + 1) * 32
        tile = a[r0:r0 + 32, tx * 32:(tx + 1) * 32]
        assert (tile == tile[0, 0]).all() and tuple(tile[0, 0, :3]) == R.FLAT_COLOURS[tid]
        assert tuple(ref[r0 + 5, tx * 32 + 5, :3]) == R.FLAT_COLOURS[tid]
    p = str(tmp_path / 'atlas.npy')
    np.save(p, ref)
    assert (R.load_atlas(p) == ref).all()
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        png = str(tmp_path / 'atlas.png')
        Image.fromarray(ref).save(png)
        assert (R.load_atlas(png) == ref).all()
    with pytest.raises(ValueError):
        R.check_atlas(np.zeros((12, 12, 4), np.uint8))
    with pytest.raises(ValueError):
        R.check_atlas(np.zeros((16, 16, 3), np.uint8))


# ---- the library ----------------------------------------------------------------------------------------------------
def _declared():
    src = open(os.path.join(ROOT, 'include', 'igw_render.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(igw_render_[a-z0-9_]+)\s*\(', src)))


def test_render_library_exports_its_declared_symbols_and_build_id():
    from gridworld_amd import render as R
    L = R.load()
    assert sorted(R.EXPORTS) == _declared()
    for name in _declared():
        assert hasattr(L, name)
    assert L.igw_render_version() == R.VERSION == 1
    assert R.build_id() == R.source_hash() == R.built_id()
    assert not R.is_stale()


def test_render_code_object_has_no_scratch(tmp_path):
    notes, asm = _kernel_notes_and_asm(tmp_path)
    _kernel_gates(notes, asm, 'igw_render_pov_kernel')
    assert not _forbidden(asm)


def test_render_pov_rejects_bad_arguments_and_a_missing_device():
    import torch
    from gridworld_amd import render as R
    L = R.load()
    buf, p16 = _buffers()
    ok = dict(agent=p16, grid=p16, occ=p16, n=1, atlas=p16, side=128, out=p16, w=64, h=64, c=3)

    def call(**kw):
        a = dict(ok, **kw)
        return L.igw_render_pov(a['agent'], a['grid'], a['occ'], a['n'], a['atlas'], a['side'], a['out'], a['w'],
                                a['h'], a['c'], None)
    for bad in (dict(c=2), dict(c=5), dict(w=0), dict(h=0), dict(w=1025), dict(h=1025), dict(side=12),
                dict(side=264), dict(side=0), dict(n=-1), dict(agent=0), dict(out=0), dict(grid=p16 + 4)):
        assert call(**bad) == -1, bad
        assert L.igw_render_last_error()
    if torch.cuda.is_available():
        assert call(n=0) == 0
    else:
        assert call() == -2 and b'no CPU fallback' in L.igw_render_last_error()
        assert call(n=0) == -2


def test_step_library_build_id_is_untouched_by_the_renderer():
    """The renderer's files are not among the step library's sources: its build id stays the one the committed
    profiles carry."""
    from gridworld_amd import build as B
    srcs = [os.path.basename(s) for s in B.SOURCES + B.HEADERS]
    assert 'igw_render.hip' not in srcs and 'igw_render.h' not in srcs
    ids = {json.load(open(f)).get('build_id') for f in glob.glob(os.path.join(ROOT, 'profiles', 'r06_traffic.json'))}
    assert ids == {B.source_hash()}
