"""CPU side of the renderer's planes (depth, label, surface; DESIGN.md section 8, "Planes"): the plane model
(tests/aux_model.py) on analytic scenes, the host-side readers (decode_surface, unproject), and the library as a
cross-compiled artefact -- declared symbols, argument checks of the _aux entries, code-object gates of their kernels.
The GPU comparison of kernel against model is tests/test_gpu_render_aux.py."""
import os
import re

import numpy as np
import pytest

import aux_model as A
import pov_model as M
from render_checks import _buffers, _kernel_gates, _kernel_notes_and_asm
from test_render_cpu import VIEWS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLD_KERNELS = ('igw_render_pov_kernel', 'igw_render_episodes_kernel', 'igw_render_views_kernel')
AUX_KERNELS = ('igw_aux_pov_kernel', 'igw_aux_episodes_kernel', 'igw_aux_views_kernel')


def _atlas():
    from gridworld_amd import render as R
    return R.default_atlas()


# ---- the model on analytic scenes -------------------------------------------------------------------------------
@pytest.mark.parametrize('face', list(VIEWS))
def test_single_block_gives_the_surface_code_label_and_plane_depth_of_each_face(face):
    pose, axis, plane = VIEWS[face]
    W = H = 32
    for colour in (1, 4, 6):
        g = np.zeros((9, 11, 11), np.int8)
        g[3, 5, 5] = colour                               # world (0, 2, 0)
        r = M.render(pose, g, _atlas(), W, H)
        depth, label, surface = A.planes(r, pose, g)
        d = M.rays(pose[3], pose[4], W, H)
        e = np.array(pose[:3], np.float64)
        t = (plane - e[axis]) / d[..., axis]
        loc = e + t[..., None] * d - (np.array([0, 2, 0]) - 0.5)
        on = (loc >= 0).all(-1) & (loc <= 1).all(-1) & M.clean(r)
        assert on.sum() > 50, face
        code = M.FACE_NAMES.index(face) * 1089 + 3 * 121 + 5 * 11 + 5
        assert (surface[on] == code).all() and (label[on] == colour).all()
        np.testing.assert_allclose(depth[on], t[on], rtol=1e-12)
        # nothing else is a block: the rest is ground or sky, with their own codes
        rest = surface[~on & M.clean(r)]
        assert ((rest == -1) | (rest >= 6 * 1089)).all()


def test_empty_grid_gives_ground_quads_white_inside_and_grey_outside():
    g = np.zeros((9, 11, 11), np.int8)
    pose = (0.3, 2.0, 0.2, 30.0, -40.0)
    r = M.render(pose, g, _atlas(), 64, 64)
    depth, label, surface = A.planes(r, pose, g)
    gnd = (r['face'] == M.GROUND) & M.clean(r)
    assert gnd.sum() > 1500
    d = M.rays(pose[3], pose[4], 64, 64)
    t = (-1.5 - pose[1]) / d[..., 1]
    hx, hz = pose[0] + t * d[..., 0], pose[2] + t * d[..., 2]
    q = surface[gnd] - 6 * 1089
    qx, qz = q // 37 - 18, q % 37 - 18
    assert (np.abs(hx[gnd] - qx) <= 0.5).all() and (np.abs(hz[gnd] - qz) <= 0.5).all()
    white = (np.abs(qx) <= 5) & (np.abs(qz) <= 5)
    assert white.any() and (~white).any()
    assert (label[gnd][white] == 7).all() and (label[gnd][~white] == 8).all()
    np.testing.assert_allclose(depth[gnd], t[gnd], rtol=1e-12)
    assert surface.max() <= 6 * 1089 + 37 * 37 - 1 < 2 ** 15


def test_everything_above_the_horizon_is_sky():
    g = np.zeros((9, 11, 11), np.int8)
    pose = (0.0, 0.0, 0.0, 0.0, 0.0)
    r = M.render(pose, g, _atlas(), 64, 64)
    depth, label, surface = A.planes(r, pose, g)
    assert np.isinf(depth[:32]).all() and (label[:32] == 0).all() and (surface[:32] == -1).all()
    assert A.SKY == (np.inf, 0, -1)
    assert np.isfinite(depth[40:]).all() and (surface[40:] >= 6 * 1089).all()


# ---- the readers ------------------------------------------------------------------------------------------------
def test_decode_surface_round_trips_every_code():
    import torch
    import gridworld_amd as G
    f, y, x, z = np.meshgrid(np.arange(6), np.arange(9), np.arange(11), np.arange(11), indexing='ij')
    codes = (f * 1089 + y * 121 + x * 11 + z).astype(np.int16)
    assert codes.min() == 0 and codes.max() == 6 * 1089 - 1 and len(np.unique(codes)) == codes.size
    for got in (G.decode_surface(codes), [t.numpy() for t in G.decode_surface(torch.from_numpy(codes))]):
        for a, b in zip(got, (f, y, x, z)):
            assert np.array_equal(a, b)
    other = np.concatenate([[-1], 6 * 1089 + np.arange(37 * 37)]).astype(np.int16)
    for got in (G.decode_surface(other), [t.numpy() for t in G.decode_surface(torch.from_numpy(other))]):
        for a in got:
            assert (a == -1).all()


def test_unproject_is_eye_plus_depth_times_the_models_ray():
    import torch
    import gridworld_amd as G
    rng = np.random.RandomState(4)
    W, H = 24, 16
    poses = np.stack([rng.uniform(-8, 8, 5), rng.uniform(-1, 6, 5), rng.uniform(-8, 8, 5), rng.uniform(-360, 360, 5),
                      rng.uniform(-90, 90, 5)], 1)
    depth = rng.uniform(0.1, 30, (5, H, W)).astype(np.float32)
    depth[:, 0, :3] = np.inf
    pts = G.unproject(torch.from_numpy(depth), poses, size=(W, H))
    assert pts.shape == (5, H, W, 3) and pts.dtype == torch.float64
    pts = pts.numpy()
    for k in range(5):
        want = poses[k, :3] + depth[k].astype(np.float64)[..., None] * M.rays(poses[k, 3], poses[k, 4], W, H)
        fin = np.isfinite(depth[k])
        np.testing.assert_allclose(pts[k][fin], want[fin], rtol=0, atol=1e-12)
        assert np.isnan(pts[k][~fin]).all()
    with pytest.raises(ValueError):
        G.unproject(torch.from_numpy(depth), poses, size=(H, W))
    with pytest.raises(ValueError):
        G.unproject(torch.from_numpy(depth), poses[:3])


def test_unknown_or_duplicated_outputs_raise_before_any_device_work():
    import gridworld_amd as G
    from gridworld_amd import render as R
    g = np.zeros((1, 9, 11, 11), np.int8)
    p = np.zeros((1, 5))
    for bad in (('rgb', 'normals'), ('depth', 'depth'), ()):
        with pytest.raises(ValueError):
            G.render_views(g, p, outputs=bad)
        with pytest.raises(ValueError):
            G.Visualizer().render(outputs=bad)
        with pytest.raises(ValueError):
            G.Visualizer().render_batch(p[:, :3], p[:, 3:], outputs=bad)
        with pytest.raises(ValueError):
            R.check_outputs(bad)
    assert R.check_outputs(['surface', 'rgb']) == ('surface', 'rgb')


# ---- the library ----------------------------------------------------------------------------------------------------
def test_the_aux_entries_are_declared_exported_and_detectable():
    from gridworld_amd import render as R
    src = open(os.path.join(ROOT, 'include', 'igw_render.h')).read()
    assert re.search(r'#define IGW_RENDER_HAS_AUX 1\b', src) and re.search(r'#define IGW_RENDER_VERSION 1\b', src)
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = sorted(set(re.findall(r'\b(igw_render_[a-z0-9_]+)\s*\(', code)))
    assert sorted(R.EXPORTS) == declared
    L = R.load()
    for name in ('igw_render_pov_aux', 'igw_render_episodes_aux', 'igw_render_views_aux'):
        assert name in declared and hasattr(L, name)
    assert L.igw_render_version() == 1
    assert [f[0] for f in R.Aux._fields_] == re.findall(r'\*\s*(\w+);', re.search(
        r'typedef struct igw_render_aux \{(.*?)\}', code, re.S).group(1))


def _aux(depth=0, label=0, surface=0):
    from gridworld_amd import render as R
    return R.Aux(depth or None, label or None, surface or None)


def _entries(L, p16):
    """name -> call(out, aux, **changes) of the three _aux entries with otherwise valid arguments."""
    import ctypes

    def pov(out, aux, n=1, c=3, grid=p16):
        return L.igw_render_pov_aux(p16, grid, p16, n, p16, 128, out, 64, 64, c, ctypes.byref(aux), None)

    def episodes(out, aux, n=1, c=3, grid=p16):
        return L.igw_render_episodes_aux(p16, 10, p16, p16, p16, grid, p16, n, 5, p16, 128, out, 6, 64, 64, c,
                                         ctypes.byref(aux), None)

    def views(out, aux, n=1, c=3, grid=p16):
        return L.igw_render_views_aux(grid, 1104, 1, None, p16, n, p16, 128, out, 64, 64, c, ctypes.byref(aux), None)
    return {'pov': pov, 'episodes': episodes, 'views': views}


@pytest.mark.parametrize('entry', ['pov', 'episodes', 'views'])
def test_aux_entries_reject_bad_arguments_and_a_missing_device(entry):
    import torch
    from gridworld_amd import render as R
    L = R.load()
    buf, p16 = _buffers()
    call = _entries(L, p16)[entry]
    # nothing to write: out and every plane NULL -- ahead of the missing device
    assert call(None, _aux()) == -1 and b'nothing to write' in L.igw_render_last_error()
    for bad in (dict(depth=p16 + 2), dict(depth=p16 + 1), dict(surface=p16 + 1), dict(depth=p16, surface=p16 + 3)):
        assert call(p16, _aux(**bad)) == -1, bad
        assert b'aligned' in L.igw_render_last_error()
        assert call(None, _aux(label=p16, **bad)) == -1, bad
    # the sibling's own checks still come first
    assert call(p16, _aux(depth=p16), c=2) == -1 and call(p16, _aux(depth=p16), n=-1) == -1
    if entry != 'views':
        assert call(p16, _aux(depth=p16), grid=p16 + 4) == -1
    # valid: any single output, label at any address
    for out, aux in ((p16, _aux()), (None, _aux(depth=p16 + 4)), (None, _aux(label=p16 + 1)),
                     (None, _aux(surface=p16 + 2)), (p16, _aux(p16, p16 + 3, p16 + 6))):
        if torch.cuda.is_available():
            assert call(out, aux, n=0) == 0
        else:
            assert call(out, aux) == -2 and b'no CPU fallback' in L.igw_render_last_error()
            assert call(out, aux, n=0) == -2


def test_aux_kernels_pass_the_code_object_gates_and_the_plain_kernels_hold_no_plane_code(tmp_path):
    notes, asm = _kernel_notes_and_asm(tmp_path)
    for old, new in zip(OLD_KERNELS, AUX_KERNELS):
        _, val, body = _kernel_gates(notes, asm, old)       # exactly one kernel matches the old name
        _, aval, abody = _kernel_gates(notes, asm, new)
        assert old not in new
        # same LDS: the planes leave from registers, nothing is staged for them
        assert aval('group_segment_fixed_size') == val('group_segment_fixed_size')
        # the planes are one 4-, one 2- and one 1-byte vector store per pixel; the surface's 2-byte store is the one
        # instruction the colour path never issues, so the plain kernels must not hold it
        assert 'global_store_short' in abody and 'global_store_dword ' in abody + ' '
        assert 'global_store_short' not in body


def test_the_gpu_scenes_are_clean_on_at_least_nine_pixels_in_ten():
    for k, (pose, grid) in enumerate(A.scenes()):
        r = M.render(pose, grid, _atlas(), 64, 64)
        share = float(M.clean(r).mean())
        assert share >= 0.9, (k, share)
    faces = set()
    for pose, grid in A.scenes():
        faces |= set(M.render(pose, grid, _atlas(), 64, 64)['face'].ravel().tolist())
    assert faces == {-1, 0, 1, 2, 3, 4, 5, 6}
