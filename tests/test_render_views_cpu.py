"""CPU side of the free-camera views (igw_render_views, include/igw_render.h; gridworld_amd/visualizer.py): the entry
point is declared, exported and bound, checks its arguments like its siblings, reports a missing device, and its
kernel passes the code-object gates of the pov kernel; the camera helpers and the Visualizer's world bookkeeping are
host code and are checked here without a launch.  The GPU comparisons are tests/test_gpu_render_views.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import pov_model as M
from render_checks import LLVM, _buffers, _kernel_gates, _kernel_notes_and_asm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_render_views_is_declared_exported_and_bound():
    from gridworld_amd import render as R
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'igw_render.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+igw_render_views\s*\(', src)
    assert 'igw_render_views' in R.EXPORTS
    L = R.load()
    assert hasattr(L, 'igw_render_views') and len(L.igw_render_views.argtypes) == 13
    syms = subprocess.check_output([os.path.join(LLVM, 'llvm-readelf'), '--dyn-syms', R.LIB], text=True)
    assert re.search(r'FUNC\s+GLOBAL\s+DEFAULT\s+\d+\s+igw_render_views$', syms, flags=re.M)
    assert callable(R.render_views_into)
    assert L.igw_render_version() == 1


def test_render_views_code_object_gates(tmp_path):
    notes, asm = _kernel_notes_and_asm(tmp_path)
    kern, val, body = _kernel_gates(notes, asm, 'igw_render_views_kernel')
    # the siblings' tests select by their names
    assert 'igw_render_pov_kernel' not in kern and 'igw_render_episodes_kernel' not in kern
    assert 'global_store' in body and 'ds_or' in body       # vector stores of the frame, the LDS bitmap build


def test_render_views_rejects_bad_arguments_and_a_missing_device():
    import torch
    from gridworld_amd import render as R
    L = R.load()
    buf, p = _buffers()
    ok = dict(grids=p, stride=1104, n_grids=3, view_grid=p, pose=p, m=8, atlas=p, side=128, out=p, w=64, h=64, c=3)

    def call(**kw):
        a = dict(ok, **kw)
        return L.igw_render_views(a['grids'], a['stride'], a['n_grids'], a['view_grid'], a['pose'], a['m'],
                                  a['atlas'], a['side'], a['out'], a['w'], a['h'], a['c'], None)
    bad = [dict(m=-1), dict(n_grids=-1), dict(stride=1088), dict(stride=0), dict(stride=-1104),
           dict(view_grid=0, n_grids=7), dict(view_grid=0, n_grids=0), dict(c=2), dict(c=5), dict(w=0), dict(h=0),
           dict(w=1025), dict(h=1025), dict(side=12), dict(side=264), dict(side=0), dict(pose=p + 4),
           dict(view_grid=p + 2), dict(atlas=p + 1)]
    bad += [{k: 0} for k in ('grids', 'pose', 'atlas', 'out')]
    for b in bad:
        assert call(**b) == -1, b
        assert L.igw_render_last_error().startswith(b'igw_render_views: '), b
    # valid without any alignment of the grids (a dense stride-1089 array), and with a NULL view_grid when every
    # view has its own row; m == 0 reads nothing: null buffers are fine, and the call is a no-op
    fine = [dict(), dict(grids=p + 1, stride=1089), dict(view_grid=0, n_grids=8), dict(view_grid=0, n_grids=9)]
    nulls = dict(grids=0, view_grid=0, pose=0, atlas=0, out=0, m=0, n_grids=0)
    if torch.cuda.is_available():
        assert call(**nulls) == 0
    else:
        for f in fine:
            assert call(**f) == -2 and b'no CPU fallback' in L.igw_render_last_error(), f
        assert call(**nulls) == -2


def test_python_interface_needs_a_device_and_checks_its_arguments_first():
    import torch
    import gridworld_amd as G
    from gridworld_amd import render as R
    assert G.render_views is G.visualizer.render_views and callable(G.VecGridWorld.render_views)
    if torch.cuda.is_available():
        return                                      # the no-device message is for hosts without a GPU
    with pytest.raises(R.RenderError):
        G.render_views(np.zeros((1, 9, 11, 11), np.int8), np.zeros((1, 5)))
    with pytest.raises(R.RenderError):
        G.Visualizer().render()


def test_look_at_points_the_forward_vector_at_the_target():
    import gridworld_amd as G
    rng = np.random.RandomState(5)
    pairs = [(rng.uniform(-25, 25, 3), rng.uniform(-6, 8, 3)) for _ in range(500)]
    pairs += [((1.5, 0, -2), (1.5, 9, -2)), ((1.5, 20, -2), (1.5, -1, -2)),                 # straight up and down
              ((0, 0, 0), (0, 0, -1)), ((0, 0, 0), (0, 0, 1)), ((0, 0, 0), (1, 0, 0)), ((0, 0, 0), (-1, 0, 0))]
    worst = 1.0
    for eye, target in pairs:
        yaw, pitch = G.look_at(eye, target)
        v = np.asarray(target, np.float64) - np.asarray(eye, np.float64)
        v /= np.linalg.norm(v)
        f = M.basis(yaw, pitch)[0]
        worst = min(worst, float(f @ v))
        assert f @ v >= 1 - 1e-12, (eye, target, yaw, pitch)
        assert -180 <= yaw <= 180 and -90 <= pitch <= 90
    print('look_at: smallest forward . v = 1 - %.3g' % (1 - worst))
    assert G.look_at((0, 0, 0), (0, 0, -1)) == (0.0, 0.0)           # yaw 0 looks along -z
    assert G.look_at((0, 0, 0), (0, 3, 0)) == (0.0, 90.0) and G.look_at((0, 0, 0), (0, -3, 0)) == (0.0, -90.0)
    assert np.allclose(G.look_at((0, 0, 0), (1, 0, 0)), (90.0, 0.0))
    assert np.allclose(G.look_at((0, 0, 0), (1, 1, -1)), (45.0, np.degrees(np.arcsin(1 / np.sqrt(3)))))
    for eye in ((1, 2, 3), (0, 0, 0)):
        with pytest.raises(ValueError):
            G.look_at(eye, eye)
    with pytest.raises(ValueError):
        G.look_at((0, 0, 0), (np.nan, 0, 0))


def test_orbit_poses_stand_on_the_circle_and_look_at_the_centre():
    import gridworld_amd as G
    centre = np.array([0.5, 1.0, -2.0])
    for n, radius, height in ((1, 8, -1), (8, 14, 3), (180, 22, 9)):
        p = G.orbit_poses(centre, radius, height, n)
        assert p.shape == (n, 5) and p.dtype == np.float64
        rel = p[:, :3] - centre
        assert np.allclose(np.hypot(rel[:, 0], rel[:, 2]), radius, atol=1e-12)
        assert np.allclose(rel[:, 1], height, atol=1e-12)
        for k in range(n):
            v = -rel[k] / np.linalg.norm(rel[k])
            assert M.basis(p[k, 3], p[k, 4])[0] @ v >= 1 - 1e-12
        if n > 1:   # evenly spaced: all neighbours at the same chord
            chord = np.linalg.norm(np.roll(rel, -1, 0) - rel, axis=1)
            assert np.allclose(chord, 2 * radius * np.sin(np.pi / n), atol=1e-9)
    assert G.orbit_poses(centre, 5, 2, 0).shape == (0, 5)
    # phase turns the ring: a quarter turn of 4 eyes is the same ring, started one eye later
    a, b = G.orbit_poses(centre, 5, 2, 4), G.orbit_poses(centre, 5, 2, 4, phase=90)
    assert np.allclose(np.roll(a, -1, 0)[:, :3], b[:, :3], atol=1e-12)
    pos, rot = G.visualizer.split_poses(a)
    assert pos.shape == (4, 3) and rot.shape == (4, 2)


def _cells(grid):
    return {(int(x) - 5, int(y) - 1, int(z) - 5): int(grid[y, x, z]) for y, x, z in np.argwhere(grid)}


def test_visualizer_world_bookkeeping_without_a_launch():
    import gridworld_amd as G
    vis = G.Visualizer(render_size=(96, 40))
    assert vis.render_size == (96, 40) and vis.position == (0, 0, 0) and vis.rotation == (0, 0)
    assert vis.grid().shape == (9, 11, 11) and vis.grid().dtype == np.int8 and not vis.grid().any()
    vis.set_world_state([(0, -1, 0, 1), (5, 7, -5, 6), (-5, 0, 5, 3)])
    assert _cells(vis.grid()) == {(0, -1, 0): 1, (5, 7, -5): 6, (-5, 0, 5): 3} == vis.world
    assert vis.grid()[0, 5, 5] == 1 and vis.grid()[8, 10, 0] == 6       # [y+1][x+5][z+5]
    vis.set_world_state([(0, -1, 0, 4)])                                 # add replaces
    assert vis.world[(0, -1, 0)] == 4 and len(vis.world) == 3
    vis.set_world_state([(5, 7, -5, 2), (1, 1, 1, 1)], add=False)         # ids are ignored, an absent block too
    assert _cells(vis.grid()) == {(0, -1, 0): 4, (-5, 0, 5): 3}
    vis.clear()
    assert not vis.world and not vis.grid().any()

    vis.set_agent_state((1, 2, 3), (40, -10))
    assert vis.position == (1, 2, 3) and vis.rotation == (40, -10)
    vis.set_agent_state(rotation=[5, 6])
    assert vis.position == (1, 2, 3) and vis.rotation == (5, 6)
    assert np.array_equal(vis.pose(), [1, 2, 3, 5, 6]) and vis.pose().dtype == np.float64
    with pytest.raises(ValueError):
        vis.set_agent_state(position=(1, 2))

    # render(blocks=) / render_batch(blocks=) replace the world, each block one level down
    vis.set_world_state([(2, 2, 2, 2)])
    vis.replace_world([(0, 0, 0, 1), (1, 8, -1, 5)])
    assert vis.world == {(0, -1, 0): 1, (1, 7, -1): 5}
    poses, grids = vis.batch_inputs([(9, 2, 9), (0, 20, 0)], [(10, 0), (0, -90)])
    assert poses.shape == (2, 5) and grids.shape == (1, 9, 11, 11) and _cells(grids[0]) == vis.world
    assert vis.position == (0, 20, 0) and vis.rotation == (0, -90)
    poses, grids = vis.batch_inputs([(9, 2, 9), (0, 20, 0)], [(10, 0), (0, -90)], [[(0, 0, 0, 1)], [(3, 1, 3, 6)]])
    assert grids.shape == (2, 9, 11, 11) and grids.dtype == np.int8
    assert _cells(grids[0]) == {(0, -1, 0): 1} and _cells(grids[1]) == {(3, 0, 3): 6} == vis.world
    with pytest.raises(ValueError):
        vis.batch_inputs([(0, 0, 0)], [(0, 0), (1, 1)])
    with pytest.raises(ValueError):
        vis.batch_inputs([(0, 0, 0)], [(0, 0)], [[], []])


@pytest.mark.parametrize('block', [(6, 0, 0, 1), (-6, 0, 0, 1), (0, 8, 0, 1), (0, -2, 0, 1), (0, 0, 6, 1),
                                   (0, 0, -6, 1), (0, 0, 0, 0), (0, 0, 0, 7), (0, 0, 0, -1), (0.5, 0, 0, 1),
                                   (0, 0, 0)])
def test_visualizer_refuses_blocks_outside_the_zone_and_unknown_ids(block):
    import gridworld_amd as G
    vis = G.Visualizer()
    vis.set_world_state([(1, 1, 1, 1)])
    with pytest.raises(ValueError):
        vis.set_world_state([(2, 2, 2, 2), block])
    assert vis.world == {(1, 1, 1): 1}                                   # nothing of a refused list is applied
    with pytest.raises(ValueError):
        # placed at y - 1: the same cell as above when given one level higher
        vis.replace_world([(2, 2, 2, 2), block if len(block) != 4 else (block[0], block[1] + 1, *block[2:])])
    assert vis.world == {(1, 1, 1): 1}


def test_render_blocks_shift_moves_the_zone_limits_with_it():
    import gridworld_amd as G
    vis = G.Visualizer()
    vis.replace_world([(0, 0, 0, 1), (0, 8, 0, 2)])                     # y - 1 = -1 and 7: the zone's floor and top
    assert vis.world == {(0, -1, 0): 1, (0, 7, 0): 2}
    for y in (-1, 9):
        with pytest.raises(ValueError):
            vis.replace_world([(0, y, 0, 1)])
