"""Free-camera views (igw_render_views, gridworld_amd/visualizer.py) on the GPU: against the brute-force f64 model of
the frame contract (tests/pov_model.py, DESIGN.md "First-person frames") from eyes no other test can produce -- outside
the build zone, beyond the ground, below it, past the far plane -- and byte for byte against igw_render_pov.

"Equal" is the project's: every pixel whose model margins are outside the boundary band (1e-3 texel, 1e-4 world
units) matches exactly; mismatches inside the band stay <= 0.1 % of the pixels compared.  Each test prints its counts,
and the file prints its wall time (the model is brute force: one 512 x 512 view only, the rest small, on a thread pool).
"""
import os
import time

import numpy as np
import pytest

import pov_model as M
from gridworld_amd import render as R
from render_checks import Tally, _models, _ref_atlas

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CENTRE = np.array([0.0, 1.5, 0.0])      # what the outside eyes look at: the middle of the lower build zone


@pytest.fixture(scope='module', autouse=True)
def _wall_time():
    t0 = time.time()
    yield
    print(f'\ntests/test_gpu_render_views.py: {time.time() - t0:.1f} s wall time')


# ---- structures (in the style of tests/test_gpu_render.py: _scripted) --------------------------------------------
def _ring():
    g = np.zeros((9, 11, 11), np.int8)             # every colour, stacked and spread, seen from all sides
    for c in range(1, 7):
        g[c - 1, 2 + c % 3 * 3, 1 + (c - 1) // 3 * 8] = c
        g[0, 1 + c, 5] = c
        g[2, 5, 1 + c] = 7 - c
    return g


def _tower():
    g = np.zeros((9, 11, 11), np.int8)
    g[:, 7, 3] = np.arange(9) % 6 + 1              # a column at x = 2, z = -2 on a 3 x 3 base
    g[0, 6:9, 2:5] = 3
    return g


def _dense(seed=11):
    rng = np.random.RandomState(seed)
    g = (rng.rand(9, 11, 11) < 0.15) * rng.randint(1, 7, (9, 11, 11))
    return g.astype(np.int8)


def _far_wall():
    g = np.zeros((9, 11, 11), np.int8)             # two layers at x = -5 and -4: the far plane of an eye at x = 25
    g[0:6, 0, :] = 2                               # (depth 30 is x = -5 on its axis) cuts through them
    g[0:4, 1, ::2] = 5
    return g


EMPTY = np.zeros((9, 11, 11), np.int8)
# Eyes off the exact lattice, as in tests/test_gpu_render.py: a ray from an integer or half-integer point through a
# symmetric pixel lands exactly on a texel or face boundary, where f32 and f64 round apart by definition (the
# boundary band); every eye below is moved by this vector BEFORE its angles are derived, so it still looks at its target
OFF = np.array([0.0137, 0.0071, -0.0113])


def _eye_at(eye, target=CENTRE):
    import gridworld_amd as G
    e = np.asarray(eye, np.float64) + OFF
    return (*e, *G.look_at(e, target))


def _outside_views():
    """~40 (pose, grid) pairs with the eye where set_tasks(init_pose=) cannot put it (|x|, |z| <= 10 there)."""
    import gridworld_amd as G
    ring, tower, dense, wall = _ring(), _tower(), _dense(), _far_wall()
    cases = []
    k = 0
    for radius in (8, 14, 22):                      # 22: beyond the ground's edge (18.5), which is then in frame
        for y in (-1, 3, 9):
            orbit = G.orbit_poses(CENTRE, radius, y - CENTRE[1], 3, phase=17 + 40 * k)
            for p in orbit:
                cases.append((_eye_at(p[:3]), (ring, tower, dense)[k % 3]))
                k += 1
    # part of the zone beyond the far plane (depth 30)
    cases += [(_eye_at((25, 6, 0)), wall), (_eye_at((25, 6, 0)), dense), (_eye_at((25, 6, 0), (0, 4, 3)), ring)]
    # below the ground plane (y = -1.5), looking up: no ground (it has a top face only), the blocks from below
    cases += [(_eye_at((2, -3, 1), (0, 2, 0)), ring), (_eye_at((-3, -3, -2), (2, 3, -2)), tower),
              ((0.3 + OFF[0], -3 + OFF[1], -0.2 + OFF[2], 0, 90), dense), (_eye_at((7, -3, 7), (0, 0, 0)), EMPTY)]
    # far outside the 37 x 37 ground, looking in and along its edge: the edge and the sky beyond it in frame
    cases += [(_eye_at((24, 5, 20), (0, 0, 0)), tower), (_eye_at((24, 5, 0), (18, -1.5, 10)), ring),
              (_eye_at((-26, 3, -26), (-18, -1.5, -18)), EMPTY), (_eye_at((0, 2, 30), (0, 0, 0)), dense)]
    # straight down from y = 20 (the whole zone and 21.5 of depth to the ground)
    cases += [((0.3 + OFF[0], 20 + OFF[1], -0.2 + OFF[2], yaw, -90), g) for yaw, g in ((0, ring), (30, dense))]
    cases += [(_eye_at((12, 7, -9)), EMPTY), (_eye_at((-9, 0.5, 13)), wall)]
    return cases


def test_eyes_outside_the_zone_match_the_model_at_all_sizes_channels_and_atlases():
    import torch
    import gridworld_amd as G
    cases = _outside_views()
    assert 38 <= len(cases) <= 44
    poses = np.array([p for p, _ in cases], np.float64)
    grids = np.stack([g for _, g in cases])
    assert (np.abs(poses[:, [0, 2]]).max(1) > 5.5).sum() >= 36            # outside the zone
    assert (np.abs(poses[:, [0, 2]]).max(1) > 10).sum() >= 20             # where no init_pose can stand
    ref, coded, flat = _ref_atlas(), M.coded_atlas(128), R.default_atlas()
    tally = Tally(f'{len(cases)} outside views')
    seen_faces = set()
    for (W, H) in ((64, 64), (96, 40)):
        models = _models(poses, grids, W, H, coded)
        for atlas, channels in ((coded, 3), (ref, 4)) if W == 64 else ((coded, 4), (flat, 3)):
            out = G.render_views(grids, poses, size=(W, H), channels=channels, atlas=atlas)
            assert out.shape == (len(cases), H, W, channels) and out.dtype == torch.uint8 and out.is_cuda
            fr = out.cpu().numpy()
            for k in range(len(cases)):
                tally.add(fr[k], M.shade(models[k], atlas, 4), channels, tag=f'view {k} {W}x{H}')
        for m in models:
            seen_faces |= set(np.unique(m['face']).tolist())
    # sky, all six faces (bottoms from below the ground) and the ground were on screen
    assert seen_faces == {-1, 0, 1, 2, 3, 4, 5, M.GROUND}
    # the far plane cut something: a view of the wall from x = 25 has blocks both drawn and clipped
    far = M.render(poses[27], grids[27], coded, 64, 64, 4)
    assert np.array_equal(grids[27], _far_wall()) and (far['face'] == 3).any() and far['t'][far['face'] == 3].max() > 29
    # below the ground: no ground pixel at all
    assert all(not (m['face'] == M.GROUND).any() for m, p in zip(_models(poses[30:34], grids[30:34], 64, 64, coded),
                                                                 poses[30:34]) if p[1] < -1.5)
    tally.check()


def test_one_512_x_512_view_matches_the_model():
    import gridworld_amd as G
    pose = np.array([_eye_at((11, 5, -9))], np.float64)
    grid = _tower()[None]
    atlas = _ref_atlas()
    out = G.render_views(grid, pose, size=(512, 512), atlas=atlas).cpu().numpy()
    tally = Tally('one 512 x 512 view (64 blocks of one view)')
    tally.add(out[0], M.render(pose[0], grid[0], atlas, 512, 512, 4), 3, tag='512x512')
    tally.check()


def _stepped(n=64, steps=40, seed=7):
    from gridworld_amd import VecGridWorld, workloads
    rng = np.random.RandomState(seed)
    pose = np.stack([rng.uniform(-8, 8, n), rng.uniform(0, 4, n), rng.uniform(-8, 8, n), rng.uniform(-180, 180, n),
                     rng.uniform(-60, 60, n)], 1)
    env = VecGridWorld(n, autoreset=True, max_steps=25)
    env.set_render_atlas(_ref_atlas())
    env.set_tasks(workloads.rt20(n, seed=seed).numpy(), workloads.uniform20(n, seed=seed).numpy(), init_pose=pose)
    env.reset()
    acts = env.fill_actions(steps, seed=seed)       # random actions
    for t in range(steps):
        env.step(acts[t])
    return env


def test_views_from_the_agents_own_poses_are_the_pov_frames_byte_for_byte():
    import torch
    env = _stepped()
    torch.cuda.synchronize()
    poses = M.pose_of_agent(env.agent_buf.cpu().numpy())
    assert int((env.grid_buf != 0).sum()) > 64 and poses.shape == (64, 5)
    for channels, size in ((3, (64, 64)), (4, (64, 64)), (3, (96, 40)), (4, (50, 70))):
        pov = env.render_pov(channels=channels, size=size)
        views = env.render_views(poses, what='grid', channels=channels, size=size)
        assert views.shape == pov.shape and torch.equal(views, pov), (channels, size)
    # rows pick envs: the spectator sees env 5's grid from env 9's eye; that is not env 9's own frame
    rows = np.array([5] * 64)
    mixed = env.render_views(poses, rows=rows)
    import gridworld_amd as G
    direct = G.render_views(env.grid[5:6].contiguous(), poses, view_grid=np.zeros(64, np.int32),
                            atlas=env._atlas())
    assert torch.equal(mixed, direct) and torch.equal(mixed[5], env.render_pov()[5])
    with pytest.raises(ValueError):
        env.render_views(poses, rows=np.array([64] * 64))
    with pytest.raises(ValueError):
        env.render_views(poses, what='occupancy')


def _three_grids_and_orbits():
    import gridworld_amd as G
    grids = np.stack([_ring(), _tower(), _dense()])
    poses = np.concatenate([G.orbit_poses(CENTRE, r, h, 60, phase=3.3) for r, h in ((9, 2), (13, 5), (17, -2))])
    view_grid = np.repeat(np.arange(3), 60)
    return grids, poses, view_grid


def test_view_grid_fans_three_grids_out_to_180_views_in_one_launch():
    import torch
    import gridworld_amd as G
    grids, poses, view_grid = _three_grids_and_orbits()
    fan = G.render_views(grids, poses, view_grid=view_grid)
    assert fan.shape == (180, 64, 64, 3)
    singles = torch.cat([G.render_views(grids[view_grid[v]][None], poses[v:v + 1]) for v in range(180)])
    assert torch.equal(fan, singles)
    assert len(torch.unique(fan.reshape(180, -1), dim=0)) == 180          # 180 different frames
    # no view_grid is arange
    g180 = grids[view_grid]
    assert torch.equal(G.render_views(g180, poses), fan)
    assert torch.equal(G.render_views(g180, poses, view_grid=np.arange(180)), fan)
    with pytest.raises(ValueError):
        G.render_views(grids, poses)                                       # 180 views of 3 grids need a view_grid
    for bad in (np.full(180, 3), np.full(180, -1), np.zeros(179, int), np.zeros(180, float)):
        with pytest.raises(ValueError):
            G.render_views(grids, poses, view_grid=bad)


def test_row_strides_1089_and_1104_are_read_in_place_and_give_the_same_frames():
    import torch
    import gridworld_amd as G
    from gridworld_amd import visualizer as V
    grids, poses, view_grid = _three_grids_and_orbits()
    dev = torch.device('cuda', torch.cuda.current_device())
    dense = torch.from_numpy(grids.reshape(3, 1089)).to(dev)
    wide = torch.full((5, 1104), 3, dtype=torch.int8, device=dev)          # rows 1..3 inside a stride-1104 buffer,
    wide[1:4, :1089] = dense                                               # other rows and the padding filled
    t, stride, n = V._grid_rows(dense, dev)
    assert (t.data_ptr(), stride, n) == (dense.data_ptr(), 1089, 3)
    t, stride, n = V._grid_rows(wide[1:4], dev)
    assert (t.data_ptr(), stride, n) == (wide[1].data_ptr(), 1104, 3)
    four = torch.as_strided(wide, (3, 9, 11, 11), (1104, 121, 11, 1), 1104)   # the layout of VecGridWorld.grid
    assert V._grid_rows(four, dev)[0].data_ptr() == wide[1].data_ptr() and V._grid_rows(four, dev)[1] == 1104
    odd = torch.zeros(3 * 1089 + 1, dtype=torch.int8, device=dev)[1:].view(3, 1089)   # rows at odd addresses
    odd.copy_(dense)
    assert V._grid_rows(odd, dev)[0].data_ptr() == odd.data_ptr() and odd.data_ptr() % 2 == 1
    a = G.render_views(dense, poses, view_grid=view_grid)
    for other in (wide[1:4], four, odd, wide[1:4, :1089], grids.astype(np.int64), dense.cpu()):
        assert torch.equal(G.render_views(other, poses, view_grid=view_grid), a)


def test_a_device_side_view_grid_out_of_range_leaves_its_frame_untouched():
    import torch
    import gridworld_amd as G
    grids, poses, _ = _three_grids_and_orbits()
    poses = poses[[0, 70, 140, 20, 100, 179]]
    rows = [0, 3, -1, 2, 2 ** 31 - 1, 1]
    vg = torch.tensor(rows, dtype=torch.int32, device='cuda')
    out = torch.full((6, 40, 96, 4), 0x5A, dtype=torch.uint8, device='cuda')
    got = G.render_views(grids, poses, view_grid=vg, size=(96, 40), channels=4, out=out)
    assert got is out
    for v, r in enumerate(rows):
        if 0 <= r < 3:
            want = G.render_views(grids[r][None], poses[v:v + 1], size=(96, 40), channels=4)[0]
            assert torch.equal(out[v], want) and not bool((out[v] == 0x5A).all())
        else:
            assert bool((out[v] == 0x5A).all()), v


def test_what_target_and_start_show_the_task_table():
    import torch
    import gridworld_amd as G
    from gridworld_amd import VecGridWorld, workloads
    n = 16
    targets, starts = workloads.rt20(n, seed=3).numpy(), workloads.uniform20(n, seed=4).numpy()
    poses = G.orbit_poses(CENTRE, 12, 4, n, phase=5)
    # with a starting grid the table's target row is the synthetic target the reward counts (target - start,
    # VecGridWorld.targets()); the starting grid and, right after the reset, the live grid are the starts
    both = VecGridWorld(n)
    both.set_tasks(targets, starts)
    both.reset()
    assert torch.equal(both.render_views(poses, what='start'), G.render_views(starts, poses))
    assert torch.equal(both.render_views(poses, what='grid'), G.render_views(starts, poses))
    assert torch.equal(both.render_views(poses, what='target'), G.render_views(both.targets(), poses))
    # without one it is the task's target grid: the goal image
    env = VecGridWorld(n)
    env.set_tasks(targets)
    env.reset()
    goal = env.render_views(poses, what='target')
    assert goal.shape == (n, 64, 64, 3)
    assert torch.equal(goal, G.render_views(targets, poses))
    assert len(torch.unique(goal.reshape(n, -1), dim=0)) == n
    # rows = task rows; the env's atlas and render_size are the defaults, size / atlas / channels override them
    rows = np.array([3, 3, 0, 15])
    env.set_render_atlas(_ref_atlas())
    env.render_size = (48, 32)
    some = env.render_views(poses[:4], rows=rows, what='target', channels=4)
    assert some.shape == (4, 32, 48, 4)
    assert torch.equal(some, G.render_views(targets[rows], poses[:4], size=(48, 32), channels=4, atlas=_ref_atlas()))
    assert not torch.equal(goal[0], G.render_views(targets[1:2], poses[:1])[0])


BLOCKS = [(0, 0, 0, 1), (1, 0, 0, 2), (0, 1, 0, 3), (-2, 0, 3, 4), (-2, 1, 3, 5), (4, 0, -4, 6), (4, 8, -4, 1)]


def test_visualizer_render_and_render_batch_match_the_model_and_each_other():
    import gridworld_amd as G
    atlas = _ref_atlas()
    vis = G.Visualizer(render_size=(96, 64), atlas=atlas)
    eye = np.array((9, 6, 9)) + OFF
    rot = G.look_at(eye, (0, 1, 0))
    img = vis.render(eye, rot, blocks=BLOCKS)
    assert isinstance(img, np.ndarray) and img.shape == (64, 96, 3) and img.dtype == np.uint8
    grid = G.visualizer.blocks_to_grid(BLOCKS, -1)                         # each block one level down
    assert grid[0, 5, 5] == 1 and grid[8, 9, 1] == 1 and np.array_equal(vis.grid(), grid)
    tally = Tally('Visualizer')
    tally.add(img, M.render((*eye, *rot), grid, atlas, 96, 64, 4), 3, tag='render')
    assert np.array_equal(vis.render(), img)                               # pose and world persist
    # T poses of the current world in one launch = T render() calls
    poses = G.orbit_poses((0, 1, 0), 13, 4, 12, phase=7)
    positions, rotations = G.visualizer.split_poses(poses)
    batch = vis.render_batch(positions, rotations)
    assert batch.shape == (12, 64, 96, 3) and batch.dtype == np.uint8
    for t in range(12):
        assert np.array_equal(batch[t], vis.render(positions[t], rotations[t])), t
    for t, res in enumerate(_models(poses, [grid] * 12, 96, 64, atlas)):
        tally.add(batch[t], res, 3, tag=f'render_batch {t}')
    # T (pose, block list) pairs: the structure growing block by block
    lists = [BLOCKS[:t + 1] for t in range(len(BLOCKS))]
    grown = vis.render_batch(positions[:7], rotations[:7], blocks=lists)
    for t in range(7):
        assert np.array_equal(grown[t], vis.render(positions[t], rotations[t], blocks=lists[t])), t
    assert np.array_equal(grown[6], batch[6]) and not np.array_equal(grown[0], batch[0])
    # set_world_state works in world coordinates (no shift); the default pose looks along -z from the origin
    flat = G.Visualizer()
    flat.set_world_state([(0, 0, -3, 3), (1, -1, -4, 6)])
    tally.add(flat.render((OFF[0], OFF[1], OFF[2])), M.render((*OFF, 0, 0), flat.grid(), R.default_atlas(), 64, 64, 4),
              3, tag='default pose')
    tally.check()


def test_two_launches_give_the_same_bytes_and_out_is_written_in_place_on_the_current_stream():
    import torch
    import gridworld_amd as G
    grids, poses, view_grid = _three_grids_and_orbits()
    out = torch.zeros((180, 64, 64, 3), dtype=torch.uint8, device='cuda')
    r1 = G.render_views(grids, poses, view_grid=view_grid, out=out)
    assert r1 is out and r1.data_ptr() == out.data_ptr() and bool(out.any())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        r2 = G.render_views(grids, poses, view_grid=view_grid)
    torch.cuda.current_stream().wait_stream(s)
    assert torch.equal(r1, r2)
    for bad in (out[:, :, :, :2], out[:179], out.cpu(), out.to(torch.int8), out.permute(0, 2, 1, 3)):
        with pytest.raises(ValueError):
            G.render_views(grids, poses, view_grid=view_grid, out=bad)
    assert G.render_views(grids, np.zeros((0, 5)), view_grid=np.zeros(0, int)).shape == (0, 64, 64, 3)
