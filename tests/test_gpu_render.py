"""The HIP first-person renderer (libigw_render.so) against the brute-force CPU model of the contract
(tests/pov_model.py, DESIGN.md "First-person frames").  "Equal": every pixel whose model margins are outside the
boundary band (1e-3 texel, 1e-4 world units) matches exactly; mismatches inside the band stay <= 0.1 % of the pixels
compared.  Each test prints its mismatch counts.  All of these together are budgeted at <= 60 s."""
import os

import numpy as np
import pytest

import pov_model as M
from gridworld_amd import render as R
from render_checks import Tally, _models, _ref_atlas

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _state(env, rows=None):
    """(poses [n,5] f64, grids [n,9,11,11]) of a batch, read back from its agent records and grid."""
    import torch
    torch.cuda.synchronize()
    a = env.agent_buf.cpu().numpy()
    g = env.grid_buf.cpu().numpy()[:, :1089].reshape(-1, 9, 11, 11)
    if rows is not None:
        a, g = a[rows], g[rows]
    return M.pose_of_agent(a), g


def _scripted():
    """~40 (pose, grid) pairs: pitch +-90, the four axis yaws, the far corners, every colour on every face."""
    rng = np.random.RandomState(11)
    ring = np.zeros((9, 11, 11), np.int8)          # every colour, stacked and spread, seen from all sides
    for c in range(1, 7):
        ring[c - 1, 2 + c % 3 * 3, 1 + (c - 1) // 3 * 8] = c
        ring[0, 1 + c, 5] = c
        ring[2, 5, 1 + c] = 7 - c
    tower = np.zeros((9, 11, 11), np.int8)
    tower[:, 7, 3] = np.arange(9) % 6 + 1         # a column at x = 2, z = -2 on a 3 x 3 base
    tower[0, 6:9, 2:5] = 3
    dense = (rng.rand(9, 11, 11) < 0.15) * rng.randint(1, 7, (9, 11, 11))
    dense[:, 4:7, 4:7] = 0                         # room for the eye
    dense = dense.astype(np.int8)
    empty = np.zeros((9, 11, 11), np.int8)
    cases = []
    for g in (ring, tower):
        cases += [((0, 3, 0, 0, -90), g), ((0, -1, 0, 30, 90), g), ((0.3, 8, -0.2, 10, -90), g)]
        for yaw in (0, 90, 180, 270):
            cases += [((0, 0, 0, yaw, 0), g), ((0.2, 1.3, 0.1, yaw, -30), g)]
        for sx in (-10, 10):
            for sz in (-10, 10):
                yaw = np.degrees(np.arctan2(-sx, sz))   # forward (sin yaw, ., -cos yaw) towards the far corner
                cases.append(((sx, 0.5, sz, yaw, -5), g))
    for _ in range(6):
        cases.append(((rng.uniform(-1, 1), rng.uniform(-1, 4), rng.uniform(-1, 1), rng.uniform(-180, 180),
                       rng.uniform(-80, 80)), dense))
    cases += [((3, 2, -4, 45, -20), empty), ((0, 0, -0.38, 60, 0), _wall_grid())]
    # eyes off the exact lattice: a ray from an integer point through a symmetric pixel lands exactly on a texel or
    # face boundary, where f32 and f64 round apart by definition (the boundary band); the angles stay exact
    # (towards the centre at the |x| = |z| = 10 corners, the limit of a task's init_pose)
    off = np.array([0.0137, 0.0071, -0.0113])
    out = []
    for p, g in cases:
        e = np.array(p[:3], np.float64)
        e = np.where(np.abs(e + off) <= 10, e + off, e - off)
        out.append(((*e, p[3], p[4]), g))
    return out


def _wall_grid():
    g = np.zeros((9, 11, 11), np.int8)
    g[0:3, :, 4] = 3
    return g


def _env_with(cases, **kw):
    from gridworld_amd import VecGridWorld
    n = len(cases)
    env = VecGridWorld(n, **kw)
    grids = np.stack([g for _, g in cases])
    env.set_tasks(grids, grids, init_pose=np.array([p for p, _ in cases], np.float64))
    env.reset()
    return env


def test_scripted_poses_sizes_channels_and_atlases_match_the_model():
    import torch
    cases = _scripted()
    env = _env_with(cases)
    poses, grids = _state(env)
    flat, ref, coded = R.default_atlas(), _ref_atlas(), M.coded_atlas(128)
    tally = Tally('scripted')
    for (W, H) in ((64, 64), (96, 64), (64, 96), (1, 1), (65, 65)):
        models = _models(poses, grids, W, H, coded)
        combos = ((coded, 3), (ref, 4), (flat, 3)) if W == H == 64 else ((coded, 4 if W == 65 else 3), (flat, 3))
        for atlas, channels in combos:
            env.set_render_atlas(atlas)
            out = env.render_pov(channels=channels, size=(W, H))
            assert out.shape == (len(cases), H, W, channels) and out.dtype == torch.uint8
            fr = out.cpu().numpy()
            for k in range(len(cases)):
                tally.add(fr[k], M.shade(models[k], atlas, 4), channels)
        if (W, H) == (64, 64):
            # every colour on every face, and the ground and sky, were on screen
            seen = {(int(f), int(c)) for m, (_, g) in zip(models, cases) for f, c in
                    zip(m['face'].ravel(), m['texel'][..., 0].ravel() // 32 + 4 * (m['texel'][..., 1].ravel() // 32))
                    if 0 <= f < 6}
            for f in range(6):
                for tile in range(2, 8):
                    assert (f, tile) in seen, (M.FACE_NAMES[f], tile)
    tally.check()


def _stepped_batch(flying, seed, atlas=None):
    import torch
    from gridworld_amd import VecGridWorld, workloads
    n = 256
    goals = np.load(os.path.join(HERE, 'golden', 'cdm_goals.npz'))['dense']
    tg_cdm, starts = workloads.cdm(n, seed, goals)
    targets = tg_cdm if flying else workloads.rt20(n, seed)
    rng = np.random.RandomState(seed)
    pose = np.stack([rng.uniform(-8, 8, n), rng.uniform(0, 4, n), rng.uniform(-8, 8, n), rng.uniform(-180, 180, n),
                     rng.uniform(-60, 60, n)], 1)
    env = VecGridWorld(n, autoreset=True, max_steps=40, action_space='flying' if flying else 'walking',
                       renderer='hip')
    if atlas is not None:
        env.set_render_atlas(atlas)
    env.set_tasks(targets.numpy(), starts.numpy(), init_pose=pose)
    obs = env.reset()
    assert obs['pov'].shape == (n, 64, 64, 3)
    if flying:
        for t in range(60):
            obs, _, _, _ = env.step(dict(movement=torch.as_tensor(rng.uniform(-1, 1, (n, 3)), dtype=torch.float32),
                                         camera=torch.as_tensor(rng.uniform(-5, 5, (n, 2)), dtype=torch.float32),
                                         inventory=torch.as_tensor(rng.randint(0, 7, n), dtype=torch.int32),
                                         placement=torch.as_tensor(rng.randint(0, 3, n), dtype=torch.int32)))
    else:
        acts = env.fill_actions(60, seed=seed)
        for t in range(60):
            obs, _, _, _ = env.step(acts[t])
    return env, obs


def test_walking_and_flying_batches_after_60_autoreset_steps_match_the_model():
    atlas = _ref_atlas()
    tally = Tally('stepped 256 walking + 256 flying')
    for flying in (False, True):
        env, obs = _stepped_batch(flying, seed=5 + flying, atlas=atlas)
        fr = obs['pov'].cpu().numpy()           # the frame step() returned: of the state after the step (auto-reset)
        poses, grids = _state(env)
        for k, res in enumerate(_models(poses, grids, 64, 64, atlas)):
            tally.add(fr[k], res, 3)
    tally.check()


def test_obs_pov_is_the_frame_of_the_current_state_and_is_reused():
    env, obs = _stepped_batch(False, seed=9)
    pov = obs['pov']
    again = env.render_pov()
    assert pov.data_ptr() == env.pov.data_ptr()
    assert np.array_equal(pov.cpu().numpy(), again.cpu().numpy())
    obs2, _, _, _ = env.step(env.fill_actions(1, seed=3)[0])
    assert obs2['pov'].data_ptr() == pov.data_ptr()
    assert np.array_equal(obs2['pov'].cpu().numpy(), env.render_pov().cpu().numpy())


def test_65536_envs_invariants_samples_out_reuse_streams_and_determinism():
    import torch
    from gridworld_amd import VecGridWorld, workloads
    n = 65536
    env = VecGridWorld(n)
    rng = np.random.RandomState(3)
    pose = np.stack([rng.uniform(-10, 10, n), rng.uniform(-1, 6, n), rng.uniform(-10, 10, n),
                     rng.uniform(-180, 180, n), rng.uniform(-90, 90, n)], 1)
    starts = workloads.uniform20(n, seed=4).numpy()
    env.set_tasks(starts, starts, init_pose=pose)
    env.reset()
    out = torch.empty((n, 64, 64, 3), dtype=torch.uint8, device='cuda')
    r1 = env.render_pov(out=out)
    assert r1 is out
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        r2 = env.render_pov()
    torch.cuda.current_stream().wait_stream(s)
    assert torch.equal(r1, r2)                                  # two renders bit-identical, on another stream too
    # sky and ground invariants over all frames: the clear colour only where no surface is; a level eye above the
    # ground with nothing above it sees sky in its top row and pixels from the atlas or sky elsewhere
    sky = torch.tensor(M.CLEAR[:3], device='cuda', dtype=torch.uint8)
    flat = torch.from_numpy(R.default_atlas()).cuda()
    palette = torch.unique(torch.cat([flat.reshape(-1, 4)[:, :3], sky[None]]), dim=0)
    colours = torch.unique(out.reshape(-1, 3)[::97], dim=0)
    assert all(bool((palette == c).all(1).any()) for c in colours)
    up = torch.from_numpy(pose[:, 4] > 50).cuda()                # looking steeply up from y <= 6 below the 7.5 ceiling
    top_row = out[:, 0].reshape(n, -1, 3)
    top_is_sky = (top_row == sky).all(-1).all(-1)
    # looking steeply down from |x|, |z| <= 4, y <= 4 the bottom row meets the ground within 5.5 of depth and 12 of
    # the centre (inside the 18.5 of the ground): never sky
    below = torch.from_numpy((pose[:, 4] < -50) & (np.abs(pose[:, 0]) <= 4) & (np.abs(pose[:, 2]) <= 4)
                             & (pose[:, 1] <= 4)).cuda()
    bottom_sky = (out[:, -1].reshape(n, -1, 3) == sky).all(-1).any(-1)
    assert int(below.sum()) > 1000 and not bool(bottom_sky[below].any())
    assert bool(top_is_sky[up].float().mean() > 0.2)
    # 64 sampled envs vs the model
    rows = rng.choice(n, 64, replace=False)
    poses, grids = _state(env, rows)
    fr = out[torch.from_numpy(rows).cuda()].cpu().numpy()
    tally = Tally('65,536-env batch, 64 sampled')
    for k, res in enumerate(_models(poses, grids, 64, 64, R.default_atlas())):
        tally.add(fr[k], res, 3)
    tally.check()
    with pytest.raises(ValueError):
        env.render_pov(out=out[:, :, :, :2])


def test_renderer_obs_through_a_sub_batch():
    import torch
    from gridworld_amd import VecGridWorld, workloads
    n = 512
    env = VecGridWorld(n, autoreset=True, max_steps=30, renderer='hip')
    tg = workloads.rt20(n, seed=2).numpy()
    rng = np.random.RandomState(2)
    pose = np.stack([rng.uniform(-5, 5, n), rng.uniform(0, 3, n), rng.uniform(-5, 5, n), rng.uniform(-180, 180, n),
                     rng.uniform(-40, 40, n)], 1)
    env.set_tasks(tg, tg, init_pose=pose)
    env.reset()
    acts = env.fill_actions(20, seed=4)
    subs = env.split(2)                 # the sub-batch streams wait for the work queued so far (the actions included)
    for t in range(20):
        for k, sb in enumerate(subs):
            sb.step_walking_ptr(acts[t, k * 256:(k + 1) * 256].contiguous())
    for sb in subs:
        sb.join()
        assert sb.obs()['pov'].shape == (256, 64, 64, 3)
    got = env.pov.cpu().numpy()
    whole = env.render_pov().cpu().numpy()
    assert np.array_equal(got, whole)
    sb_out = subs[1].render_pov(channels=4)
    subs[1].join()
    assert np.array_equal(sb_out.cpu().numpy()[..., :3], whole[256:])
    env._release_children(subs)


def test_facade_pov_and_render_match_the_model_and_default_still_raises():
    import gridworld_amd as G
    with pytest.raises(NotImplementedError):
        G.make('IGLUGridworld-v0')
    env = G.make('IGLUGridworld-v0', renderer='hip')
    env.set_render_atlas(_ref_atlas())
    tg = np.zeros((9, 11, 11), np.int32)
    tg[0, 3:7, 2] = 1
    tg[1, 4, 2] = 5
    env.set_task(G.Task('chat', tg, starting_grid=[(-1, 0, -3, 3), (0, 0, -3, 4), (1, 0, -3, 6)]))
    obs = env.reset()
    assert obs['pov'].shape == (64, 64, 3) and obs['pov'].dtype == np.uint8
    tally = Tally('facade')
    for t in range(12):
        rgba = env.render()
        assert rgba.shape == (64, 64, 4) and rgba.dtype == np.uint8
        assert np.array_equal(rgba[..., :3], obs['pov'])
        u = env.unwrapped
        pose = (*u.agent.position, *u.agent.rotation)
        res = M.render(pose, u.grid, _ref_atlas(), 64, 64, 4)
        tally.add(rgba, res, 4)
        tally.add(obs['pov'], res, 3)
        obs, _, _, _ = env.step(t % 18)
    tally.check()
    fake = G.make('IGLUGridworld-v0', renderer='hip', fake=True)
    fake.set_task(G.Task('chat', tg))
    assert fake.reset()['pov'].shape == (64, 64, 3)
