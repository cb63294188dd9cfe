"""Frames of logged episodes (igw_render_episodes, EpisodeLogger(pov=True), the facade's Logged) against the live
renderer, against igw_render_pov on the decoded log, and against the brute-force model tests/pov_model.py.
"Outside the band" as in tests/test_gpu_render.py: pixels whose model margins are >= 1e-3 texel and >= 1e-4 world
units; each comparison prints its mismatch counts.  All of these together are budgeted at <= 60 s."""
import glob
import os

import numpy as np
import pytest

import pov_model as M
from gridworld_amd import render as R
from render_checks import Tally, _models, _ref_atlas

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SPACES = ('walking', 'flying', 'walking_dict')


def _tasks(n, seed):
    """Targets, starting grids and init poses of n rows: every third row has a starting grid, every row a random
    init pose (row 1's is rejected by _env)."""
    from gridworld_amd import workloads
    targets = workloads.rt20(n, seed=seed).numpy()
    starts = np.zeros_like(targets)
    rng = np.random.RandomState(seed)
    for k in range(0, n, 3):
        for _ in range(6):
            starts[k, rng.randint(0, 3), rng.randint(0, 11), rng.randint(0, 11)] = rng.randint(1, 7)
    pose = np.stack([rng.uniform(-4, 4, n), rng.uniform(0, 3, n), rng.uniform(-4, 4, n), rng.uniform(-180, 180, n),
                     rng.uniform(-40, 40, n)], 1)
    return targets, starts, pose


def _env(space, n, max_steps, autoreset, seed=1, **kw):
    from gridworld_amd import VecGridWorld
    env = VecGridWorld(n, autoreset=autoreset, max_steps=max_steps, action_space='flying' if space == 'flying' else
                       'walking', discretize=space != 'walking_dict', **kw)
    env.set_render_atlas(_ref_atlas())
    targets, starts, pose = _tasks(n, seed)
    env.set_tasks(targets, starts, init_pose=pose)
    # row 1 again through the C ABI with an init pose outside the accepted range (set_tasks refuses it): the kernel
    # replaces it by the default pose and counts it (stats()['bad_poses'])
    import torch
    row = torch.zeros((1, 1104), dtype=torch.int8, device=env.device)
    row[0, :1089] = torch.from_numpy(targets[1].reshape(-1).astype(np.int8))
    bad = torch.tensor([[50.0, 0.0, 0.0, 10.0, 0.0]], dtype=torch.float64, device=env.device)
    assert env.lib.igw_prepare_tasks(env.ctx, 1, 1, row.data_ptr(), None, None, None, bad.data_ptr(),
                                     env._stream()) == 0
    torch.cuda.synchronize()
    return env


def _actions(space, n, T, seed):
    import torch
    rng = np.random.RandomState(seed)
    dev = 'cuda'
    out = []
    for _ in range(T):
        if space == 'walking':
            out.append(torch.as_tensor(rng.randint(0, 18, n), dtype=torch.int32, device=dev))
        elif space == 'flying':
            out.append(dict(movement=torch.as_tensor(rng.uniform(-1, 1, (n, 3)), dtype=torch.float32, device=dev),
                            camera=torch.as_tensor(rng.uniform(-5, 5, (n, 2)), dtype=torch.float32, device=dev),
                            inventory=torch.as_tensor(rng.randint(0, 7, n), dtype=torch.int32, device=dev),
                            placement=torch.as_tensor(rng.randint(0, 3, n), dtype=torch.int32, device=dev)))
        else:
            b = rng.randint(0, 2, (n, 8))
            b[:, 7] = rng.randint(0, 7, n)
            out.append(dict(buttons=torch.as_tensor(b, dtype=torch.uint8, device=dev),
                            camera=torch.as_tensor(rng.uniform(-5, 5, (n, 2)), dtype=torch.float32, device=dev)))
    return out


def _run(space, n=16, n_log=8, max_steps=16, T=40, autoreset=True, capacity=None, live=False):
    """Steps a batch with EpisodeLogger(pov=True); returns (env, logger, episodes, frame after reset, live frames
    [T][n_log] after every step when live=True)."""
    import torch
    from gridworld_amd.wrappers import EpisodeLogger
    env = _env(space, n, max_steps, autoreset)
    log = EpisodeLogger(env, n_envs=n_log, capacity=capacity, pov=True)
    env.reset()
    pov0 = env.render_pov()[:n_log].cpu().numpy()
    frames = []
    for a in _actions(space, n, T, seed=3):
        env.step(a)
        if live:
            frames.append(env.render_pov()[:n_log].clone())
        if not autoreset and bool(env.done[:n_log].all()):
            break
    torch.cuda.synchronize()
    eps = log.collect(dump=False)
    return env, log, eps, pov0, [f.cpu().numpy() for f in frames]


def _occ(grid):
    """include/igw.h occupancy bitmap of one [9, 11, 11] grid: 48 uint32 words."""
    bits = np.zeros(48 * 32, np.uint8)
    y, x, z = np.nonzero(grid)
    bits[y * 169 + (x + 1) * 13 + (z + 1)] = 1
    return np.packbits(bits.reshape(-1, 32)[:, ::-1], axis=1).view('>u4').astype(np.uint32).reshape(48)


def _pov_of(grids, poses, atlas):
    """igw_render_pov on agent records holding `poses` (x, y, z, yaw, pitch f64) over `grids`: uint8 [n, 64, 64, 3]."""
    import torch
    n = len(grids)
    agent = np.zeros((n, 64), np.uint8)
    agent[:, :40] = np.ascontiguousarray(poses, np.float64).view(np.uint8).reshape(n, 40)
    g = np.zeros((n, 1104), np.int8)
    g[:, :1089] = np.asarray(grids).reshape(n, -1)
    occ = np.stack([_occ(x) for x in np.asarray(grids)])
    a, gd, od = (torch.from_numpy(x).cuda() for x in (agent, g, occ))
    out = torch.empty((n, 64, 64, 3), dtype=torch.uint8, device='cuda')
    R.render_into(a.data_ptr(), gd.data_ptr(), od.data_ptr(), n, torch.from_numpy(atlas).cuda(), out.data_ptr(), 64,
                  64, 3, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _log_poses(ep):
    """The f64 poses of entries 1..T: the logged f32 agentPos (x, y, z, pitch, yaw) widened, yaw / pitch swapped."""
    ap = ep['agentPos'][1:].astype(np.float64)
    return np.stack([ap[:, 0], ap[:, 1], ap[:, 2], ap[:, 4], ap[:, 3]], 1)


@pytest.mark.parametrize('space', SPACES)
def test_log_frames_entry0_exact_entries_exact_and_against_the_model(space):
    atlas = _ref_atlas()
    env, log, eps, pov0, _ = _run(space)
    assert env.stats()['bad_poses'] >= 1
    assert len(eps) >= 8 and {e['env'] for e in eps} == set(range(8))
    tally = Tally(f'log frames vs model ({space})')
    for ep in eps:
        T = len(ep['reward'])
        assert ep['pov'].shape == (T + 1, 64, 64, 3) and ep['pov'].dtype == np.uint8
        # entry 0: the frame render_pov drew right after the explicit reset (every episode of an env starts from its
        # own task row here: no task sampling)
        assert np.array_equal(ep['pov'][0], pov0[ep['env']]), ep['env']
        # entries t >= 1: igw_render_pov on the decoded f32 pose and grid[t], bit for bit
        poses = _log_poses(ep)
        assert np.array_equal(ep['pov'][1:], _pov_of(ep['grid'][1:], poses, atlas))
        # and the model on (grid[t], f32 pose), every third entry
        ks = list(range(1, T + 1, 3))
        for k, res in zip(ks, _models(poses[[k - 1 for k in ks]], ep['grid'][ks].astype(np.int8), 64, 64, atlas)):
            tally.add(ep['pov'][k], res, 3)
    tally.check()


def test_log_frames_follow_the_live_frames_and_keep_the_terminal_state_of_an_autoreset():
    atlas = _ref_atlas()
    # without autoreset every step's live frame shows the logged state, the terminal step included
    env, log, eps, pov0, live = _run('walking', max_steps=16, T=16, autoreset=False, live=True)
    assert len(eps) == 8 and all(len(e['reward']) == 16 and e['done'][-1] for e in eps)
    tally = Tally('log frames vs live frames (no autoreset)')
    for ep in eps:
        e = ep['env']
        ks = list(range(1, 17, 2)) + [16]
        for k, res in zip(ks, _models(_log_poses(ep)[[k - 1 for k in ks]], ep['grid'][ks].astype(np.int8), 64, 64,
                                      atlas)):
            tally.add(live[k - 1][e], res, 3)         # the live frame (f64 pose) against the model of the log's state
            tally.add(ep['pov'][k], res, 3)
        assert np.array_equal(ep['pov'][0], pov0[e])
    tally.check()
    terminal = {e['env']: e['pov'][-1] for e in eps}
    # with autoreset the live frame after the last step already shows the new episode; the log keeps the terminal
    # state, the same bytes as the run without autoreset
    env2, log2, eps2, _, live2 = _run('walking', max_steps=16, T=16, autoreset=True, live=True)
    assert len(eps2) == 8
    for ep in eps2:
        assert np.array_equal(ep['pov'][-1], terminal[ep['env']])
        assert not np.array_equal(ep['pov'][-1], live2[15][ep['env']])
        assert np.array_equal(live2[15][ep['env']], ep['pov'][0])   # the new episode starts from the same row


def test_truncation_to_the_capacity_and_packing_without_gaps_or_overlap():
    import torch
    atlas = _ref_atlas()
    env, log, eps, _, _ = _run('flying', max_steps=20, T=40, capacity=7)
    assert eps and all(e['pov'].shape[0] == 8 and len(e['reward']) == 7 for e in eps)
    for ep in eps[:4]:
        assert np.array_equal(ep['pov'][1:], _pov_of(ep['grid'][1:], _log_poses(ep), atlas))
    # direct call: episodes of different lengths at frame offsets with gaps, into a sentinel-filled buffer; length 0,
    # a length beyond max_length (clamped) and an episode outside the record buffer (not drawn)
    cap = log.records.shape[2]
    n_rec = log.records.shape[0] * 2 * cap
    ep_rows = [(0, 0, 7), (1, 1, 3), (2, 0, 0), (3, 1, 99), (4, 0, 5)]
    first = [(e * 2 + s) * cap for e, s, _ in ep_rows[:4]] + [n_rec - 2]          # the last one overruns: skipped
    length = [ln for _, _, ln in ep_rows]
    frame0 = [2, 12, 17, 19, 30]
    n_frames = 40
    out = torch.full((n_frames, 64, 64, 3), 0xA5, dtype=torch.uint8, device='cuda')
    heads = log.heads.cpu().numpy()
    tasks = [int(heads[e, s, 0]) for e, s, _ in ep_rows]
    rows = torch.tensor(tasks, device='cuda')
    start = env.task_start.index_select(0, rows)
    pose = env.task_meta.index_select(0, rows)[:, :40].contiguous().view(torch.float64)
    dv = lambda x, dt: torch.tensor(x, dtype=dt, device='cuda')  # noqa: E731
    f, ln, f0 = dv(first, torch.int64), dv(length, torch.int32), dv(frame0, torch.int64)
    R.render_episodes_into(log.records.data_ptr(), n_rec, f.data_ptr(), ln.data_ptr(), f0.data_ptr(),
                           start.data_ptr(), pose.data_ptr(), len(ep_rows), cap, torch.from_numpy(atlas).cuda(),
                           out.data_ptr(), n_frames, 64, 64, 3, torch.cuda.current_stream().cuda_stream)
    got = out.cpu().numpy()
    written = set()
    for i, ((e, s, _), fr0, n) in enumerate(zip(ep_rows[:4], frame0, [7, 3, 0, cap])):
        written |= set(range(fr0, fr0 + n + 1))
        rec = log.records[e, s, :n].cpu().numpy()
        ap = rec[:, :20].copy().view(np.float32).astype(np.float64)
        poses = np.stack([ap[:, 0], ap[:, 1], ap[:, 2], ap[:, 4], ap[:, 3]], 1)
        grid = env.task_start[tasks[i], :1089].cpu().numpy().reshape(9, 11, 11)
        grids = [grid.copy()]
        ch = rec[:, 40:42].copy().view(np.uint16)[:, 0]
        for c in ch:
            g = grids[-1].copy()
            if c != 0xffff:
                g.reshape(-1)[c & 0x7ff] = (c >> 11) & 7
            grids.append(g)
        if n:
            assert np.array_equal(got[fr0 + 1:fr0 + n + 1], _pov_of(np.stack(grids[1:]), poses, atlas))
        assert not (got[fr0] == 0xA5).all()
    untouched = [k for k in range(n_frames) if k not in written]
    assert (got[untouched] == 0xA5).all()
    assert len(written) == 8 + 4 + 1 + cap + 1


def test_graph_replayed_episodes_give_the_frames_of_eager_steps():
    import torch
    from gridworld_amd.wrappers import EpisodeLogger
    n, T = 16, 30
    acts = torch.stack(_actions('walking', n, T, seed=8))
    res = []
    for graph in (False, True):
        env = _env('walking', n, 12, True)
        log = EpisodeLogger(env, n_envs=8, pov=True)
        env.reset()
        if graph:
            g = env.capture_steps(acts)
            g.replay()
        else:
            for t in range(T):
                env.step(acts[t])
        torch.cuda.synchronize()
        res.append({(e['env'], e['episode']): e['pov'] for e in log.collect(dump=False)})
    assert res[0].keys() == res[1].keys() and len(res[0]) >= 8
    for k in res[0]:
        assert np.array_equal(res[0][k], res[1][k]), k


def test_facade_logged_writes_one_rgb_frame_per_entry(tmp_path):
    import gridworld_amd as G
    from gridworld_amd.wrappers import Logged
    atlas = _ref_atlas()
    env = Logged(G.make('IGLUGridworld-v0', render=True, renderer='hip', max_steps=14))
    env.set_render_atlas(atlas)
    env.turn_on()
    env.set_path(str(tmp_path))
    tg = np.zeros((9, 11, 11), np.int32)
    tg[0, 3:7, 2] = 1
    env.set_task(G.Task('chat', tg, starting_grid=[(-1, 0, -3, 3), (0, 0, -3, 4)]))
    obs = env.reset()
    u = env.unwrapped
    seen, states = [obs['pov']], [((*u.agent.position, *u.agent.rotation), u.grid.copy())]
    done, t = False, 0
    while not done:
        obs, _, done, _ = env.step((t * 7) % 18)
        seen.append(obs['pov'])
        states.append(((*u.agent.position, *u.agent.rotation), u.grid.copy()))
        t += 1
    files = glob.glob(str(tmp_path / '**' / '*.npz'), recursive=True)
    assert len(files) == 1
    z = np.load(files[0])
    assert z['pov'].shape == (t + 1, 64, 64, 3) and z['pov'].dtype == np.uint8 and t == 14
    assert np.array_equal(z['pov'][0], seen[0])
    tally = Tally('facade Logged pov vs obs pov')
    for k, (pose, grid) in enumerate(states):
        res = M.render(pose, grid.astype(np.int8), atlas, 64, 64, 4)
        tally.add(z['pov'][k], res, 3)
        tally.add(seen[k], res, 3)
    tally.check()
    # the vector facade logs no frames
    v = Logged(G.make('IGLUGridworldVector-v0', max_steps=5))
    assert v._log.pov is False
