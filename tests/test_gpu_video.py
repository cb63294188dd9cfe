"""Video on top of the encoder: EpisodeLogger(pov_codec='jpeg'), save_video, Visualizer.render_video and the facade's
Logged.  The checks are on encoder input equality: the logged streams are the encode_jpeg bytes of exactly the frames
the raw path logs (tests/test_gpu_jpeg.py holds encode_jpeg to the model).  Small batches: a few seconds together."""
import glob

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _logged_run(**kw):
    import torch
    from gridworld_amd import VecGridWorld, workloads
    from gridworld_amd.wrappers import EpisodeLogger
    n = 8
    env = VecGridWorld(n, device='cuda:0', autoreset=True, size_reward=False, max_steps=12)
    env.set_tasks(workloads.rt20(n, seed=3).numpy())
    log = EpisodeLogger(env, n_envs=4, pov=True, **kw)
    env.reset()
    acts = env.fill_actions(30, seed=7)
    for t in range(30):
        env.step(acts[t])
    torch.cuda.synchronize()
    return env, log, log.collect(dump=False)


def test_logger_streams_are_the_encoded_raw_frames_and_save_video_holds_them(tmp_path):
    import torch
    import gridworld_amd as G
    _, _, raw = _logged_run()
    env, log, eps = _logged_run(pov_codec='jpeg', pov_quality=85)
    assert len(eps) == len(raw) >= 4
    for ep, ref in zip(eps, raw):
        assert (ep['env'], ep['episode']) == (ref['env'], ref['episode'])
        assert 'pov' not in ep and len(ep['pov_jpeg']) == len(ref['pov']) == len(ep['reward']) + 1
        want = G.jpeg_bytes(*G.encode_jpeg(torch.from_numpy(ref['pov']).cuda(), 85))
        assert ep['pov_jpeg'] == want
        assert all(j[:2] == b'\xff\xd8' and j[-2:] == b'\xff\xd9' for j in want)
    # the video of a compressed episode holds its streams; of a raw one, the streams of its frames
    p = log.save_video(eps[0], str(tmp_path / 'ep.avi'), fps=20)
    frames, meta = G.codec.read_avi(p, info=True)
    assert frames == eps[0]['pov_jpeg'] and meta == dict(frames=len(frames), size=(64, 64), fps=20.0)
    log.pov_quality = 85
    assert G.codec.read_avi(log.save_video(raw[0], str(tmp_path / 'raw.avi'))) == eps[0]['pov_jpeg']
    # dumped, the streams travel in the npz
    log.set_path(str(tmp_path))
    log._dumped.clear()
    again = log.collect(dump=True)
    z = np.load(again[0]['file'])
    ends = [0] + z['pov_jpeg_end'].tolist()
    assert [z['pov_jpeg'][a:b].tobytes() for a, b in zip(ends[:-1], ends[1:])] == again[0]['pov_jpeg']
    with pytest.raises(ValueError):
        _logged_run(pov_codec='h264')


def test_visualizer_render_video_is_render_batch_encoded(tmp_path):
    import torch
    import gridworld_amd as G
    vis = G.Visualizer(render_size=(96, 64))
    vis.set_world_state([(0, 0, 0, 1), (0, 1, 0, 3), (1, 0, 0, 5), (-2, 0, 2, 6)])
    pos, rot = G.visualizer.split_poses(G.orbit_poses((0, 1, 0), 7, 4, 12))
    path = vis.render_video(str(tmp_path / 'orbit'), pos, rot, fps=30, quality=70)
    assert path == str(tmp_path / 'orbit') + '.avi'
    frames, meta = G.codec.read_avi(path, info=True)
    assert meta == dict(frames=12, size=(96, 64), fps=30.0)
    batch = vis.render_batch(pos, rot)
    assert frames == G.jpeg_bytes(*G.encode_jpeg(torch.from_numpy(batch).cuda(), 70))
    # pairs of pose and block list
    blocks = [[(0, 1, 0, 1 + k % 6), (k % 3, 1, 1, 2)] for k in range(12)]
    path = vis.render_video(str(tmp_path / 'pairs'), pos, rot, blocks=blocks)
    batch = vis.render_batch(pos, rot, blocks=blocks)
    assert G.codec.read_avi(path) == G.jpeg_bytes(*G.encode_jpeg(torch.from_numpy(batch).cuda(), 90))


def test_facade_logged_writes_one_avi_per_episode_beside_the_npz(tmp_path):
    import torch
    import gridworld_amd as G
    from gridworld_amd.wrappers import Logged
    env = Logged(G.make('IGLUGridworld-v0', render=True, renderer='hip', max_steps=9))
    env.turn_on()
    env.set_path(str(tmp_path))
    tg = np.zeros((9, 11, 11), np.int32)
    tg[0, 3:7, 2] = 1
    env.set_task(G.Task('chat', tg, starting_grid=[(-1, 0, -3, 3), (0, 0, -3, 4)]))
    for episode in range(2):
        env.reset()
        done, t = False, 0
        while not done:
            _, _, done, _ = env.step((t * 5 + episode) % 18)
            t += 1
    npz = sorted(glob.glob(str(tmp_path / '**' / '*.npz'), recursive=True))
    avi = sorted(glob.glob(str(tmp_path / '**' / '*.avi'), recursive=True))
    assert len(npz) == len(avi) == 2 and [f[:-4] for f in npz] == [f[:-4] for f in avi]
    for a, b in zip(npz, avi):
        pov = np.load(a)['pov']
        frames, meta = G.codec.read_avi(b, info=True)
        assert len(frames) == len(pov) == 10 and meta['size'] == (64, 64) and meta['fps'] == 20.0
        assert frames == G.jpeg_bytes(*G.encode_jpeg(torch.from_numpy(pov).cuda(), 90))
    # with logging off nothing is written
    off = Logged(G.make('IGLUGridworld-v0', render=True, renderer='hip', max_steps=3))
    off.set_path(str(tmp_path / 'off'))
    off.set_task(G.Task('chat', tg))
    off.reset()
    for t in range(3):
        off.step(0)
    assert not glob.glob(str(tmp_path / 'off' / '**' / '*.avi'), recursive=True)
