"""Wrappers of the reference that sit on the step path (gridworld/wrappers.py)."""
import os
import uuid

import numpy as np
import torch

from . import _lib as L
from . import codec as K
from . import relabel as RL
from . import render as R
from . import spaces
from .env import Wrapper  # noqa: F401  (gridworld/env.py:306-314; re-exported: the reference imports gym.Wrapper here)


class Actions(Wrapper):
    """Discrete(17) action set without `place` (gridworld/wrappers.py:11-32): new index -> Discrete(18) index.
    With select_and_place the hotbar actions place blocks, so index 17 (use) is redundant."""

    def __init__(self, env):
        super().__init__(env)
        self.action_map = list(range(17))  # 0 noop, 1-4 move, 5 jump, 6-11 hotbar, 12-15 camera, 16 break
        self.action_space = spaces.Discrete(len(self.action_map))

    def step(self, action):
        return self.env.step(self.action_map[action])


class EpisodeLogger:
    """Per-episode npz dumps of what the reference's `Logged` wrapper collects (gridworld/wrappers.py:66-134:
    every observation key stacked over reset + steps, `reward`, `done`, the actions as csv; no video), taken
    from the trajectory log the step kernels keep on the device (VecGridWorld.enable_trajectory_log,
    include/igw.h: igw_set_trajectory_log) -- the env loop itself never copies observations to the host.

        log = EpisodeLogger(vec_env, n_envs=4, path='episodes')
        ... step / reset as usual ...; files = log.collect()      # any time; dumps the episodes that finished

    Arrays per file (T = steps of the episode): agentPos f32[T+1,5], inventory f32[T+1,6], compass f32[T+1,1],
    grid int32[T+1,9,11,11] (rebuilt from the starting grid and the logged one-cell changes), reward f64[T],
    done bool[T], plus `task` (row of the task table), `env`, `episode`.  Entry 0 is the reset observation.

    `actions` are the actions AS EXECUTED, not the raw inputs the reference's Logged appends (wrappers.py:98): the
    device record packs a flying action's inventory into 3 bits and its placement into 2 (include/igw.h), so an
    inventory id the kernel rejected (outside 0..6: run as 0 and counted in stats()['bad_actions']) is logged as 0 and
    a placement other than 1 / 2 as 0.  Replaying a log therefore reproduces the trajectory, not the bad-action
    counts; Discrete(18) ids, movement / camera floats and Dict buttons are logged raw.

    pov=True adds `pov` uint8 [T+1, H, W, 3] (W, H = vec.render_size, RGB, the env's atlas): the first-person frame of
    every entry, drawn on the device by ONE igw_render_episodes launch per collect() for all the episodes it returns
    (include/igw_render.h).  Entry 0 is the reset state seen from the task row's f64 init pose; entry t >= 1 is grid[t]
    seen from agentPos[t], the f32 pose the log holds ("First-person frames").  The last entry of an
    episode that ended in an auto-reset is its terminal state, which render_pov() can no longer show.  Like `grid`,
    the frames read the episode's task row (starting grid, init pose): a set_tasks that rewrites that row between the
    episode and collect() changes them.  pov_outputs (with pov=True; default ('rgb',)) names what that launch writes,
    as for VecGridWorld: 'rgb' is `pov`; 'depth' f32, 'label' u8 and 'surface' i16 add arrays of those names,
    [T+1, H, W] each (include/igw_render.h: igw_render_aux), from the one igw_render_episodes_aux launch.

    pov_codec='jpeg' (with pov=True) keeps the frames compressed: an episode carries `pov_jpeg`, a list of T+1 byte
    strings, in place of the raw `pov` array -- the JPEG streams (quality pov_quality) of exactly
    the frames the raw path logs, encoded on the device by ONE igw_jpeg_encode launch behind the render launch; only
    the streams cross to the host.  The npz holds them as `pov_jpeg` (uint8, the streams end to end) and
    `pov_jpeg_end` (int64 [T+1], where each ends).  save_video(episode, path) writes them as a Motion-JPEG AVI."""

    def __init__(self, vec, n_envs=1, path='episodes', desc='', glob_step=0, capacity=None, pov=False,
                 pov_outputs=('rgb',), pov_codec=None, pov_quality=90):
        self.vec, self.path, self.desc, self.glob_step = vec, path, desc, glob_step
        self.pov = bool(pov)
        self.pov_outputs = R.check_outputs(pov_outputs)
        self.pov_codec, self.pov_quality = K.check_codec(pov_codec), int(pov_quality)
        if self.pov_codec and 'rgb' not in self.pov_outputs:
            raise ValueError("pov_codec='jpeg' encodes the colour frame: pov_outputs must hold 'rgb'")
        if not 1 <= self.pov_quality <= 100:
            raise ValueError(f'pov_quality must be in 1..100, got {pov_quality}')
        self.records, self.heads = vec.enable_trajectory_log(n_envs, capacity)
        self.n_envs = int(n_envs)
        self._dumped = {}  # env -> last episode number written
        self.episodes = []  # the dicts that were dumped (also returned by collect)

    def set_path(self, path):
        self.path = path

    def set_desc(self, desc, glob_step):
        self.desc, self.glob_step = desc, glob_step

    def _decode(self, env, slot, task, length):
        v = self.vec
        raw = self.records[env, slot, :length].cpu().numpy()   # record layout: include/igw.h (igw_set_trajectory_log)
        f32 = raw[:, :28].copy().view(np.float32).reshape(length, 7)
        inv = raw[:, 28:40].copy().view(np.int16).reshape(length, 6)
        change = raw[:, 40:42].copy().view(np.uint16)[:, 0].astype(np.int64)
        tag = raw[:, 43].astype(np.int64)
        meta = v.task_meta[task].cpu().numpy()
        inv0 = meta[64:76].view(np.int16).astype(np.float32)
        grid0 = v.task_start[task, :L.CELLS].cpu().numpy().astype(np.int32).reshape(9, 11, 11)
        grids = np.empty((length + 1, 9, 11, 11), np.int32)
        grids[0] = grid0
        for t in range(length):
            grids[t + 1] = grids[t]
            if change[t] != 0xffff:
                grids[t + 1].reshape(-1)[change[t] & 0x7ff] = (change[t] >> 11) & 7
        space = int(tag[0] & 3) if length else 0
        if space == 0:
            actions = raw[:, 44:48].copy().view(np.int32)[:, 0]
        elif space == 1:
            actions = {'movement': raw[:, 44:56].copy().view(np.float32).reshape(length, 3),
                       'camera': raw[:, 56:64].copy().view(np.float32).reshape(length, 2),
                       'inventory': ((tag >> 2) & 7).astype(np.int32), 'placement': ((tag >> 5) & 3).astype(np.int32)}
        else:
            actions = {'buttons': raw[:, 44:52].copy(), 'camera': raw[:, 52:60].copy().view(np.float32).reshape(length, 2)}
        zeros = np.zeros((1, 5), np.float32)
        return {'agentPos': np.concatenate([zeros, f32[:, :5]]),
                'inventory': np.concatenate([inv0[None], inv.astype(np.float32)]),
                'compass': np.concatenate([np.zeros((1, 1), np.float32), f32[:, 6:7]]),
                'grid': grids, 'reward': f32[:, 5].astype(np.float64), 'done': raw[:, 42].astype(bool),
                'actions': actions, 'task': int(task)}

    def _render(self, todo):
        """pov frames (and planes) of the episodes (env, slot, task, length, episode) in one igw_render_episodes (or
        _aux) launch on the env's stream: a list of dicts array name -> [length + 1, H, W, ...] array."""
        v = self.vec
        if not todo:
            return []
        dev, cap = v.device, self.records.shape[2]
        env, slot, task, length = (np.array([t[i] for t in todo], np.int64) for i in range(4))
        frame0 = np.concatenate([[0], np.cumsum(length + 1)])
        rows = torch.from_numpy(task).to(dev)
        first = torch.from_numpy((env * 2 + slot) * cap).to(dev)
        length_d = torch.from_numpy(length.astype(np.int32)).to(dev)
        frame0_d = torch.from_numpy(frame0[:-1].copy()).to(dev)
        start = v.task_start.index_select(0, rows)                                     # [m, 1104] i8
        pose = v.task_meta.index_select(0, rows)[:, :40].contiguous().view(torch.float64)   # [m, 5] x, y, z, yaw, pitch
        args = (self.records.data_ptr(), self.records.shape[0] * 2 * cap, first.data_ptr(), length_d.data_ptr(),
                frame0_d.data_ptr(), start.data_ptr(), pose.data_ptr(), len(todo), cap)
        # as for VecGridWorld, the default ('rgb',) is the plain entry
        outputs = None if self.pov_outputs == ('rgb',) else self.pov_outputs
        res = R.launch('episodes', args, int(frame0[-1]), v.render_size, 3, outputs, None, v._atlas(), dev, v._stream())
        if outputs is None:
            res = {'rgb': res}
        jpegs = None
        if self.pov_codec:   # (on v._stream(), the current one)
            jpegs = K.jpeg_bytes(*K.encoded(self.pov_codec, None, self.pov_quality, None, lambda: res.pop('rgb')))
        host = {'pov' if k == 'rgb' else k: t.cpu().numpy() for k, t in res.items()}
        eps = [{k: h[frame0[i]:frame0[i + 1]] for k, h in host.items()} for i in range(len(todo))]
        if jpegs is not None:
            for i, ep in enumerate(eps):
                ep['pov_jpeg'] = jpegs[frame0[i]:frame0[i + 1]]
        return eps

    def save_video(self, episode, path, fps=20):
        """Writes an episode's frames (a dict collect() returned) as a Motion-JPEG AVI at `path`: its `pov_jpeg` streams
        as they are, or its raw `pov` frames encoded first (one igw_jpeg_encode launch at pov_quality).  Returns the
        path."""
        jpegs = episode.get('pov_jpeg')
        if jpegs is None:
            if 'pov' not in episode:
                raise ValueError('the episode has no frames: log with EpisodeLogger(pov=True)')
            jpegs = K.jpeg_bytes(*K.encode_jpeg(torch.from_numpy(np.ascontiguousarray(episode['pov']))
                                                .to(self.vec.device), self.pov_quality))
        return K.write_avi(path, jpegs, self.vec.render_size, fps)

    def relabel(self, episodes=None, goals='final', gamma=1.0, outputs=RL.DEFAULT):
        """Hindsight rewards of collected episodes (VecGridWorld.relabel): one igw_relabel launch for
        `episodes` (dicts collect() returned; default: all of them) under G goals each.  `goals`: 'final' (the grid the
        episode ended with), 'own' (its task row's target as the task table holds it now), integer entries [G] or [E, G]
        of the episode itself, or targets [E, G, 9, 11, 11].  The change words are rebuilt from each dict's `grid`
        sequence, so an episode whose slot of the device log was overwritten since still answers.  Every dict gains
        `<output>_relabel` for the outputs named -- reward, done, progress as [G, T] (T the episode's steps), end, ret,
        target_size as [G], target as [G, 9, 11, 11] -- and the list is returned."""
        v = self.vec
        eps = list(self.episodes if episodes is None else episodes)
        names = RL.check_outputs(outputs)
        if v.cfg.size_reward:
            raise ValueError('relabel predicts the reward of the env itself; with size_reward=True the step returns '
                             "SizeReward's (make the env with size_reward=False)")
        if not eps:
            return eps
        dev = v.device
        length = np.array([len(ep['reward']) for ep in eps], np.int64)
        first = np.concatenate([[0], np.cumsum(length)])
        rec = np.zeros((max(int(first[-1]), 1), L.TRAJ_BYTES), np.uint8)
        for i, ep in enumerate(eps):
            g = np.asarray(ep['grid']).reshape(len(ep['grid']), -1)
            diff = g[1:] != g[:-1]
            cell = diff.argmax(1)
            word = np.where(diff.any(1), cell | g[1:][np.arange(len(cell)), cell].astype(np.int64) << 11, 0xffff)
            rec[first[i]:first[i + 1], 40:42] = word.astype(np.uint16).view(np.uint8).reshape(-1, 2)
        starts = np.stack([np.asarray(ep['grid'][0]).reshape(-1) for ep in eps]).astype(np.int8)
        kw = {}
        if isinstance(goals, str) and goals == 'final':
            kw['at'] = length[:, None]
        elif isinstance(goals, str) and goals == 'own':
            rows = torch.as_tensor([ep['task'] for ep in eps], device=dev)
            kw['targets'] = (v.task_target.index_select(0, rows) + v.task_start.index_select(0, rows))[:, None, :]
        elif isinstance(goals, str):
            raise ValueError(f"relabel: goals is 'final', 'own', entries or targets, got {goals!r}")
        else:
            g = np.asarray(goals.cpu() if torch.is_tensor(goals) else goals)
            if g.ndim == 1:
                g = np.broadcast_to(g, (len(eps), len(g)))
            kw['at' if g.ndim == 2 else 'targets'] = np.ascontiguousarray(g)
        res = RL.relabel(torch.from_numpy(rec).to(dev), first[:-1], length, starts, right_scale=v.cfg.right_placement_scale,
                         wrong_scale=v.cfg.wrong_placement_scale, max_steps=v.cfg.max_steps, gamma=gamma, outputs=names,
                         pad=max(int(length.max()), 1), **kw)
        host = {k: t.cpu().numpy() for k, t in res.items()}
        for i, ep in enumerate(eps):
            for k, h in host.items():
                ep[k + '_relabel'] = h[i, :, :length[i]] if k in ('reward', 'done', 'progress') else h[i]
        return eps

    def collect(self, dump=True):
        """Decodes (and with dump=True writes) every logged episode that finished since the last call."""
        torch.cuda.synchronize(self.vec.device)
        heads = self.heads.cpu().numpy()
        todo = []
        for env in range(self.n_envs):
            for slot in (0, 1):
                task, length, episode, finished = (int(x) for x in heads[env, slot])
                if not finished or length == 0 or self._dumped.get(env, -1) >= episode:
                    continue
                todo.append((env, slot, task, length, episode))
                self._dumped[env] = max(self._dumped.get(env, -1), episode)
        frames = self._render(todo) if self.pov else None
        out = []
        for i, (env, slot, task, length, episode) in enumerate(todo):
            ep = self._decode(env, slot, task, length)
            ep.update(env=env, episode=episode)
            if frames is not None:
                ep.update(frames[i])
            if dump:
                d = f'{self.path}/step{self.glob_step}'
                os.makedirs(d, exist_ok=True)
                fname = f'{d}/ep_{self.desc}_{uuid.uuid4().hex[:6]}'
                arrays = {k: v for k, v in ep.items() if k not in ('actions', 'pov_jpeg')}
                if 'pov_jpeg' in ep:
                    arrays['pov_jpeg'] = np.frombuffer(b''.join(ep['pov_jpeg']), np.uint8)
                    arrays['pov_jpeg_end'] = np.cumsum([len(j) for j in ep['pov_jpeg']], dtype=np.int64)
                if isinstance(ep['actions'], dict):
                    arrays.update({'action_' + k: v for k, v in ep['actions'].items()})
                np.savez_compressed(fname + '.npz', **arrays)
                if not isinstance(ep['actions'], dict):
                    with open(fname + '.csv', 'w') as f:
                        for a in ep['actions']:
                            f.write(f'{int(a)}\n')
                ep['file'] = fname + '.npz'
            out.append(ep)
        self.episodes.extend(out)
        return out


class Logged(Wrapper):
    """The reference's Logged wrapper for the 1-env facade (gridworld/wrappers.py:66-134): turn_on() / set_path() /
    set_desc(); an episode is written when it ends while logging is on.  When the env draws frames (render=True,
    renderer='hip', not fake) the npz holds `pov` uint8 [T+1, H, W, 3], one RGB frame per entry, equal to the env's
    obs['pov'] after each step (up to f32 rounding of the logged pose, EpisodeLogger).  The reference's own list
    interleaves that RGB frame with a render() frame flipped to BGR for its cv2 video writer (wrappers.py:95-100);
    here there is one RGB frame per entry, and the video beside the npz, {same name}.avi, is Motion-JPEG of those
    T+1 frames in log order (EpisodeLogger.save_video; video_fps, default 20, and video_quality, default 90, are
    attributes) where the reference writes an mp4."""

    def __init__(self, env):
        super().__init__(env)
        self.logging = False
        self.turned_off = True
        u = env.unwrapped
        self._log = EpisodeLogger(u._vec, 1, path='episodes', pov=u._renders())
        self.video_fps, self.video_quality = 20, 90

    def turn_on(self):
        self.turned_off = False
        self.logging = True

    def set_path(self, path):
        self._log.set_path(path)

    def set_desc(self, desc, glob_step):
        self._log.set_desc(desc, glob_step)

    def step(self, action):
        obs, reward, done, info = self.env.step(action)
        if done:
            for ep in self._log.collect(dump=self.logging):
                if 'file' in ep and 'pov' in ep:
                    self._log.pov_quality = self.video_quality
                    self._log.save_video(ep, ep['file'][:-4] + '.avi', self.video_fps)
        return obs, reward, done, info
