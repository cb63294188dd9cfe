"""The query launches of the batched env (vec_env._Rows): one adapter per query library, from a row range of a batch's
state -- a whole VecGridWorld or a SubBatch, `env` -- to the library module's launch().  Every adapter takes the stream
to launch on and `alloc_stream`, the torch stream its allocations and torch operations go to (None: the current one).
What the adapters share is stated once in front of them."""
import numpy as np
import torch

from . import _lib as L
from . import aim as A
from . import goal as G
from . import peek as P
from . import peek_dict as PD
from . import query as Q
from . import recall as RCL
from . import relabel as RL
from . import vox as X
from . import worth as W

_TASK = ('task_target', 'task_start', 'task_meta', 'task_index')
_GOAL_STATE = ('grid', 'hist', 'aux', 'agent') + _TASK            # what igw_goal and igw_worth read, in their order
_PEEK_STATE = ('grid', 'occ', 'hist', 'aux', 'agent') + _TASK     # ... and the peek entries


def _state(env, names):
    """The range's rows of the state tensors and the task table's tensors, by name."""
    root, sl = env._root(), env._sl
    agent, grid, occ = env._rows
    got = dict(grid=grid, occ=occ, agent=agent, hist=root.hist_buf[sl], aux=root.aux_buf[sl])
    return [got[k] if k in got else getattr(root, k) for k in names]


def _reward(cfg, select_and_place=False):
    """(right_scale, wrong_scale, max_steps[, select_and_place]) as the libraries take them."""
    return (cfg.right_placement_scale, cfg.wrong_placement_scale, cfg.max_steps) + \
        ((cfg.select_and_place,) if select_and_place else ())


def _no_size_reward(size_reward, who):
    if size_reward:
        raise ValueError(f'{who} predicts the reward of the env itself; with size_reward=True the step returns '
                         "SizeReward's (make the env with size_reward=False)")


def _integers(x):
    """Whether a tensor or an array holds integers: no floats, complex numbers or bools."""
    if torch.is_tensor(x):
        return not (x.is_floating_point() or x.is_complex() or x.dtype == torch.bool)
    return x.dtype.kind in 'iu'


def _space(env):
    return 'flying' if env.flying else 'walking_dict' if env.walk_dict else 'walking'


def finished_episodes(heads, lo, cap):
    """(first int64 [n], length int32 [n], task int64 [n], valid uint8 [n]) of the most recent finished episode of every
    env of a slice heads[lo:lo + n] of the log's heads (include/igw.h: task row, steps recorded, episode number,
    finished per slot): plain torch on the heads' device, nothing comes to the host."""
    n = heads.shape[0]
    fin = (heads[:, :, 3] != 0) & (heads[:, :, 1] > 0)
    number = heads[:, :, 2].long() & 0xffffffff
    score = torch.where(fin, number, torch.full_like(number, -1))
    slot = score.argmax(1)
    valid = score.gather(1, slot[:, None])[:, 0] >= 0
    row = heads.gather(1, slot[:, None, None].expand(n, 1, 4))[:, 0]
    length = torch.where(valid, row[:, 1].clamp(0, cap), torch.zeros_like(row[:, 1]))
    task = torch.where(valid, row[:, 0], torch.zeros_like(row[:, 0])).long()
    first = ((torch.arange(n, device=heads.device) + lo) * 2 + slot) * cap
    return first, length.to(torch.int32), task, valid.to(torch.uint8)


def _log_range(env, who):
    """(rec, heads, cap, lo, e): the log's records, heads and capacity, and the range's logged envs [lo, lo + e).
    ValueError without a log and for a range that holds no logged env; nothing touches the device."""
    root = env._root()
    if root._traj is None:
        raise ValueError(f'{who} reads the episode log: call enable_trajectory_log() or make an EpisodeLogger first')
    rec, heads, n_logged, cap = root._traj
    lo, hi = env.lo, min(env.lo + env.num_envs, n_logged)
    if hi <= lo:
        raise ValueError(f'{who}: none of the envs [{env.lo}, {env.lo + env.num_envs}) is logged (the log holds the first {n_logged})')
    return rec, heads, cap, lo, hi - lo


def _last_episodes(env, heads, lo, cap):
    """(first, length, task, valid, starts) of the logged envs whose heads are `heads`, the log's [lo:lo + e]:
    finished_episodes() with the task row clamped to the table, and the grids the episodes started from.  Torch
    operations on the current stream."""
    root = env._root()
    first, length, task, valid = finished_episodes(heads, lo, cap)
    task = task.clamp(0, root.num_tasks - 1)
    return first, length, task, valid, root.task_start.index_select(0, task)


def mask_rows(env, out, look, sample, stream, alloc_stream=None):
    """One igw_action_mask launch (query.launch)."""
    if env.flying or env.walk_dict:
        raise ValueError('action_mask is defined for the Discrete(18) walking action space only (the flying and Dict '
                         'actions turn the camera in the same step as they place)')
    agent, _, occ = env._rows
    return Q.launch(agent, occ, env.num_envs, env.select_and_place, out, look, sample, env.env_index_base, env.device,
                    stream, alloc_stream)


def aim_rows(env, max_turns, place, brk, out, stream, alloc_stream=None):
    """One igw_aim launch (aim.launch)."""
    if env.flying or env.walk_dict:
        raise ValueError('aim is defined for the Discrete(18) walking action space only (its turns are that space\'s '
                         '5-degree camera actions)')
    agent, _, occ = env._rows
    return A.launch(agent, occ, env.num_envs, max_turns, place, brk, out, env.device, stream, alloc_stream)


def peek_rows(env, actions, gamma, names, out, stream, alloc_stream=None):
    """One igw_peek launch (peek.launch)."""
    if env.flying or env.walk_dict:
        raise ValueError('peek is defined for the Discrete(18) walking action space only')
    _no_size_reward(env.cfg.size_reward, 'peek')
    if not torch.is_tensor(actions):
        actions = np.asarray(actions)
    if not _integers(actions):
        raise ValueError(f'peek: actions must be integers, got {actions.dtype}')
    P.shape_of(actions, env.num_envs)
    if not (torch.is_tensor(actions) and actions.dtype == torch.int32 and actions.device == env.device
            and actions.is_contiguous()):
        with torch.cuda.stream(alloc_stream):
            # (anything outside 0..17 is a no-op whatever its width: it becomes -1 before the narrowing, which would wrap a
            # wide value into the range)
            if torch.is_tensor(actions):
                host = torch.where((actions < 0) | (actions > 17), torch.full_like(actions, -1), actions)
            else:
                host = torch.from_numpy(np.where((actions < 0) | (actions > 17), -1, actions).astype(np.int32))
            actions = host.to(device=env.device, dtype=torch.int32).contiguous()
    env._in_use(actions)
    return P.launch(_state(env, _PEEK_STATE), env.num_envs, actions, _reward(env.cfg, True), gamma, names, out, env.device,
                    stream, alloc_stream)


def peek_dict_rows(env, actions, gamma, names, out, stream, alloc_stream=None):
    """One igw_peek_flying / igw_peek_walking_dict launch (peek_dict.launch)."""
    if not (env.flying or env.walk_dict):
        raise ValueError('peek_dict is defined for the flying and the walking Dict action spaces; in the Discrete(18) '
                         'space call env.peek')
    _no_size_reward(env.cfg.size_reward, 'peek_dict')
    PD.shape_of(_space(env), actions, env.num_envs)
    res, bufs = PD.launch(_space(env), _state(env, _PEEK_STATE), env.num_envs, actions, _reward(env.cfg, True), gamma,
                          names, out, env.device, stream, alloc_stream)
    env._in_use(*bufs)
    return res


def vox_rows(env, spec, out, restart, fill, goal, stream, alloc_stream=None):
    """One igw_vox_obs launch (vox.launch): 'grid' is the range's grid rows, 'target' the task table's synthetic target
    plus its starting grid by task row, 'want' / 'todo' the rows of `goal` (the dict goal() returned, or the range's
    persistent one)."""
    lack = [k for k in spec.needs() if goal is None or k not in goal]
    if lack:
        raise ValueError(f"vox_obs: the planes {lack} are the goal query's: pass goal=env.goal(want=True, todo=True)")
    root, sl, n = env._root(), env._sl, env.num_envs
    agent, grid, _ = env._rows
    sources = []
    for name, _ in spec.planes:
        if name == 'grid':
            sources.append((grid.data_ptr(), None, L.GRID_STRIDE, 0))
        elif name == 'target':
            sources.append((root.task_target.data_ptr(), root.task_start.data_ptr(), L.GRID_STRIDE, 1))
        else:
            ptr, stride = X.rows_of(f'goal[{name!r}]', goal[name], n)
            sources.append((ptr, None, stride, 0))
    return X.launch(agent, root.aux_buf[sl], n, spec, sources, out, restart, fill, env.device, stream, alloc_stream)


def worth_rows(env, names, allow, stocked, out, stream, alloc_stream=None):
    """One igw_worth launch (worth.launch)."""
    return W.launch(_state(env, _GOAL_STATE), env.num_envs, _reward(env.cfg), allow, stocked, names, out, env.device,
                    stream, alloc_stream)


def relabel_rows(env, goals, gamma, names, out, stream, alloc_stream=None):
    """One igw_relabel launch (relabel.launch) over the range's logged envs."""
    root, dev = env._root(), env.device
    _no_size_reward(env.cfg.size_reward, 'relabel')
    rec, heads, cap, lo, e = _log_range(env, 'relabel')
    with torch.cuda.stream(alloc_stream):
        first, length, task, valid, starts = _last_episodes(env, heads[lo:lo + e], lo, cap)
        targets = at = None
        if isinstance(goals, str):
            if goals == 'final':
                at = length[:, None].contiguous()
            elif goals == 'own':
                targets = (root.task_target.index_select(0, task) + starts)[:, None, :].contiguous()
            else:
                raise ValueError(f"relabel: goals is 'final', 'own', entries [E, G] or targets [E, G, 9, 11, 11], got {goals!r}")
        else:
            g = goals if torch.is_tensor(goals) else torch.as_tensor(np.asarray(goals))
            if not _integers(g):
                raise ValueError(f'relabel: goals must be integers, got {g.dtype}')
            if g.dim() == 2 and g.shape[0] == e:
                at = g.to(device=dev, dtype=torch.int32).contiguous()
            elif g.dim() in (3, 5) and g.shape[0] == e:
                targets = RL.grid_rows(g, dev, (e, int(g.shape[1])))
            else:
                raise ValueError(f'relabel: goals must be entries [{e}, G] or targets [{e}, G, 9, 11, 11] / [{e}, G, 1104], '
                                 f'got shape {tuple(g.shape)}')
    env._in_use(first, length, starts, targets, at, valid)
    res = RL.launch(rec, first, length, starts, targets, at, cap, _reward(env.cfg), gamma, names, out, dev, stream,
                    alloc_stream)
    res.update(length=length, valid=valid)
    return res


def recall_rows(env, spec, batch, seed, episode, step, goals, goal, names, out, stream, alloc_stream=None):
    """One igw_recall launch (recall.launch) over the range's logged envs."""
    root, dev = env._root(), env.device
    rec, heads, cap, lo, e = _log_range(env, 'recall')
    if (episode is None) != (step is None):
        raise ValueError('recall: give episode and step together, or batch= alone')
    if episode is None and (batch is None or isinstance(batch, bool) or int(batch) != batch or int(batch) < 0):
        raise ValueError(f'recall: give batch=, the number of samples to draw, or episode= and step=, got batch={batch!r}')

    def ints(name, x, dtype):
        t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
        if not _integers(t) or t.dim() != 1:
            raise ValueError(f'recall: {name} must be integers [B], got {t.dtype} {tuple(t.shape)}')
        return t.to(device=dev, dtype=dtype).contiguous()
    if goals is not None and not (isinstance(goals, dict) and 'target' in goals) and not (isinstance(goals, str) and goals == 'own'):
        raise ValueError("recall: goals is None, 'own' or the dict relabel() returned with 'target', got "
                         f'{goals if isinstance(goals, str) else type(goals).__name__!r}')
    if goals is None and RCL.needs_goal(spec):
        raise ValueError("recall: a 'target' plane shows the sample's goal: pass goals='own' or goals=env.relabel(..., "
                         "outputs=(..., 'target'))")
    if goal is not None and not isinstance(goals, dict):
        raise ValueError('recall: goal= names a column of goals=r, the dict relabel() returned')
    with torch.cuda.stream(alloc_stream):
        first, length, task, _, starts = _last_episodes(env, heads[lo:lo + e], lo, cap)
        init_pose = root.task_meta.index_select(0, task)[:, :40].contiguous().view(torch.float64)   # x, y, z, yaw, pitch
        if episode is None:
            episode, step = RCL.sample(length, int(batch), seed)
        else:
            episode, step = ints('episode', episode, torch.int32), ints('step', step, torch.int32)
            if episode.shape != step.shape:
                raise ValueError(f'recall: episode and step must have one length, got {tuple(episode.shape)}, {tuple(step.shape)}')
        b = episode.shape[0]
        rows, index, extra = None, None, {}
        if isinstance(goals, str):
            rows = root.task_target.index_select(0, task) + starts
        elif isinstance(goals, dict):
            rows = goals['target']
            if not torch.is_tensor(rows) or rows.dim() != 5 or rows.shape[0] != e or rows.device != dev:
                raise ValueError(f"recall: goals['target'] must be relabel()'s [{e}, G, 9, 11, 11] on {dev}")
            n_g = int(rows.shape[1])
            g = torch.zeros_like(episode, dtype=torch.int64) if goal is None else ints('goal', goal, torch.int64)
            if g.shape != episode.shape:
                raise ValueError(f'recall: goal must be [{b}], got {tuple(g.shape)}')
            ep = episode.long()
            inside = (ep >= 0) & (ep < e) & (g >= 0) & (g < n_g)
            index = torch.where(inside, ep * n_g + g, torch.full_like(g, -1))
            for k in ('reward', 'done'):
                if k in goals:
                    t = goals[k]
                    if not torch.is_tensor(t) or t.dim() != 3 or tuple(t.shape[:2]) != (e, n_g) or t.device != dev:
                        raise ValueError(f"recall: goals[{k!r}] must be relabel()'s [{e}, {n_g}, L] on {dev}")
                    at = (step.long() - 1)
                    ok = inside & (at >= 0) & (at < length.index_select(0, ep.clamp(0, e - 1)).clamp(max=t.shape[2]))
                    got = t[ep.clamp(0, e - 1), g.clamp(0, n_g - 1), at.clamp(0, t.shape[2] - 1)]
                    extra[k + '_relabel'] = torch.where(ok, got, torch.zeros_like(got))
    env._in_use(first, length, starts, init_pose, episode, step, rows, index)
    res = RCL.launch(rec, first, length, starts, init_pose, episode, step, spec, rows, index, cap, names, out, dev, stream,
                     alloc_stream, _space(env))
    res.update(extra, episode=episode, step=step)
    return res


def check_gain(other_space, size_reward):
    if other_space:
        raise ValueError('goal: gain is defined for the Discrete(18) walking action space only (the action mask it is '
                         'built on is)')
    _no_size_reward(size_reward, 'goal: gain')


def goal_rows(env, names, out, stream, alloc_stream=None, captured=False):
    """One igw_goal launch (goal.launch); with gain the two igw_action_mask launches in front of it (_Rows.goal).
    `captured`: the launch is part of a capture on `stream`, which then is torch's current stream; otherwise the torch
    work goes to the range's stream."""
    mask, look = None, None
    agent, _, occ = env._rows
    if 'gain' in names:
        check_gain(env.flying or env.walk_dict, env.cfg.size_reward)
        mask, look, full, spare = env._goal_scratch()
        ask = lambda ag, m, lk: Q.action_mask_into(ag.data_ptr(), occ.data_ptr(), env.num_envs,  # noqa: E731
                                                   env.select_and_place, m.data_ptr(), lk, None, 0, 0, 0, stream)
        ask(agent, mask, None)
        with torch.cuda.stream(None if captured else env.stream):
            full.copy_(agent, non_blocking=True)
            full.view(torch.int16)[:, 24:30].fill_(20)
        ask(full, spare, look.data_ptr())
    return G.launch(_state(env, _GOAL_STATE), env.num_envs, _reward(env.cfg, True), mask, look, names, out, env.device,
                    stream, alloc_stream)
