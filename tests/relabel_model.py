"""A numpy model of the relabel query (include/igw_relabel.h), for tests/relabel_cases.py,
tests/test_relabel_cpu.py and tests/test_gpu_relabel.py.

It works from (start, change words, target, scales, max_steps, gamma) alone: the grid sequence is the start with the
change words applied in order, the maximal intersection is the CPU oracle's stateless Task evaluation
(oracle.task_eval(target - start, grid_t - start)) taken only where the block count of grid_t - start moved, and the
cache that goes stale in between is kept explicitly."""
import numpy as np

CELLS, ROW, RECORD = 1089, 1104, 64
NONE = 0xffff
_evals = {}


def max_int(syn_target, syn_grid):
    """oracle.task_eval(...)['max_int'], remembered per (target, grid)."""
    from oracle import oracle as O
    key = (syn_target.tobytes(), syn_grid.tobytes())
    if key not in _evals:
        _evals[key] = int(O.task_eval(syn_target, syn_grid)['max_int'])
    return _evals[key]


def grids_of(start, change):
    """int8 [len + 1, 1089]: entry 0 the start, entry t the grid after step t (a change to a cell >= 1089 is ignored)."""
    g = np.empty((len(change) + 1, CELLS), np.int8)
    g[0] = start[:CELLS]
    for t, w in enumerate(np.asarray(change, np.int64)):
        g[t + 1] = g[t]
        if w != NONE and (w & 0x7ff) < CELLS:
            g[t + 1, w & 0x7ff] = (w >> 11) & 7
    return g


def episode(start, change, target, right_scale=1.0, wrong_scale=0.1, max_steps=250, gamma=1.0, L=None):
    """One (episode, goal) pair: dict of reward float32 [L], done uint8 [L], progress int16 [L], end, ret (float32),
    target_size; and for the coverage counts recoloured (steps that changed a cell with wrong == 0) and stale_paid (steps
    paid right != 0 while the cache lagged the live maximum)."""
    start = np.asarray(start, np.int8)[:CELLS]
    start = np.where((start < 0) | (start > 6), 0, start).astype(np.int8)
    target = np.asarray(target, np.int8)[:CELLS]
    target = np.where((target < 0) | (target > 7), 0, target).astype(np.int8)
    n = len(change)
    L = n if L is None else L
    T = (target - start).astype(np.int8)
    tsize = int(np.count_nonzero(T))
    grids = grids_of(start, change)
    res = dict(reward=np.zeros(L, np.float32), done=np.zeros(L, np.uint8), progress=np.zeros(L, np.int16),
               target_size=tsize, recoloured=0, stale_paid=0)
    cached, prev, end, stale = 0, 0, 0, False
    ret, g = np.float64(0.0), np.float64(1.0)
    for t in range(1, n + 1):
        syn = (grids[t] - start).astype(np.int8)
        size = int(np.count_nonzero(syn))
        wrong = prev - size
        prev = size
        before = cached
        if wrong != 0:
            cached = max_int(T, syn)
            res['stale_paid'] += int(stale and cached != before)
            stale = False
        elif (grids[t] != grids[t - 1]).any():
            res['recoloured'] += 1
            stale = stale or max_int(T, syn) != cached
        right = cached - before
        done = cached == tsize or t == max_steps
        reward = np.float64(wrong) * np.float64(wrong_scale) if right == 0 else np.float64(right) * np.float64(right_scale)
        if end == 0:
            with np.errstate(all='ignore'):
                ret = ret + g * reward
                g = g * np.float64(gamma)
        if done and end == 0:
            end = t
        with np.errstate(all='ignore'):
            res['reward'][t - 1] = np.float32(reward)
        res['done'][t - 1] = done
        res['progress'][t - 1] = cached
    with np.errstate(all='ignore'):
        res.update(end=end, ret=np.float32(ret))
    return res


def relabel(records, first, length, starts, targets=None, at=None, L=1, right_scale=1.0, wrong_scale=0.1, max_steps=250,
            gamma=1.0):
    """igw_relabel on numpy arrays: records uint8 [n, 64], first [E], length [E], starts int8 [E, 1104], targets int8
    [E, G, 1104] or at [E, G].  Returns the seven outputs (target as [E, G, 1104])."""
    records = np.ascontiguousarray(records, np.uint8).reshape(-1, RECORD)
    words = records[:, 40:42].copy().view(np.uint16)[:, 0]
    E = len(first)
    G = (targets if at is None else at).shape[1]
    out = dict(reward=np.zeros((E, G, L), np.float32), done=np.zeros((E, G, L), np.uint8),
               progress=np.zeros((E, G, L), np.int16), end=np.zeros((E, G), np.int32), ret=np.zeros((E, G), np.float32),
               target_size=np.zeros((E, G), np.int16), target=np.zeros((E, G, ROW), np.int8))
    for e in range(E):
        n = min(max(int(length[e]), 0), L)
        f = int(first[e])
        if f < 0 or f + n > len(words):
            continue
        change = words[f:f + n]
        start = np.asarray(starts[e], np.int8)[:CELLS]
        start = np.where((start < 0) | (start > 6), 0, start).astype(np.int8)
        grids = grids_of(start, change)
        for g in range(G):
            if at is None:
                goal = np.asarray(targets[e, g], np.int8)[:CELLS]
                goal = np.where((goal < 0) | (goal > 7), 0, goal).astype(np.int8)
            else:
                goal = grids[min(max(int(at[e, g]), 0), n)]
            r = episode(start, change, goal, right_scale, wrong_scale, max_steps, gamma, L)
            for k in ('reward', 'done', 'progress', 'end', 'ret', 'target_size'):
                out[k][e, g] = r[k]
            out['target'][e, g, :CELLS] = goal
    return out
