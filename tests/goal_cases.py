"""The cases the goal-query tests share (tests/test_goal_cpu.py, tests/test_gpu_goal.py) and their truth, computed from the
CPU oracle alone.

The cases are the six of tests/mask_cases.py and `recolour`, at the same checkpoints, with the same nine oracle blocks
per checkpoint (the base and eight probes).  Per checkpoint and env, with S = grid - start and T = target - start:
  align       oracle.task_eval(T, S)['argmax'] = (dx, dz, rot)
  want        that call's rotation `rot` of T, read at (x + dx, z + dz): the slice pairing of tasks/task.py:125-131
  todo        want where want != S, else 0
  fit         (task_eval's max_int, its target_size, nnz(S), task_state()['syn_max_int'])
  gain, ends  ob.reward / ob.done of the probe blocks after their probe step; every other action the base block's no-op
`recolour` reaches what none of the six does: a cached max_int that lags the live one (a cell recoloured with
wrong_placement == 0), so that the next placement is paid from the stale value."""
import functools

import numpy as np

import mask_cases as MC

E, T, CHECKPOINTS, PROBES = MC.E, MC.T, MC.CHECKPOINTS, MC.PROBES
RIGHT, WRONG = 1.0, 0.1   # the default scales (create_env, gridworld/env.py:333-338)


def _recolour():
    """Break a starting block of colour 1 where the target wants colour 2 (wrong = -1: the count is taken), place
    colour 2 there (wrong = 0: the reference keeps its cached max_int of 0 while the live one is 1), turn to the next
    cell; env i starts i % 16 steps late."""
    target = np.zeros((E, 9, 11, 11), np.int8)
    target[:, 0, 5, 3] = target[:, 0, 5, 4] = 2
    target[:, 0, 4, 4] = 3
    start = np.zeros_like(target)
    start[:, 0, 5, 3] = start[:, 0, 5, 4] = 1
    seq = [14] * 9 + [0] * 3 + [16, 7] + [13] * 9
    a = np.zeros((T, E), np.int32)
    for i in range(E):
        s = i % 16
        a[s:s + len(seq), i] = seq
    return dict(kw=dict(MC.KW), targets=target, starts=start, poses=None, actions=a)


@functools.lru_cache(None)
def cases():
    return dict(MC.cases(), recolour=_recolour())


def shifted(rot_t, dx, dz):
    """want[y][x][z] = rot_t[y][x + dx][z + dz] where both indices are in 0..10, else 0."""
    out = np.zeros_like(rot_t)
    x0, x1, z0, z1 = max(-dx, 0), 11 + min(-dx, 0), max(-dz, 0), 11 + min(-dz, 0)
    out[:, x0:x1, z0:z1] = rot_t[:, x0 + dx:x1 + dx, z0 + dz:z1 + dz]
    return out


def env_truth(target, start, grid, cached):
    """(align [3], fit [4], want, todo) of one env from the oracle's stateless Task evaluation."""
    from oracle import oracle as O
    t, s = target.astype(np.int8) - start.astype(np.int8), grid.astype(np.int8) - start.astype(np.int8)
    ev = O.task_eval(t, s)
    dx, dz, r = (int(v) for v in ev['argmax'])
    want = shifted(ev['rot'][r].reshape(9, 11, 11), dx, dz)
    todo = np.where(want != s.reshape(9, 11, 11), want, 0).astype(np.int8)
    return (np.array([dx, dz, r], np.int8),
            np.array([ev['max_int'], ev['target_size'], np.count_nonzero(s), cached], np.int16), want, todo)


def truth_of(case, checkpoints=CHECKPOINTS):
    """dict of arrays (of a case of any number of envs E) over [checkpoint, env]: align int8 [C, E, 3], fit int16 [C, E, 4], want / todo int8
    [C, E, 9, 11, 11], gain float32 [C, E, 18], ends uint8 [C, E, 18]; and for the coverage floors changed bool
    [C, E, 8] (the probe changed the grid) and live float32 [C, E, 8] (what a model that counts the probe's reward from
    the LIVE maximum instead of the cached one would pay)."""
    C, E = len(checkpoints), len(case['targets'])
    starts = case['starts'] if case['starts'] is not None else np.zeros_like(case['targets'])
    res = dict(align=np.zeros((C, E, 3), np.int8), fit=np.zeros((C, E, 4), np.int16),
               want=np.zeros((C, E, 9, 11, 11), np.int8), todo=np.zeros((C, E, 9, 11, 11), np.int8),
               gain=np.zeros((C, E, 18), np.float32), ends=np.zeros((C, E, 18), np.uint8),
               changed=np.zeros((C, E, 8), bool), live=np.zeros((C, E, 8), np.float32))
    for c, tc in enumerate(checkpoints):
        ob = MC.oracle_batch(case, 9)
        for t in range(tc):
            ob.step_walking(np.tile(case['actions'][t], 9), nthreads=8)
        before = ob.grid.copy()
        state0 = [ob.envs[i].task_state() for i in range(E)]
        for i in range(E):
            res['align'][c, i], res['fit'][c, i], res['want'][c, i], res['todo'][c, i] = env_truth(
                case['targets'][i], starts[i], before[i].reshape(9, 11, 11), state0[i]['syn_max_int'])
        ob.step_walking(np.concatenate([np.zeros(E, np.int32)] + [np.full(E, p, np.int32) for p in PROBES]))
        res['gain'][c] = ob.reward[:E, None]
        res['ends'][c] = ob.done[:E, None]
        for j, p in enumerate(PROBES):
            rows = slice((j + 1) * E, (j + 2) * E)
            res['gain'][c, :, p], res['ends'][c, :, p] = ob.reward[rows], ob.done[rows]
            res['changed'][c, :, j] = (ob.grid[rows] != before[:E]).any(1)
            for i in range(E):
                st = ob.envs[(j + 1) * E + i].task_state()
                wrong = state0[i]['syn_prev_size'] - st['syn_prev_size']
                right = st['syn_max_int'] - int(res['fit'][c, i, 0]) if wrong != 0 else 0
                res['live'][c, i, j] = np.float32(right * RIGHT if right != 0 else wrong * WRONG)
    return res


@functools.lru_cache(None)
def truth(name):
    """truth_of the named case at CHECKPOINTS (read-only, computed once)."""
    res = truth_of(cases()[name])
    for v in res.values():
        v.setflags(write=False)
    return res
