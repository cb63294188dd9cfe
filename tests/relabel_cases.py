"""The cases the relabel-query tests share (tests/test_relabel_cpu.py, tests/test_gpu_relabel.py) and their truth, from
the CPU oracle alone.

The cases are the eight of tests/worth_cases.py: E = 32 envs, T = 48 steps.  Every env's episode is relabelled under six
goals:
  own      the episode's own target
  final    its grid at entry T (what it ended up building)
  at24     its grid at entry 24
  at5      its grid at entry 5
  at0      its starting grid (an empty synthetic target: done on every step)
  rolled   the next env's target
Truth of a goal: an OracleBatch with set_tasks(goal, starts) (+ the case's poses), reset and stepped with the case's
actions -- reward, done and the synthetic task's cached max_int of every step.  The change words are the base run's grid
differences, in the trajectory record's encoding (include/igw.h)."""
import functools

import numpy as np

import mask_cases as MC
import worth_cases as WC

E, T = WC.E, WC.T
RIGHT, WRONG = WC.RIGHT, WC.WRONG
GOALS = ('own', 'final', 'at24', 'at5', 'at0', 'rolled')
AT = {'final': T, 'at24': 24, 'at5': 5, 'at0': 0}     # the goals that are entries of the episode itself
NONE = 0xffff


def cases():
    return WC.cases()


def run(case, targets, max_steps=None):
    """The case's actions stepped by the oracle under `targets` [E, 9, 11, 11]: reward float32 [E, T], done uint8 [E, T],
    progress int16 [E, T] (task_state()['syn_max_int'] after the step) and grids int8 [T + 1, E, 1089]."""
    kw = dict(case['kw']) if max_steps is None else dict(case['kw'], max_steps=max_steps)
    ob = MC.oracle_batch(dict(case, kw=kw, targets=targets))
    n = len(targets)
    res = dict(reward=np.zeros((n, T), np.float32), done=np.zeros((n, T), np.uint8), progress=np.zeros((n, T), np.int16),
               grids=np.zeros((T + 1, n, 1089), np.int8))
    res['grids'][0] = ob.grid
    for t in range(T):
        ob.step_walking(case['actions'][t], nthreads=8)
        res['reward'][:, t], res['done'][:, t] = ob.reward, ob.done
        res['progress'][:, t] = [e.task_state()['syn_max_int'] for e in ob.envs]
        res['grids'][t + 1] = ob.grid
    return res


def words_of(grids):
    """uint16 [E, T]: the change word of every step of a grid sequence [T + 1, E, 1089]."""
    diff = grids[1:] != grids[:-1]
    assert (diff.sum(2) <= 1).all()
    cell = diff.argmax(2)                                              # [T, E]
    colour = np.take_along_axis(grids[1:], cell[..., None], 2)[..., 0].astype(np.int64)
    return np.where(diff.any(2), cell | colour << 11, NONE).astype(np.uint16).T.copy()


@functools.lru_cache(None)
def base(name):
    """The base run of the named case (its own targets): run()'s dict plus change uint16 [E, T] and starts int8
    [E, 1089].  Read-only."""
    case = cases()[name]
    res = run(case, case['targets'])
    res['change'] = words_of(res['grids'])
    res['starts'] = WC.starts_of(case).reshape(E, -1).astype(np.int8)
    assert np.array_equal(res['grids'][0], res['starts'])
    for v in res.values():
        v.setflags(write=False)
    return res


def goal_grids(name):
    """int8 [E, 6, 1089]: the six goal grids of every env, in GOALS' order."""
    case, b = cases()[name], base(name)
    own = case['targets'].reshape(E, -1).astype(np.int8)
    pick = {'own': own, 'rolled': np.roll(own, -1, axis=0)}
    pick.update({k: b['grids'][t] for k, t in AT.items()})
    return np.stack([pick[k] for k in GOALS], 1)


@functools.lru_cache(None)
def truth(name, max_steps=None):
    """The oracle's answer for the named case under every goal: reward float32 / done uint8 / progress int16 [E, 6, T]
    and grids int8 [6, T + 1, E, 1089].  Read-only."""
    case, goals = cases()[name], goal_grids(name)
    runs = [run(case, goals[:, g].reshape(E, 9, 11, 11), max_steps) for g in range(len(GOALS))]
    res = {k: np.stack([r[k] for r in runs], 1) for k in ('reward', 'done', 'progress')}
    res['grids'] = np.stack([r['grids'] for r in runs])
    for v in res.values():
        v.setflags(write=False)
    return res


def end_of(done):
    """int32 [...]: t of the first done step along the last axis, 0 without one."""
    return np.where(done.any(-1), done.argmax(-1) + 1, 0).astype(np.int32)


def records_of(change):
    """uint8 [E * T, 64]: zeroed trajectory records that carry the change words [E, T], episode after episode."""
    rec = np.zeros((change.size, 64), np.uint8)
    rec[:, 40:42] = np.ascontiguousarray(change.reshape(-1)).view(np.uint8).reshape(-1, 2)
    return rec
