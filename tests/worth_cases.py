"""The cases the worth-query tests share (tests/test_worth_cpu.py, tests/test_gpu_worth.py) and their truth: the numpy
model of tests/worth_model.py on the CPU oracle's states.

The cases are the seven of tests/goal_cases.py at the same checkpoints and `unbuild`, which reaches what none of them
does: a place that REMOVES votes.  Its start holds two extra colour-1 blocks where the target is empty (synthetic -1) and
one the target wants in colour 2; the script breaks one of the extra blocks (a break that adds a vote for -1: reward +1).
From then on "place colour 1 back" takes that vote away (right < 0) and "break the other extra block" adds one
(right > 0)."""
import functools

import numpy as np

import goal_cases as GC
import mask_cases as MC
import worth_model as WM

E, T, CHECKPOINTS, PROBES = MC.E, MC.T, MC.CHECKPOINTS, MC.PROBES
RIGHT, WRONG = GC.RIGHT, GC.WRONG


def _unbuild():
    target = np.zeros((E, 9, 11, 11), np.int8)
    start = np.zeros_like(target)
    start[:, 0, 5, 3] = start[:, 0, 5, 4] = 1      # extra: the target is empty there
    start[:, 0, 4, 4] = 1                          # to be recoloured
    target[:, 0, 4, 4] = 2
    target[:, 0, 6, 4] = 3
    seq = [14] * 9 + [0] * 3 + [16] + [13] * 9
    a = np.zeros((T, E), np.int32)
    for i in range(E):
        s = i % 16
        a[s:s + len(seq), i] = seq
    return dict(kw=dict(MC.KW), targets=target, starts=start, poses=None, actions=a)


@functools.lru_cache(None)
def cases():
    return dict(GC.cases(), unbuild=_unbuild())


def starts_of(case):
    return case['starts'] if case['starts'] is not None else np.zeros_like(case['targets'])


def states_of(case, checkpoints=CHECKPOINTS):
    """The oracle's state at every checkpoint, arrays over [checkpoint, env]: grid int8 [C, E, 9, 11, 11], cached,
    step_no int32 [C, E], inventory int32 [C, E, 6]; and what the eight probe steps did: cell int32 [C, E, 8] (the
    changed cell, -1 for none), plane (0 = the cell was emptied, k = colour k was placed), gain float32 and ends uint8
    [C, E, 8] (the probe step's reward and done)."""
    C, n = len(checkpoints), len(case['targets'])
    res = dict(grid=np.zeros((C, n, 9, 11, 11), np.int8), cached=np.zeros((C, n), np.int32),
               step_no=np.zeros((C, n), np.int32), inventory=np.zeros((C, n, 6), np.int32),
               cell=np.full((C, n, 8), -1, np.int32), plane=np.full((C, n, 8), -1, np.int32),
               gain=np.zeros((C, n, 8), np.float32), ends=np.zeros((C, n, 8), np.uint8))
    for c, tc in enumerate(checkpoints):
        ob = MC.oracle_batch(case, 9)
        for t in range(tc):
            ob.step_walking(np.tile(case['actions'][t], 9), nthreads=8)
        before = ob.grid[:n].copy()
        res['grid'][c] = before.reshape(n, 9, 11, 11)
        res['inventory'][c] = ob.inventory[:n]
        for i in range(n):
            st = ob.envs[i].task_state()
            res['cached'][c, i], res['step_no'][c, i] = st['syn_max_int'], st['step_no']
        ob.step_walking(np.concatenate([np.zeros(n, np.int32)] + [np.full(n, p, np.int32) for p in PROBES]))
        for j in range(8):
            rows = slice((j + 1) * n, (j + 2) * n)
            diff = ob.grid[rows] != before
            assert (diff.sum(1) <= 1).all()
            cell = np.where(diff.any(1), diff.argmax(1), -1)
            res['cell'][c, :, j] = cell
            res['plane'][c, :, j] = np.where(cell >= 0, ob.grid[rows][np.arange(n), np.maximum(cell, 0)], -1)
            res['gain'][c, :, j], res['ends'][c, :, j] = ob.reward[rows], ob.done[rows]
    return res


def model_of(case, states, rows=None):
    """The model on the states: a list over checkpoints of lists over envs (`rows`: which, default all) of
    worth_model.env_worth dicts."""
    starts, kw = starts_of(case), case['kw']
    rows = range(len(case['targets'])) if rows is None else rows
    return [[WM.env_worth(case['targets'][i], starts[i], states['grid'][c, i], int(states['cached'][c, i]),
                          int(states['step_no'][c, i]), kw['max_steps']) for i in rows]
            for c in range(len(states['cached']))]


@functools.lru_cache(None)
def states(name):
    res = states_of(cases()[name])
    for v in res.values():
        v.setflags(write=False)
    return res


@functools.lru_cache(None)
def model(name):
    """model_of the named case at CHECKPOINTS, every env (computed once; treat as read-only)."""
    return model_of(cases()[name], states(name))


def words(name):
    """int16 [C, E, 7, 1104]: the model's words of the named case."""
    return np.stack([np.stack([m['word'] for m in row]) for row in model(name)])
