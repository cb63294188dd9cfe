"""The cases the recall-query tests share (tests/test_recall_cpu.py, tests/test_gpu_recall.py) and their truth, from the
CPU oracle alone.

The cases are the eight of tests/worth_cases.py: E = 32 envs, T = 48 steps, every (e, t) pair a sample.  base(name) steps
the oracle over the case's actions and keeps what the log would hold and what the live state was:
  grids    int8 [T + 1, E, 1089]     the grid at every entry
  change   uint16 [E, T]             relabel_cases.words_of(grids)
  pos      float32 [E, T, 5]         the step's agentPos output (x, y, z, pitch, yaw): what the log keeps
  live     float64 [E, T + 1, 5]     internals() x, y, z, yaw, pitch at every entry: what a live vox_obs read
  init     float64 [E, 5]            the reset pose (= live[:, 0], = the case's poses where it has them)
  starts   int8 [E, 1089]
records_of() makes zeroed 64-byte records of them, episode after episode."""
import functools

import numpy as np

import mask_cases as MC
import relabel_cases as RC
import vox_model as VM
import worth_cases as WC

E, T = WC.E, WC.T
SPEC_STACKS = (1, 2, 4, 8)      # the K of the GPU comparison's specs: the coverage is counted for the largest window
# What coverage() counts over the eight cases: each floor is the count the oracle gives.
FLOORS = {'t = 1 (entry 0, the reset pose)': 256, 't = length': 256, 'a stack reaching before entry 0': 1792,
          "the step's own word is not empty": 1939, 'a cell changed twice within one window': 3343,
          'obs and next_obs in different quadrants': 73, 'quadrant 0': 10121, 'quadrant 1': 1685, 'quadrant 2': 343,
          'quadrant 3': 395, 'a head cell outside the grid': 0, 'a half-integer x or z': 267,
          'live and logged head cells differ': 3}
# Below 20 because the walking cases do not allow more: the agent never leaves the grid, and the float32 log rounds a
# head cell differently on three entries only.
NOT_IN_THE_CASES = ('a head cell outside the grid', 'live and logged head cells differ')


def cases():
    return WC.cases()


@functools.lru_cache(None)
def base(name):
    case = cases()[name]
    ob = MC.oracle_batch(case)
    res = dict(grids=np.zeros((T + 1, E, 1089), np.int8), pos=np.zeros((E, T, 5), np.float32),
               live=np.zeros((E, T + 1, 5)))
    res['grids'][0] = ob.grid
    res['live'][:, 0] = ob.internals()[:, :5]
    for t in range(T):
        ob.step_walking(case['actions'][t], nthreads=8)
        res['grids'][t + 1] = ob.grid
        res['pos'][:, t] = ob.agentPos
        res['live'][:, t + 1] = ob.internals()[:, :5]
    res['change'] = RC.words_of(res['grids'])
    res['starts'] = WC.starts_of(case).reshape(E, -1).astype(np.int8)
    res['init'] = res['live'][:, 0].copy()
    if case['poses'] is not None:
        assert np.array_equal(res['init'], np.asarray(case['poses'], np.float64))
    assert np.array_equal(res['grids'][0], res['starts'])
    for v in res.values():
        v.setflags(write=False)
    return res


def records_of(change, pos):
    """uint8 [E * T, 64]: zeroed trajectory records that carry the change words [E, T] and the poses [E, T, 5]."""
    rec = np.zeros((change.size, 64), np.uint8)
    rec[:, 0:20] = np.ascontiguousarray(pos.reshape(-1, 5)).view(np.uint8).reshape(-1, 20)
    rec[:, 40:42] = np.ascontiguousarray(change.reshape(-1)).view(np.uint8).reshape(-1, 2)
    return rec


def pairs():
    """(episode int32 [E * T], step int32 [E * T]): every (e, t), t = 1 .. T."""
    e, t = np.meshgrid(np.arange(E), np.arange(1, T + 1), indexing='ij')
    return e.reshape(-1).astype(np.int32), t.reshape(-1).astype(np.int32)


def log_pose(b):
    """float64 [E, T + 1, 4] (x, y, z, yaw) of every entry as the log has it: the reset pose, then the f32 agentPos."""
    p = b['pos'].astype(np.float64)
    return np.concatenate([b['init'][:, None, :4], p[:, :, [0, 1, 2, 4]]], 1)


def head_differs(b):
    """bool [E, T + 1]: rint of the live float64 state and rint of its float32 rounding pick different head cells."""
    live, log = b['live'][:, :, :3], log_pose(b)[:, :, :3]
    return (np.rint(live) != np.rint(log)).any(2)


def coverage(b, k=max(SPEC_STACKS)):
    """The counts of test_recall_cpu's floors for one case, over its E * T samples, on the oracle-side arrays alone."""
    pose = log_pose(b)                                   # [E, T + 1, 4]
    q = VM.quadrant(pose[..., 3])                        # [E, T + 1]
    hx, hy, hz = (np.rint(pose[..., i]).astype(np.int64) + off for i, off in ((0, 5), (1, 1), (2, 5)))
    outside = (hx < 0) | (hx > 10) | (hz < 0) | (hz > 10) | (hy < 0) | (hy > 8)
    frac = np.abs(pose[..., [0, 2]] - np.floor(pose[..., [0, 2]]))
    half = (frac == 0.5).any(-1)
    change = b['change'].astype(np.int64)
    cell =np.where(change != RC.NONE, change & 0x7ff, -1)
    twice = 0
    for e in range(E):
        for t in range(1, T + 1):                        # the window's own words: records max(0, t - k) .. t - 1
            w = cell[e, max(0, t - k):t]
            w = w[w >= 0]
            twice += len(w) != len(set(w.tolist()))
    t = np.arange(1, T + 1)
    return {'t = 1 (entry 0, the reset pose)': E, 't = length': E,
            'a stack reaching before entry 0': E * int((t < k).sum()),
            "the step's own word is not empty": int((change != RC.NONE).sum()),
            'a cell changed twice within one window': twice,
            'obs and next_obs in different quadrants': int((q[:, 1:] != q[:, :-1]).sum()),
            'quadrant 0': int((q == 0).sum()), 'quadrant 1': int((q == 1).sum()),
            'quadrant 2': int((q == 2).sum()), 'quadrant 3': int((q == 3).sum()),
            'a head cell outside the grid': int(outside.sum()),
            'a half-integer x or z': int(half.sum()),
            'live and logged head cells differ': int(head_differs(b).sum())}
