"""The cases the voxel-observation tests share (tests/test_vox_cpu.py, tests/test_gpu_vox.py) and what the model
(tests/vox_model.py) is fed with, all of it from the CPU oracle.

  walking    the six scenarios of tests/mask_cases.py and `recolour` of tests/goal_cases.py, at their checkpoints
  flying     one 16-env batch as smoke() builds it (device-trig oracle, auto-reset), at FLY_CHECKPOINTS
  directed   a table of reset poses (walking and flying), compared straight after reset()
Per (checkpoint, env) the truth holds the oracle's grid, its binary64 pose (x, y, z, yaw of internals()), the user's
target grid and the goal query's want / todo (goal_cases.env_truth: the oracle's stateless Task evaluation)."""
import functools

import numpy as np

import goal_cases as GC
import mask_cases as MC

E, CHECKPOINTS = MC.E, MC.CHECKPOINTS
FLY_N, FLY_T, FLY_CHECKPOINTS = 16, 60, (0, 1, 7, 20, 41, 60)
FLY_KW = dict(size_reward=False, max_steps=40, action_space='flying')
# the directed table.  Every value passes the pose validation of set_tasks (|x|, |z| <= 10, |y| <= 64, |yaw| <= 1e6),
# so none is dropped.
XZ = (-0.5, 0.5, 1.5, 2.5, 5.5, -7.0, 7.0)         # half-even ties; centres on and beyond the edge
YS = (-0.25, 0.5, 7.5, 8.9)                        # the head level inside, at 9 and at 10
YAWS = (0.0, float(np.nextafter(45.0, 0.0)), 45.0, float(np.nextafter(135.0, 0.0)), 135.0, 225.0, 315.0, 360.0)
FLY_YAWS = YAWS + (-45.0, -45.5, 404.5, 99999.0)
FLOORS = {'quadrant 0': 20, 'quadrant 1': 20, 'quadrant 2': 20, 'quadrant 3': 20, 'half-integer x or z': 20,
          'head outside in x / z': 10, 'head outside in y': 10, 'want with a negative id': 20,
          'target differs from the table row': 20}
DIRECTED_FLOORS = tuple(FLOORS)[:7]                # what the directed table alone has to reach


def walking_cases():
    return GC.cases()


def directed_poses(flying):
    """float64 [M, 5] (x, y, z, yaw, pitch): every yaw with every (x, z) pair, the level cycling through YS."""
    yaws = FLY_YAWS if flying else YAWS
    rows = [(x, YS[(a + b + j) % len(YS)], z, yaw, 0.0)
            for j, yaw in enumerate(yaws) for a, x in enumerate(XZ) for b, z in enumerate(XZ)]
    return np.array(rows, np.float64)


def directed_case(flying):
    """Reset poses over a world that is not symmetric under any turn: rt20 targets and 30 starting blocks of random
    colours per env (so that 'target' needs the starting grid and 'want' has negative ids)."""
    from gridworld_amd import workloads
    poses = directed_poses(flying)
    m = len(poses)
    rng = np.random.RandomState(23 + int(flying))
    targets = workloads.rt20(m, seed=9).numpy().astype(np.int8)
    starts = np.zeros((m, 1089), np.int8)
    for i in range(m):
        starts[i, rng.permutation(1089)[:30]] = rng.randint(1, 7, 30)
    kw = dict(FLY_KW) if flying else dict(MC.KW)
    return dict(kw=kw, targets=targets, starts=starts.reshape(m, 9, 11, 11), poses=poses)


def _snapshot(ob, case, n):
    starts = case.get('starts')
    starts = np.zeros_like(case['targets']) if starts is None else starts
    grid = ob.grid[:n].reshape(n, 9, 11, 11).copy()
    want, todo = np.zeros_like(grid), np.zeros_like(grid)
    for i in range(n):
        _, _, want[i], todo[i] = GC.env_truth(case['targets'][i], starts[i], grid[i], 0)
    return dict(grid=grid, pose=ob.internals()[:n, :4].copy(), want=want, todo=todo)


def _finish(shots, case):
    res = {k: np.stack([s[k] for s in shots]) for k in shots[0]}
    res['target'] = np.broadcast_to(case['targets'].astype(np.int8), res['grid'].shape).copy()
    starts = case.get('starts')
    res['table'] = res['target'] - (0 if starts is None else starts.astype(np.int8))   # the task table's synthetic row
    for v in res.values():
        v.setflags(write=False)
    return res


@functools.lru_cache(None)
def walking_truth(name):
    """dict over [checkpoint, env] of a walking case: grid, want, todo, target, table int8 [C, E, 9, 11, 11], pose
    float64 [C, E, 4]."""
    case = walking_cases()[name]
    ob = MC.oracle_batch(case)
    shots = []
    for t in range(max(CHECKPOINTS) + 1):
        if t in CHECKPOINTS:
            shots.append(_snapshot(ob, case, E))
        ob.step_walking(case['actions'][t], nthreads=8)
    return _finish(shots, case)


def flying_case():
    """smoke()'s flying batch: targets, and the four action arrays of every step."""
    from gridworld_amd import workloads
    targets = workloads.rt20(64, seed=3).numpy().astype(np.int8)[:FLY_N]
    rng = np.random.RandomState(5)
    acts = [dict(movement=rng.uniform(-1, 1, (FLY_N, 3)).astype(np.float32),
                 camera=rng.uniform(-5, 5, (FLY_N, 2)).astype(np.float32),
                 inventory=rng.randint(0, 7, FLY_N).astype(np.int32),
                 placement=rng.randint(0, 3, FLY_N).astype(np.int32)) for _ in range(FLY_T)]
    return dict(kw=dict(FLY_KW), targets=targets, starts=None, poses=None, actions=acts)


@functools.lru_cache(None)
def flying_truth():
    from oracle import oracle as O
    case = flying_case()
    ob = O.OracleBatch(FLY_N, **case['kw'])
    ob.set_tasks(case['targets'])
    ob.reset()
    shots = []
    O.use_device_trig(True)
    try:
        for t in range(FLY_T + 1):
            if t in FLY_CHECKPOINTS:
                shots.append(_snapshot(ob, case, FLY_N))
            if t < FLY_T:
                a = case['actions'][t]
                ob.step_flying(a['movement'], a['camera'], a['inventory'], a['placement'], autoreset=True)
    finally:
        O.use_device_trig(False)
    return _finish(shots, case)


@functools.lru_cache(None)
def directed_truth(flying):
    """The one checkpoint of a directed case: straight after reset()."""
    from oracle import oracle as O
    case = directed_case(flying)
    m = len(case['poses'])
    ob = O.OracleBatch(m, **case['kw'])
    ob.set_tasks(case['targets'], case['starts'])
    ob.set_initial_pose(case['poses'])
    ob.reset()
    return _finish([_snapshot(ob, case, m)], case)


def all_truths():
    """name -> truth of every case."""
    res = {name: walking_truth(name) for name in walking_cases()}
    res['flying'] = flying_truth()
    res['directed_walking'], res['directed_flying'] = directed_truth(False), directed_truth(True)
    return res


def coverage(truth):
    """The counts FLOORS asks for, over the (checkpoint, env) pairs of one truth."""
    import vox_model as VM
    pose = truth['pose'].reshape(-1, 4)
    q = VM.quadrant(pose[:, 3])
    hx, hy, hz = VM.head_cell(pose)
    half = lambda v: np.abs(v - np.floor(v) - 0.5) == 0.0  # noqa: E731
    rows = lambda k: truth[k].reshape(len(pose), -1)  # noqa: E731
    got = {'quadrant %d' % k: int((q == k).sum()) for k in range(4)}
    got['half-integer x or z'] = int((half(pose[:, 0]) | half(pose[:, 2])).sum())
    got['head outside in x / z'] = int(((hx < 0) | (hx > 10) | (hz < 0) | (hz > 10)).sum())
    got['head outside in y'] = int(((hy < 0) | (hy > 8)).sum())
    got['want with a negative id'] = int((rows('want') < 0).any(1).sum())
    got['target differs from the table row'] = int((rows('target') != rows('table')).any(1).sum())
    return got
