"""The sizes, the windows and the scenario of the tests past the 2^31 and 2^32 byte marks (tests/test_gpu_large.py; checked
on the oracle alone by tests/test_large_cases_cpu.py).

Sizes.  Every buffer of the ABI is addressed as base + index * stride.  A byte offset kept in 32 bits wraps at 2^31
(signed) or 2^32 (unsigned), so the smallest batch that can show either is the one whose widest row passes 2^32: the
1,024-byte histogram row at env 2^22.  All sizes below are derived from gridworld_amd/_lib.py and the headers.

Windows.  Nothing of whole-batch size is copied to the host: `windows(stride, n)` names the rows that are -- the first
64, 64 around each mark, the last 64 (with the ragged tail) -- and the union over the strides of one batch is what is
gathered on the device and compared with the oracle.

Scenario.  64 shared task rows (env i plays row i % 64): rt20 targets, a third of the rows with a starting grid, every
row with its own initial pose, looking down at the ground in front of the agent so that placing works from the first
step.  Walking actions are igw_fill_actions_walking's counter RNG (restated here in numpy), flying actions a counter hash
that numpy and torch compute alike."""
import functools
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from gridworld_amd import _lib as L

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
MARKS = (1 << 31, 1 << 32)
SPAN = 64                      # envs per window (one wavefront's worth of 64-lane groups, 16 blocks of 4-lane groups)


def header_int(path, name):
    """The integer a header or kernel source gives `name` (#define NAME v / constexpr int NAME = v)."""
    with open(os.path.join(ROOT, path)) as fh:
        text = fh.read()
    m = re.search(r'(?:#define\s+%s\s+|constexpr\s+int\s+%s\s*=\s*)(\d+)' % (name, name), text)
    assert m, f'{name} not found in {path}'
    return int(m.group(1))


# ---- bytes per row (include/igw.h through gridworld_amd/_lib.py) ---------------------------------------------------------
GRID_ROW = L.GRID_STRIDE                      # 1,104
HIST_ROW = 2 * L.HIST_ROW                     # 1,024: 512 uint16 bins
OCC_ROW = 4 * L.OCC_WORDS                     # 192
OUT_ROW, AGENT_ROW, AUX_ROW = L.OUT_BYTES, L.AGENT_BYTES, L.AUX_BYTES
STEP_STRIDES = (GRID_ROW, HIST_ROW, OUT_ROW)  # the strides whose windows the step tests gather
BLOCK = header_int('gridworld_amd/csrc/igw_device.h', 'IGW_BLOCK')
FLY_ENVS_PER_BLOCK = BLOCK // L.auto_lanes(1 << 22)   # 4-lane groups at this size: 64 envs per block

N_MARK = MARKS[1] // HIST_ROW                 # 2^22: the first env whose histogram row starts at or past 2^32
N_WALK = N_MARK + 101                         # a ragged last wavefront past the mark
N_FLY = N_MARK + 64                           # a whole number of blocks: the flying kernel's EXACT variant

# ---- the render, observation and codec launches --------------------------------------------------------------------------
SIZE = (64, 64)
CHUNK = header_int('gridworld_amd/csrc/render/igw_render_frame.h', 'kChunk')
SINK_SLOTS = header_int('gridworld_amd/csrc/render/igw_render_obs.hip', 'kSinkSlots')
MAX_STACK = header_int('include/igw_render_obs.h', 'IGW_RENDER_MAX_STACK')
FRAME_ROW = SIZE[0] * SIZE[1] * 3             # 12,288 bytes of RGB
DEPTH_ROW, SURFACE_ROW, LABEL_ROW = SIZE[0] * SIZE[1] * 4, SIZE[0] * SIZE[1] * 2, SIZE[0] * SIZE[1]
N_POV = -(-MARKS[1] // FRAME_ROW) + SPAN      # 349,526 + 64 frames: `out` passes 2^32, depth passes it at 262,144
OBS_STACK = MAX_STACK
OBS_ROW = OBS_STACK * FRAME_ROW * 4           # float32, RGB, K = 8: 393,216 bytes per env
N_OBS = -(-MARKS[1] // OBS_ROW) + SPAN        # 10,923 + 64 envs
JPEG_STRIDE = 1 << 20
N_JPEG = MARKS[1] // JPEG_STRIDE + 8          # 4,096 + 8 slots of 1 MiB


def windows(stride, n):
    """Sorted unique row indices of a buffer of n rows of `stride` bytes: the first 64, the 64 around each mark the
    buffer reaches (32 on either side of row floor(mark / stride), which holds or starts at the mark's byte), the last
    64 and with them the ragged tail past the last whole group of 64."""
    rows = set(range(min(SPAN, n)))
    for mark in MARKS:
        mid = mark // stride
        if mid < n:
            rows.update(range(max(mid - SPAN // 2, 0), min(mid + SPAN // 2, n)))
    rows.update(range(max(min(n - SPAN, n // SPAN * SPAN - SPAN), 0), n))
    return np.array(sorted(rows), np.int64)


def marks_in(stride, n):
    """The marks that a buffer of n rows of `stride` bytes reaches, each with the rows of its window."""
    return [(mark, np.arange(max(mark // stride - SPAN // 2, 0), min(mark // stride + SPAN // 2, n)))
            for mark in MARKS if mark // stride < n]


def step_windows(n):
    """The union of windows() over the grid, histogram and output strides of a batch of n envs."""
    return np.unique(np.concatenate([windows(s, n) for s in STEP_STRIDES]))


# ---- the scenario -----------------------------------------------------------------------------------------------------
NUM_TASKS = 64
T = 16                          # steps
MAX_STEPS = 9                   # the time limit ends every episode at step 9: seven steps of the second one follow
KW = dict(size_reward=False, max_steps=MAX_STEPS)
WALK_SEED, FLY_SEED, TASK_SEED = 90210, 31337, 64
MIN_TARGET = MAX_STEPS + 2      # a synthetic target this large cannot be finished inside the time limit (see tasks())


@functools.lru_cache(None)
def tasks():
    """(targets, starts int8 [64, 9, 11, 11], poses float64 [64, 5] as x, y, z, yaw, pitch).  Rows 0, 3, 6, ... start with
    four of their target's blocks standing and one block the target does not want (a negative synthetic id).  An
    episode ends before the time limit only when max_int reaches the synthetic target's size; max_int is 0 after a
    reset and a step changes one cell, so with at least MAX_STEPS + 2 blocks left no episode ends early and the
    whole batch's episode clock is known without stepping it."""
    from gridworld_amd import workloads
    targets = workloads.rt20(NUM_TASKS, seed=TASK_SEED).numpy().astype(np.int8)
    starts = np.zeros_like(targets)
    rng = np.random.RandomState(TASK_SEED)
    for r in range(0, NUM_TASKS, 3):
        cells = np.flatnonzero(targets[r])
        keep = rng.permutation(cells)[:4]
        starts[r].reshape(-1)[keep] = targets[r].reshape(-1)[keep]
        free = np.flatnonzero(targets[r, 0] == 0)
        starts[r, 0].reshape(-1)[rng.choice(free)] = 1 + r % 6
    # yaw and pitch on the step's 5-degree lattice (where libm and the device's table agree bit for bit); the eye looks
    # down at the ground two or three cells ahead
    poses = np.stack([rng.uniform(-3, 3, NUM_TASKS), np.zeros(NUM_TASKS), rng.uniform(-3, 3, NUM_TASKS),
                      5.0 * rng.randint(-36, 37, NUM_TASKS), 5.0 * rng.randint(-12, -6, NUM_TASKS)], 1)
    for a in (targets, starts, poses):
        a.setflags(write=False)
    return targets, starts, poses


def env_task(n):
    return (np.arange(n) % NUM_TASKS).astype(np.int32)


_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _splitmix64(z):
    z = (z + np.uint64(0x9E3779B97F4A7C15)) & _M64
    z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & _M64
    z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & _M64
    return z ^ (z >> np.uint64(31))


def walk_actions(envs, steps=T, seed=WALK_SEED):
    """int32 [steps, len(envs)]: what igw_fill_actions_walking(seed) gives env `envs[i]` at step t -- a host restatement
    of csrc/igw_device.h rng_action18() (the GPU test checks it against the gathered columns of the device's own)."""
    with np.errstate(over='ignore'):
        e = np.asarray(envs, np.uint64)[None, :]
        t = np.arange(steps, dtype=np.uint64)[:, None]
        h = _splitmix64(np.uint64(seed) ^ _splitmix64(e * np.uint64(0x100000001B3) + t))
        return (((h >> np.uint64(32)) * np.uint64(18)) >> np.uint64(32)).astype(np.int32)


def _mix32(h):
    """murmur3's 32-bit finaliser on int64 arrays / tensors that hold values below 2^32 (products wrap in 64 bits; the
    mask keeps their low 32 bits, which a wrap leaves right): the same integers from numpy and from torch."""
    m = 0xFFFFFFFF
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & m
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & m
    return h ^ (h >> 16)


def fly_actions(envs, t, seed=FLY_SEED):
    """The flying action of step t for the envs `envs` (a numpy int64 array or a torch int64 tensor, on any device):
    dict(movement f32 [n, 3] in [-1, 1), camera f32 [n, 2] in [-5, 5), inventory i32 [n] in 0..6, placement i32 [n] in
    0..2).  24-bit fractions, so the float32 values are exact in either library."""
    torch_side = not isinstance(envs, np.ndarray)
    e = envs.reshape(-1, 1)
    if torch_side:
        import torch
        c = torch.arange(7, dtype=torch.int64, device=envs.device).reshape(1, 7)
    else:
        c = np.arange(7, dtype=np.int64).reshape(1, 7)
    with np.errstate(over='ignore'):
        h = _mix32(_mix32((e * 0x9E3779B1 + seed) & 0xFFFFFFFF) ^ ((c * 0x85EBCA77 + t * 0xC2B2AE3D + 0x27D4EB2F) & 0xFFFFFFFF))
    frac = h >> 8                                       # 24 bits
    if torch_side:
        u = frac.to(torch.float64) / float(1 << 24)
        f32, i32 = (lambda x: x.to(torch.float32).contiguous()), (lambda x: x.to(torch.int32).contiguous())
    else:
        u = frac.astype(np.float64) / float(1 << 24)
        f32, i32 = (lambda x: np.ascontiguousarray(x, np.float32)), (lambda x: np.ascontiguousarray(x, np.int32))
    return dict(movement=f32(u[:, 0:3] * 2.0 - 1.0), camera=f32(u[:, 3:5] * 10.0 - 5.0),
                inventory=i32((frac[:, 5] * 7) >> 24), placement=i32((frac[:, 6] * 3) >> 24))


def oracle_batch(envs, blocks=1, **kw):
    """An OracleBatch of `blocks` copies of the scenario's envs `envs` (global indices: env i plays row i % 64), reset."""
    from oracle import oracle as O
    targets, starts, poses = tasks()
    rows = np.tile(np.asarray(envs) % NUM_TASKS, blocks)
    ob = O.OracleBatch(len(rows), **dict(KW, **kw))

    def prepare(lo):   # (Task.__init__ is most of the cost; the oracle's envs share nothing and its calls release the lock)
        for i in range(lo, min(lo + 64, len(rows))):
            e = ob.envs[i]
            e.set_task(targets[rows[i]], starts[rows[i]])
            e.set_initial_pose(poses[rows[i]])
            o = e.reset()
            ob.agentPos[i], ob.inventory[i], ob.compass[i] = o['agentPos'], o['inventory'], o['compass'][0]
            ob.grid[i] = o['grid'].reshape(-1)
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
        list(pool.map(prepare, range(0, len(rows), 64)))
    return ob


def replay(mode, envs):
    """The scenario's T steps of the envs `envs` on the oracle alone: (ob, done uint8 [T, n], changed bool [T, n] --
    the step changed the env's grid row, auto-reset included)."""
    from oracle import oracle as O
    envs = np.asarray(envs, np.int64)
    ob = oracle_batch(envs, **({'action_space': 'flying'} if mode == 'flying' else {}))
    done, changed = np.zeros((T, len(envs)), np.uint8), np.zeros((T, len(envs)), bool)
    acts = walk_actions(envs) if mode == 'walking' else None
    O.use_device_trig(mode == 'flying')
    try:
        for t in range(T):
            before = ob.grid.copy()
            if mode == 'walking':
                ob.step_walking(acts[t], autoreset=True, nthreads=8)
            else:
                a = fly_actions(envs, t)
                ob.step_flying(a['movement'], a['camera'], a['inventory'], a['placement'], autoreset=True, nthreads=8)
            done[t], changed[t] = ob.done, (ob.grid != before).any(1)
    finally:
        O.use_device_trig(False)
    return ob, done, changed


class Gathered:
    """Rows `idx` (a device int64 tensor) of a VecGridWorld's records, gathered on the device: the buffers under their
    names and VecGridWorld._make_views' observation views over the copies, so that what compares a whole small batch
    (fuzz_parity.compare, test_gpu_parity._check_occ / _check_hist, internals(), task_state()) compares these rows."""

    def __init__(self, env, idx, state=True):
        import torch
        self.num_envs = n = int(idx.numel())
        self.out_buf, self.grid_buf = env.out_buf[idx], env.grid_buf[idx]
        f = self.out_buf.view(torch.float32)
        self.agent_pos, self.inventory, self.compass, self.reward = f[:, 0:5], f[:, 5:11], f[:, 11], f[:, 12]
        self.done = self.out_buf[:, 52]
        self.grid = self.grid_buf[:, :L.CELLS].reshape(n, 9, 11, 11)
        if state:
            self.agent_buf, self.aux_buf = env.agent_buf[idx], env.aux_buf[idx]
            self.occ_buf, self.hist_buf = env.occ_buf[idx], env.hist_buf[idx]

    def internals(self):
        from gridworld_amd import VecGridWorld
        return VecGridWorld.internals(self)

    def task_state(self):
        from gridworld_amd import VecGridWorld
        return VecGridWorld.task_state(self)
