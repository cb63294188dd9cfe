"""The cases the aim tests share (tests/test_aim_cpu.py, tests/test_gpu_aim.py) and their truth, from the CPU oracle
(DESIGN.md section 12).  Two yardsticks:

The probe is the oracle itself.  For a state (a grid and x, y, z, yaw, pitch) and every direction (di, dj) of the window
an oracle env whose starting grid is that grid is reset at the pose (x, y, z, yaw + 5 di, pitch + 5 dj) and takes one
step of 17; a second one takes 16.  The one grid cell that changed is that direction's place / break cell, and the
per-cell minimum of the directions' codes is the truth.  (One env per action is reused over the directions: reset()
restores the starting grid, the inventory and the pose, which is asserted.)  The grids keep every colour at 19 or fewer
blocks, so that the fresh inventory never refuses a place.

The model is a plain restatement of include/igw_aim.h in numpy: Python floats, math.sin / math.cos of math.radians (on
the 5-degree lattice these agree with the device's table bit for bit, see mask_cases._poses), np.rint, the ground plane
at y = -2 for x, z in -18..18.  It exists because the probe costs about a millisecond per direction; the two are
compared by tests/test_aim_cpu.py.

States: mask_cases.cases(), 32 envs each, at checkpoints 0, 12 and 25 of the case's action stream (the oracle stepped
there: its grid and internals()), and one directed case of eight envs (directed())."""
import functools
import math

import numpy as np

import mask_cases as MC

CHECKPOINTS = (0, 12, 25)
HALF, ROW, CELLS, MAX_TURNS = 36, 1104, 1089, 72
KW = MC.KW
DIRECTED_E = 8


def directed():
    """Eight envs on a grid with a wall, a tower and a roof block:
      0, 1  stand on the ground at pitch -90 / -85: `previous` is the cell they stand in, the overlap refuses
      2     stands at the zone's edge looking out and down: `previous` lies outside the build zone
      3, 4  start with the eye inside a block: the ray's first sample hits, there is no `previous`
      5     stands under a block and looks straight up at its underside (pitch 90)
      6     pitch -90 in the air above the tower; 7 pitch 90 in the zone's corner.
    Envs 0, 1 and 7 have a lone block seven cells straight behind them, narrower than the 10 degrees between di = -35 and
    di = 35: only di = -36 reaches it (the wrap).  They keep their yaw and move the pitch by 5 degrees a step (0 and 1
    up, 7 down); the others turn left at every step."""
    starts = np.zeros((DIRECTED_E, 9, 11, 11), np.int8)
    for i in range(DIRECTED_E):
        starts[i, 0:2, 8, 2:9] = 1 + i % 6          # a wall at x = 3, three high (no colour has more than 19 blocks)
        starts[i, 2, 8, 2:9] = 1 + (i + 1) % 6
        starts[i, 0:2, 1, 1] = 1 + (i + 1) % 6      # a tower at (-4, -4), two high
    starts[0, 0, 5, 9] = 3                          # (0, -1, 4): behind env 0, which looks along -z
    starts[1, 0, 0, 9] = 4                          # (-5, -1, 4): behind env 1, which looks along +x
    starts[7, 0, 10, 3] = 5                         # (5, -1, -2): behind env 7, which looks along +z
    starts[3, 1, 7, 7] = 3                          # (2, 0, 2): env 3's eye
    starts[4, 1, 3, 6] = 4                          # (-2, 0, 1): env 4's eye
    starts[5, 3, 3, 3] = 5                          # (-2, 2, -2): above env 5
    poses = np.array([[0.0, 0.0, -3.0, 0.0, -90.0],
                      [2.0, 0.0, 4.0, 90.0, -85.0],
                      [4.6, 0.0, 0.0, 90.0, -25.0],
                      [2.0, 0.0, 2.0, 0.0, -30.0],
                      [-2.1, 0.0, 1.2, -45.0, 10.0],
                      [-2.0, 0.0, -2.0, 180.0, 90.0],
                      [-4.0, 3.0, -4.0, 0.0, -90.0],
                      [5.0, 0.0, 5.0, 180.0, 90.0]])
    targets = np.zeros_like(starts)
    targets[:, 0, 5, 5] = 1
    actions = np.full((MC.T, DIRECTED_E), 12, np.int32)
    actions[:, [0, 1]], actions[:, 7] = 15, 14
    return dict(kw=dict(KW), targets=targets, starts=starts, poses=poses, actions=actions)


@functools.lru_cache(None)
def cases():
    """name -> case (mask_cases.cases() and 'directed')."""
    return dict(MC.cases(), directed=directed())


@functools.lru_cache(None)
def states(name):
    """(grids int8 [C, E, 9, 11, 11], poses float64 [C, E, 5] as x, y, z, yaw, pitch, internals float64 [C, E, 8]) of the
    named case at CHECKPOINTS, from stepping the oracle (read-only, computed once)."""
    case = cases()[name]
    ob = MC.oracle_batch(case)
    E = len(case['targets'])
    grids, inter = [], []
    for t in range(CHECKPOINTS[-1] + 1):
        if t in CHECKPOINTS:
            grids.append(ob.grid.reshape(E, 9, 11, 11).copy())
            inter.append(ob.internals())
        ob.step_walking(case['actions'][t], nthreads=8)
    grids, inter = np.stack(grids), np.stack(inter)
    poses = inter[..., :5].copy()
    for a in (grids, poses, inter):
        a.setflags(write=False)
    return grids, poses, inter


def all_states():
    """Every (name, checkpoint index, env, grid, pose) of every case."""
    for name in cases():
        grids, poses, _ = states(name)
        for c in range(len(CHECKPOINTS)):
            for e in range(grids.shape[1]):
                yield name, c, e, grids[c, e], poses[c, e]


def code_of(di, dj):
    return (abs(di) + abs(dj)) << 16 | (dj + HALF) << 8 | (di + HALF)


def window(pitch, max_turns):
    """(di, dj) int arrays of the directions that exist and cost at most max_turns, dj-major."""
    dj, di = np.meshgrid(np.arange(-HALF, HALF + 1), np.arange(-HALF, HALF), indexing='ij')
    pd = float(pitch) + 5.0 * dj
    keep = (np.abs(di) + np.abs(dj) <= max_turns) & (pd >= -90.0) & (pd <= 90.0)
    return di[keep], dj[keep]


def _planes(cells, codes):
    """The per-cell unsigned minimum of `codes` over the directions whose cell (`cells`, -1 = none) it is, as int32."""
    plane = np.full(CELLS, 0xffffffff, np.uint32)
    ok = cells >= 0
    np.minimum.at(plane, cells[ok], codes[ok].astype(np.uint32))
    return plane.view(np.int32)


# ---- the model ---------------------------------------------------------------------------------------------------------
def model(grid, pose, max_turns=MAX_TURNS):
    """include/igw_aim.h restated: dict(place, brk int32 [1089]; di, dj, place_cell, break_cell per direction (-1 = none);
    overlap, off_zone bool per direction: `previous` exists but the agent stands in it / it lies outside the zone)."""
    px, py, pz, yaw, pitch = (float(v) for v in pose)
    di, dj = window(pitch, max_turns)
    # the sight vector, one libm evaluation per lattice angle
    ycs = {d: (math.cos(math.radians((yaw + 5.0 * d) - 90.0)), math.sin(math.radians((yaw + 5.0 * d) - 90.0)))
           for d in range(-HALF, HALF)}
    pcs = {d: (math.cos(math.radians(pitch + 5.0 * d)), math.sin(math.radians(pitch + 5.0 * d)))
           for d in range(-HALF, HALF + 1)}
    cy, sy = (np.array([ycs[d][k] for d in di]) for k in (0, 1))
    m, vy = (np.array([pcs[d][k] for d in dj]) for k in (0, 1))
    vx, vz = cy * m, sy * m
    sx, sy_, sz = vx / 5.0, vy / 5.0, vz / 5.0
    # the world: the ground plane and the grid's blocks, y = -2..7, x and z = -18..18
    world = np.zeros((10, 37, 37), bool)
    world[0] = True
    world[1:, 13:24, 13:24] = np.asarray(grid).reshape(9, 11, 11) != 0
    n = len(di)
    x, y, z = np.full(n, px), np.full(n, py), np.full(n, pz)
    hit, have_prev = np.zeros(n, bool), np.zeros(n, bool)
    block, prev, last = np.zeros((n, 3), np.int64), np.zeros((n, 3), np.int64), None
    for s in range(40):
        key = np.stack([np.rint(x), np.rint(y), np.rint(z)], 1).astype(np.int64)
        inside = (np.abs(key[:, 0]) <= 18) & (np.abs(key[:, 2]) <= 18) & (key[:, 1] >= -2) & (key[:, 1] <= 7)
        k = np.where(inside[:, None], key, 0)
        in_world = inside & world[k[:, 1] + 2, k[:, 0] + 18, k[:, 2] + 18]
        new = ~hit & in_world & (True if last is None else (key != last).any(1))
        block[new] = key[new]
        if last is not None:
            prev[new], have_prev[new] = last[new], True
        hit |= new
        last = key
        x, y, z = x + sx, y + sy_, z + sz
    zone = lambda c: (np.abs(c[:, 0]) <= 5) & (np.abs(c[:, 2]) <= 5) & (c[:, 1] >= -1) & (c[:, 1] < 8)  # noqa: E731
    cell = lambda c: (c[:, 1] + 1) * 121 + (c[:, 0] + 5) * 11 + (c[:, 2] + 5)  # noqa: E731
    ay = py - 1.0 + 0.25
    bx, by, bz = prev[:, 0] - 0.5, prev[:, 1].astype(float), prev[:, 2] - 0.5
    overlap = (bx <= px) & (px <= bx + 1) & (bz <= pz) & (pz <= bz + 1) & \
        (((by <= ay) & (ay <= by + 1)) | ((by <= ay + 1) & (ay + 1 <= by + 1)))
    cand = hit & have_prev
    place_ok = cand & zone(prev) & ~overlap
    break_ok = hit & (block[:, 1] != -2)
    assert zone(block[break_ok]).all()
    place_cell = np.where(place_ok, cell(prev), -1)
    break_cell = np.where(break_ok, cell(block), -1)
    codes = (np.abs(di) + np.abs(dj)) << 16 | (dj + HALF) << 8 | (di + HALF)
    return dict(place=_planes(place_cell, codes), brk=_planes(break_cell, codes), di=di, dj=dj, codes=codes,
                place_cell=place_cell, break_cell=break_cell, overlap=cand & zone(prev) & overlap,
                off_zone=cand & ~zone(prev))


@functools.lru_cache(None)
def truth(name, max_turns):
    """(place, brk) int32 [C, E, 1104] of the named case from the model, pad words -1 (read-only, computed once)."""
    grids, poses, _ = states(name)
    C, E = grids.shape[:2]
    place, brk = np.full((C, E, ROW), -1, np.int32), np.full((C, E, ROW), -1, np.int32)
    for c in range(C):
        for e in range(E):
            m = model(grids[c, e], poses[c, e], max_turns)
            place[c, e, :CELLS], brk[c, e, :CELLS] = m['place'], m['brk']
    place.setflags(write=False)
    brk.setflags(write=False)
    return place, brk


# ---- the probe ---------------------------------------------------------------------------------------------------------
def probe(grid, pose, max_turns):
    """(place, brk) int32 [1089] of one state from the oracle alone.  Under oracle.use_device_trig(True) the oracle's trig
    is the device's, and the answer is the kernel's off the 5-degree lattice too."""
    from oracle import oracle as O
    grid = np.asarray(grid, np.int8).reshape(9, 11, 11).copy()
    if max(np.bincount(grid.reshape(-1).astype(np.int64), minlength=7)[1:]) > 19:
        # (the cells matter, not the colours: the same blocks with the six colours dealt out in turn)
        filled = np.flatnonzero(grid)
        grid.reshape(-1)[filled] = 1 + np.arange(len(filled)) % 6
    assert max(np.bincount(grid.reshape(-1).astype(np.int64), minlength=7)[1:]) <= 19, 'a colour has more than 19 blocks'
    px, py, pz, yaw, pitch = (float(v) for v in pose)
    target = np.zeros((9, 11, 11), np.int8)
    target[0, 5, 5] = 1
    envs = []
    for _ in range(2):
        e = O.OracleEnv(**KW)
        e.set_task(target, grid)
        envs.append(e)
    di, dj = window(pitch, max_turns)
    cells = np.full((2, len(di)), -1, np.int64)
    flat = grid.reshape(-1)
    for k, (a, b) in enumerate(zip(di, dj)):
        p5 = (px, py, pz, yaw + 5.0 * float(a), pitch + 5.0 * float(b))
        for j, (e, action) in enumerate(zip(envs, (17, 16))):
            e.set_initial_pose(p5)
            before = e.reset()['grid'].reshape(-1)
            assert np.array_equal(before, flat)
            assert np.array_equal(e.internal()[:5], p5)
            changed = np.flatnonzero(e.step(action)[0]['grid'].reshape(-1) != before)
            assert len(changed) <= 1
            if len(changed):
                cells[j, k] = changed[0]
    codes = (np.abs(di) + np.abs(dj)) << 16 | (dj + HALF) << 8 | (di + HALF)
    return _planes(cells[0], codes), _planes(cells[1], codes)
