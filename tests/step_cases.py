"""Directed scenarios of the step path (CPU only; no GPU, no reference needed to build them).

Random walks near the origin leave most of the rare situations of the reference's physics unvisited
(profiles/r15_step_census.json: what every fixture, the parity scenarios and 100 fuzz cases never reach).  These cases
are scripted to land in them, one situation each, and together they reach every bin of tests/step_census.py and -- with
the older scenarios -- every branch outcome of the step path except those of UNREACHABLE below.

A case is a dict: name, space ('walking' = Discrete(18), 'flying'), target and start (dense int8 [9, 11, 11]), pose
(x, y, z, yaw, pitch; inside set_tasks' validated range) and its scripted actions: int32 [T] for walking, for flying
a dict(movement f32 [T, 3], camera f32 [T, 2], inventory i32 [T], placement i32 [T]).  Scripts are as long as their
situation needs; batch() pads the shorter ones with no-ops.  All angles are multiples of five degrees and all walking
cases stay on Discrete(18)'s lattice, where the reference's libm and the kernels' table agree bit for bit; the flying
cases are recorded from the reference with correctly rounded trig and stepped by the oracle in device-trig mode, as
s4_fly_crlibm is.

Geometry used below: yaw 0 looks along -z, 90 along +x, 180 along +z, 270 along -x; pitch +90 is up.  An agent standing
on the ground has its eye at y = -0.25, its head in cell y = 0 and its legs in cell y = -1; grid level = y + 1.
"""
import functools

import numpy as np

# Bins and branch outcomes no scenario can reach, each with the reason.  tests/test_step_census_cpu.py asserts that
# everything else IS reached and that everything named here is NOT (so a stale entry fails as well).
UNREACHABLE = {
    'hit.bottom.level-1':
        'the cell under a block of the lowest level is the ground plane (y = -2 under the whole zone): the ray stops there',
    'ray.reenters_zone':
        'every coordinate of the samples is monotone along the ray and rint() is monotone, so the samples whose key lies '
        'inside the (box-shaped) zone are one run: a ray that has left the zone stays outside',
    'agent.off_ground_plane':
        'update_substep moves an agent sideways only to a candidate within the zone padded by 2 (|x|, |z| <= 7), so '
        '|x|, |z| never exceed the larger of 7 and the initial pose, which set_tasks bounds by 10: nobody walks or '
        'flies off the 37 x 37 ground plane',
    'world_lookup | if (x < -18 || x > 18 || z < -18 || z > 18) return 0; | branch 1':
        'same reason: agents stay within |x|, |z| <= 10, collide looks one cell further, a sight ray 7.8 further',
    'world_lookup | if (x < -18 || x > 18 || z < -18 || z > 18) return 0; | branch 3': 'as branch 1',
    'world_lookup | if (x < -18 || x > 18 || z < -18 || z > 18) return 0; | branch 5': 'as branch 1',
    'world_lookup | if (x < -18 || x > 18 || z < -18 || z > 18) return 0; | branch 6': 'as branch 1',
    'update | dt = dt < 0.2 ? dt : 0.2; | branch 1':
        'world_step always calls update(1 / 20.): the clamp of dt never acts',
    'grid_set | if (build_zone(pos[0], pos[1], pos[2], 0)) | branch 1':
        'a place reaches grid_set only after build_zone(previous) held, a break only for a block found in the grid',
}

TARGET_CORNER = (5, 7, 5, 1)    # a block no script places: episodes end by max_steps alone


def dense(blocks):
    g = np.zeros((9, 11, 11), np.int8)
    for x, y, z, c in blocks:
        g[y + 1, x + 5, z + 5] = c
    return g


def walking(name, pose, script, start=(), target=None):
    start = list(start)
    return dict(name=name, space='walking', start=dense(start), pose=np.asarray(pose, np.float64),
                target=dense(start + [TARGET_CORNER] if target is None else target),
                actions=np.asarray(script, np.int32))


def flying(name, pose, steps, start=(), target=None):
    """steps: [(movement3, camera2, inventory, placement)]"""
    start = list(start)
    return dict(name=name, space='flying', start=dense(start), pose=np.asarray(pose, np.float64),
                target=dense(start + [TARGET_CORNER] if target is None else target),
                actions=dict(movement=np.asarray([s[0] for s in steps], np.float32).reshape(-1, 3),
                             camera=np.asarray([s[1] for s in steps], np.float32).reshape(-1, 2),
                             inventory=np.asarray([s[2] for s in steps], np.int32),
                             placement=np.asarray([s[3] for s in steps], np.int32)))


FWD, BACK, LEFT, RIGHT, JUMP, BREAK, PLACE, NOOP = 1, 2, 3, 4, 5, 16, 17, 0
YAW_L, YAW_R, DOWN, UP = 12, 13, 14, 15


def _face_poses(x, y, z):
    """side of the block at (x, y, z) -> a pose two cells from it, looking straight at it"""
    return {'top': (x, y + 2, z, 0, -90), 'bottom': (x, y - 1.4, z, 0, 90),
            'xlo': (x - 2, y, z, 90, 0), 'xhi': (x + 2, y, z, 270, 0),
            'zlo': (x, y, z - 2, 180, 0), 'zhi': (x, y, z + 2, 0, 0)}


def _faces():
    """Every side of a block on every level: one floating block, place against the side, break what was placed, break
    the block.  The side places land on every level 0..8; the place on top of level 8 is refused by the ceiling."""
    out = []
    for y in range(-1, 8):
        for side, pose in _face_poses(0, y, 0).items():
            if side == 'bottom' and y == -1:
                continue
            out.append(walking(f'face_{side}_level{y}', pose, [PLACE, BREAK, BREAK, BREAK], start=[(0, y, 0, 2)]))
    return out


def _walls():
    """Places through each wall from the last cell inside (the ray ends on the ground outside), from below the ground
    (floor) and rays from outside the zone back into it."""
    out = [walking('wall_xhi', (4.75, -0.25, 0, 90, -30), [PLACE, BREAK, 7]),
           walking('wall_xlo', (-4.75, -0.25, 0, 270, -30), [PLACE, BREAK, 8]),
           walking('wall_zlo', (0, -0.25, -4.75, 0, -30), [PLACE, BREAK, 9]),
           walking('wall_zhi', (0, -0.25, 4.75, 180, -30), [PLACE, BREAK, 10]),
           # below the ground plane, looking up at it: the place is refused by the floor; then free fall: terminal
           # velocity after 50 steps, every occupancy key clamped from the first step on
           walking('under_ground_free_fall', (0, -5, 0, 0, 90), [PLACE, BREAK] + [NOOP, FWD, PLACE, BREAK, JUMP] * 11),
           walking('under_ground_outside', (-9, -3.5, 9.5, 45, 60), [PLACE, BREAK, JUMP] + [LEFT, UP, PLACE] * 6)]
    for name, pose, block in (('xhi', (8, 0, 0, 270, 0), (4, 0, 0, 3)), ('xlo', (-8, 0, 0, 90, 0), (-4, 0, 0, 3)),
                              ('zhi', (0, 0, 8, 0, 0), (0, 0, 4, 3)), ('zlo', (0, 0, -8, 180, 0), (0, 0, -4, 3))):
        # outside the padded zone a walking agent only falls: the moves are refused, the ray comes back into the zone
        out.append(walking(f'outside_{name}_looking_in', pose, [BREAK, FWD, FWD, PLACE, DOWN, DOWN, DOWN, PLACE, BREAK],
                           start=[block]))
    out.append(walking('ring_walk_out', (5.5, -0.25, 5.5, 135, -45), [FWD] * 10 + [PLACE, BREAK, BACK, BACK]))
    out.append(walking('corner_pose', (10, 0, -10, 315, -20), [PLACE, BREAK, FWD, RIGHT, JUMP, NOOP]))
    return out


def _collide():
    out = []
    for yaw, (dx, dz), face in ((0, (0, -1), 'zneg'), (180, (0, 1), 'zpos'), (90, (1, 0), 'xpos'), (270, (-1, 0), 'xneg')):
        out.append(walking(f'walk_into_{face}_legs', (0, -0.25, 0, yaw, 0), [FWD] * 5 + [JUMP, FWD, FWD], start=[(dx, -1, dz, 4)]))
        out.append(walking(f'walk_into_{face}_head', (0, -0.25, 0, yaw, 0), [FWD] * 5 + [BACK, LEFT], start=[(dx, 0, dz, 4)]))
    # a ceiling at head height, jumps under it; a head / legs inside a block
    ceiling = [(x, 1, z, 5) for x in (-1, 0, 1) for z in (-1, 0, 1)]
    out.append(walking('jump_under_ceiling', (0, -0.25, 0, 0, 0), [JUMP, NOOP, NOOP, FWD, JUMP, NOOP, UP, UP, BREAK, PLACE, JUMP], start=ceiling))
    out.append(walking('head_in_block', (0, 0.3, 0, 0, 0), [PLACE, BREAK, JUMP, NOOP], start=[(0, 0, 0, 5)]))
    out.append(walking('legs_in_block', (0, -0.3, 0, 0, 0), [NOOP, JUMP, NOOP], start=[(0, -1, 0, 5)]))
    # a drop from the top of the validated range: 12 sub-steps, terminal velocity just above the ground
    out.append(walking('drop_from_64', (0, 64, 0, 0, -90), [NOOP] * 48 + [PLACE, NOOP, NOOP, NOOP, BREAK, NOOP, NOOP, NOOP]))
    out.append(walking('drop_onto_block', (2, 30, 2, 0, -90), [NOOP] * 36, start=[(2, 3, 2, 6)]))
    return out


def _towers():
    pillar8 = [(0, y, 0, 1) for y in range(-1, 7)]
    top = dense(pillar8 + [(0, 7, 0, 1)])
    return [
        # on a tower up to level 7: a place into the own legs, a jump, the place on level 8 as soon as the feet are clear
        # (it completes the target: the episode ends mid-script), from there the ceiling refuses
        walking('tower_place_level8', (0, 7.75, 0, 0, -90), [PLACE, JUMP] + [PLACE] * 12, start=pillar8,
                target=[(0, y, 0, 1) for y in range(-1, 8)]),
        walking('tower_ceiling', (0, 9.25, 0, 0, -90), [PLACE, PLACE, BREAK, NOOP, NOOP, PLACE],
                start=pillar8 + [(0, 7, 0, 1)], target=[(x, y, z, c) for (x, y, z, c) in pillar8] + [(0, 7, 0, 2)]),
        # a pillar broken from under the agent, block by block, then the ground
        walking('pillar_broken_from_under', (0, 2.75, 0, 0, -90), ([BREAK] + [NOOP] * 5) * 3 + [BREAK, PLACE, BREAK],
                start=[(0, y, 0, 3) for y in range(-1, 2)]),
        dict(walking('above_the_zone', (3, 12, -3, 90, -90), [NOOP] * 4 + [PLACE, BREAK], start=[(3, 7, -3, 2)]), target=top),
    ]


def _inventory():
    floor20 = [(x, -1, z, 1) for x in range(-5, 5) for z in (3, 4)]
    floor30 = [(x, -1, z, 2) for x in range(-5, 5) for z in (3, 4, 5)]
    look = [DOWN] * 9
    return [walking('empty_slot', (0, -0.25, 0, 0, 0), look + [PLACE, BREAK, PLACE, 7, PLACE], start=floor20),
            walking('negative_slot', (0, -0.25, 0, 0, 0), look + [7, BREAK, PLACE, 6, PLACE], start=floor30),
            walking('nothing_in_reach', (0, -0.25, 0, 0, 90), [PLACE, BREAK, 11, UP, YAW_L, YAW_L]),   # pitch clamped, yaw wraps
            walking('yaw_wrap_down', (0, -0.25, 0, 360, -90), [YAW_R, DOWN, YAW_R, BREAK])]


def _ties():
    """Coordinates on rounding ties (fraction exactly .5, both signs): the pose itself, every sample of a ray along a
    cell boundary, and the ray's end points."""
    return [walking('tie_positive', (0.5, -0.25, 2.5, 0, 0), [BREAK, PLACE, NOOP, FWD, BREAK], start=[(0, 0, 0, 2), (1, 0, 0, 3)]),
            walking('tie_negative', (-0.5, -0.25, -2.5, 180, 0), [BREAK, PLACE, NOOP, FWD, BREAK], start=[(0, 0, 0, 2), (-1, 0, 0, 3)]),
            walking('diagonal', (0, -0.25, 0, 135, 0), [PLACE, BREAK, BREAK], start=[(1, 0, 1, 2)]),   # the ray crosses a cell's edge
            walking('tie_height', (1.5, 0.5, -1.5, 90, 0), [PLACE, BREAK, NOOP, NOOP, BREAK], start=[(4, 0, -1, 2), (4, 1, -2, 3), (4, 0, -2, 4)]),
            walking('tie_edge_of_zone', (5.5, -0.25, -5.5, 270, 0), [PLACE, BREAK, LEFT, RIGHT], start=[(3, 0, -5, 2), (3, 0, -4, 2)])]


def _flying():
    z3, c0 = (0, 0, 0), (0, 0)
    tower = [(2, y, 0, 4) for y in range(-1, 8)]
    return [
        # forward / back along the sight line (strafe[1] == 0: the vertical component survives), both signs
        flying('fly_along_sight', (0, 2, 0, 0, 30), [((-1, 0, 0), c0, 0, 0), ((1, 0, 0), c0, 0, 0), ((-1, 0, 0), (5, -5), 0, 0),
                                                     ((1, 0, 0), c0, 3, 0), ((-1, 0, 0), (0, -60), 0, 1), (z3, c0, 0, 2)]),
        # an ascent with a sideways strafe, then a descent onto the ground
        flying('fly_ascent_strafe', (0, 0, 0, 90, 0), [((0, 1, 1), c0, 0, 0)] * 4 + [((0, -1, 1), (10, 0), 0, 0)] * 3 +
               [((1, 1, -1), c0, 0, 0)] * 6 + [(z3, (0, -45), 2, 0), (z3, c0, 0, 2), (z3, c0, 0, 2)]),
        # up along a tower to above the zone, a place against it on every level on the way, out through the ceiling
        flying('fly_up_the_tower', (0, -0.25, 0, 90, 0), [(z3, c0, 1 + k % 6, 1) if k % 2 == 0 else ((0, 0, 1), c0, 0, 0)
                                                            for k in range(36)] + [(z3, (0, -90), 0, 0), (z3, c0, 0, 2)], start=tower),
        # out of the zone sideways until the padded zone refuses the move, looking back in
        flying('fly_out_and_look_back', (4, 1, 0, 270, 0), [((0, 1, 0), c0, 0, 0)] * 8 + [((0, -1, 0), c0, 0, 0)] * 8 +
               [(z3, c0, 0, 2), (z3, c0, 5, 1)], start=[(0, 1, 0, 6)]),
        flying('fly_outside_pose', (-10, 5, 10, 135, -35), [(z3, c0, 0, 1), (z3, c0, 0, 2), ((-1, 0, 1), c0, 0, 0), ((1, 1, -1), (-30, 20), 1, 0)]),
        flying('fly_tie', (2.5, 3.5, -0.5, 270, 0), [(z3, c0, 0, 2), (z3, c0, 2, 1), ((0, 0, 1), c0, 0, 0), ((0, 0, -1), c0, 0, 2)], start=[(0, 4, 0, 6), (0, 3, -1, 5)]),
    ]


@functools.lru_cache(None)
def cases():
    out = _faces() + _walls() + _collide() + _towers() + _inventory() + _ties() + _flying()
    names = [c['name'] for c in out]
    assert len(set(names)) == len(names)
    for c in out:
        p = c['pose']
        assert abs(p[0]) <= 10 and abs(p[2]) <= 10 and abs(p[1]) <= 64 and (p[3:] % 5 == 0).all(), c['name']
    return tuple(out)


def length(case):
    a = case['actions']
    return len(a['inventory'] if isinstance(a, dict) else a)


def batch(space):
    """The cases of one action space as one batch: dict(names, kw, targets, starts, poses, actions, T).  Every script is
    padded with no-ops to T = max_steps + 3 steps, max_steps being the longest script: every env runs into the time
    limit once and takes its first steps of a second episode."""
    cs = [c for c in cases() if c['space'] == space]
    max_steps = max(length(c) for c in cs)
    T = max_steps + 3
    n = len(cs)
    if space == 'walking':
        actions = np.zeros((T, n), np.int32)
        for i, c in enumerate(cs):
            actions[:length(c), i] = c['actions']
    else:
        actions = dict(movement=np.zeros((T, n, 3), np.float32), camera=np.zeros((T, n, 2), np.float32),
                       inventory=np.zeros((T, n), np.int32), placement=np.zeros((T, n), np.int32))
        for i, c in enumerate(cs):
            for k, v in c['actions'].items():
                actions[k][:length(c), i] = v
    kw = dict(size_reward=False, max_steps=max_steps)
    if space == 'flying':
        kw['action_space'] = 'flying'
    return dict(names=[c['name'] for c in cs], kw=kw, targets=np.stack([c['target'] for c in cs]),
                starts=np.stack([c['start'] for c in cs]), poses=np.stack([c['pose'] for c in cs]), actions=actions, T=T)


def actions_at(b, t, idx=None):
    """The batch's actions of step t (for the envs idx), as OracleBatch.step_walking / step_flying take them."""
    a = b['actions']
    sel = (lambda v: v[t]) if idx is None else (lambda v: v[t][idx])
    if isinstance(a, dict):
        return tuple(sel(a[k]) for k in ('movement', 'camera', 'inventory', 'placement'))
    return (sel(a),)


def run_oracle(O, b, idx=None, record=False):
    """Steps the batch (or its envs idx, repeats allowed) on the oracle module O with the in-step auto-reset, device
    trig for the flying batch.  Yields per step (t, OracleBatch) -- or, with record, returns the arrays of every step."""
    idx = np.arange(len(b['names'])) if idx is None else np.asarray(idx)
    kw = dict(b['kw'])
    ob = O.OracleBatch(len(idx), **kw)
    ob.set_tasks(b['targets'][idx], b['starts'][idx])
    ob.set_initial_pose(b['poses'][idx])
    flying = kw.get('action_space') == 'flying'
    O.use_device_trig(flying)
    try:
        ob.reset()
        for t in range(b['T']):
            a = actions_at(b, t, idx)
            (ob.step_flying if flying else ob.step_walking)(*a, autoreset=True)
            yield t, ob
    finally:
        O.use_device_trig(False)


def record(O, b):
    """Every step's outputs of the batch on oracle module O: dict of arrays over [T, n, ...]."""
    keys = ('agentPos', 'inventory', 'compass', 'reward', 'done', 'grid')
    out = {k: [] for k in keys + ('internal',)}
    for t, ob in run_oracle(O, b):
        for k in keys:
            out[k].append(getattr(ob, k).copy())
        out['internal'].append(ob.internals())
    return {k: np.stack(v) for k, v in out.items()}


FIXTURE = 'golden/s14_step_cases.npz'


def against_fixture(O, space, fixture):
    """The oracle (module O) through the batch of `space` the way the reference was recorded (one env per case, an
    episode that ended is reset before the next step): every field of tests/golden/s14_step_cases.npz bit for bit.
    Returns the number of env-steps compared."""
    b = batch(space)
    fx = {k[len(space) + 1:]: fixture[k] for k in fixture.files if k.startswith(space + '_')}
    flying = space == 'flying'
    O.use_device_trig(flying)
    try:
        for i, name in enumerate(b['names']):
            env = O.OracleEnv(**b['kw'])
            env.set_task(b['targets'][i], b['starts'][i])
            env.set_initial_pose(b['poses'][i])
            env.reset()
            done = False
            for t in range(b['T']):
                where = f'{name} step {t}'
                assert bool(fx['reset_before'][i, t]) == done, where + ' episode boundary'
                if done:
                    env.reset()
                a = actions_at(b, t, i)
                act = dict(movement=a[0], camera=a[1], inventory=a[2], placement=a[3]) if flying else int(a[0])
                obs, reward, done, _ = env.step(act)
                assert np.float64(reward).tobytes() == fx['reward'][i, t].tobytes() and done == bool(fx['done'][i, t]), where + ' reward / done'
                assert np.array_equal(obs['grid'].reshape(-1), fx['grid'][i, t]), where + ' grid'
                assert np.array_equal(obs['inventory'], fx['inventory'][i, t]), where + ' inventory'
                assert obs['agentPos'].tobytes() == fx['agentPos'][i, t].tobytes(), where + f" agentPos {obs['agentPos']} vs {fx['agentPos'][i, t]}"
                assert obs['compass'][0].tobytes() == fx['compass'][i, t].tobytes(), where + ' compass'
                assert env.internal().tobytes() == fx['internal'][i, t].tobytes(), where + f" internals {env.internal()} vs {fx['internal'][i, t]}"
    finally:
        O.use_device_trig(False)
    return len(b['names']) * b['T']
