"""Directed scenarios of the reward path (CPU only; no GPU, no reference needed to build them).

Random policies build near where they stand and almost never finish anything (profiles/r25_reward_census.json: the
reward situations every fixture, the parity scenarios, 100 fuzz cases and the directed step cases never reach).  These
cases are scripted to land in them, one situation each: completion at every rotation, at shifted and extreme
alignments and on the step the time limit ends as well, an empty synthetic task, a tower climbed to level 8, every
synthetic id -6..6, start blocks broken, restored and recoloured (the only way the reference's cached max_int goes
stale) with the recount that catches up by two in either direction, ties, drops of a unique and of a shared maximum, a
full one-colour level, a full-grid and a non-invariant user task, SizeReward on and off.  Together they reach every
reward bin of tests/step_census.py and -- with the older scenarios -- every branch outcome of the oracle's task
functions, except those of UNREACHABLE below.

A case is a dict: name, group, target and start (dense int8 [9, 11, 11]), full (the user task's full grid or None),
invariant, pose (x, y, z, yaw, pitch) and its Discrete(18) script.  With select_and_place (the default) action 5 + c
selects colour c and places it; 16 breaks; 12 / 13 turn by five degrees, 14 / 15 pitch by five.  All angles stay on the
five-degree lattice, where the reference's libm and the kernels' table agree bit for bit.  A group is one batch (one
env configuration): 'main' without SizeReward, 'size' with it; 'short' is the main group again under a time limit of
six steps, where completions, time limits and the in-step reset meet and the scripts run on into later episodes.

Geometry as in tests/step_cases.py: yaw 0 looks along -z, 90 along +x; an agent on the ground has its eye at y = -0.25;
grid level = y + 1.
"""
import functools

import numpy as np

from step_cases import dense

# Bins and branch outcomes no scenario can reach, each with the reason.  tests/test_reward_census_cpu.py asserts that
# everything else IS reached and that nothing named here is.  There is none: every reward bin is reached by the cases below
# and every branch outcome of the five task functions by them and the older scenarios together (the `argmax3` outcomes of
# task_maximal_intersection through oracle.task_eval, which the task-kernel tests are compared with).
UNREACHABLE = {}

YAW_L, YAW_R, DOWN, UP, BREAK, NOOP, JUMP = 12, 13, 14, 15, 16, 0, 5
P1, P2, P3, P4, P5, P6 = 6, 7, 8, 9, 10, 11     # select colour c and place it

GROUND = (0, -0.25, 0, 0, -30)     # on the ground at the origin, looking at the ground two cells along -z
PAIR = [(0, -1, 0, 1), (1, -1, 0, 2)]           # two colours: every rotation and translation of it is distinct
FLOOR = [(x, -1, z, 1) for x in range(-5, 6) for z in range(-5, 6)]


def row(z, colours):
    return [(x - 3, -1, z, c) for x, c in enumerate(colours, 1)]


def case(name, pose, script, target, start=(), full=None, invariant=True, group='main'):
    return dict(name=name, group=group, pose=np.asarray(pose, np.float64), actions=np.asarray(script, np.int32),
                target=dense(target), start=dense(start), full=None if full is None else dense(full), invariant=invariant)


def _completions():
    corner = [(-5, -1, -5, 1), (-4, -1, -5, 2)]
    return [
        # the pair built at each of its four orientations, away from where the target has it
        case('complete_rot0', GROUND, [P1] + [YAW_R] * 4 + [P2], PAIR),
        case('complete_rot3', GROUND, [P1, P2], PAIR),
        case('complete_rot2', (-2, -0.25, 3, 0, -30), [P1] + [YAW_L] * 4 + [P2], PAIR),
        case('complete_rot1', (3, -0.25, 3, 0, -30), [YAW_L] * 34 + [P1, P2], PAIR),
        case('complete_unshifted', (0, -0.25, 2, 0, -30), [P1] + [YAW_R] * 4 + [P2], PAIR),
        # a target in one corner built in the opposite one: the largest admissible shift along both axes
        case('complete_extreme', (4, -0.25, 3, 180, -30), [P1] + [YAW_L] * 4 + [P2], corner),
        case('complete_extreme_rot2', (-4, -0.25, -3, 0, -30), [P1] + [YAW_L] * 4 + [P2], corner),
        case('complete_extreme_rotated', (-3, -0.25, 4, 180, -30), [YAW_R] * 10 + [P2] + [YAW_R] * 5 + [P1], corner),
        # batch() puts no-ops in front of this script so that its last place falls on the group's max_steps
        case('complete_at_max_steps', (1, -0.25, 0, 90, -30), [P1] + [YAW_R] * 4 + [P2], PAIR),
        # target == start: max_int == target_size == 0, done on the first step whatever it does
        case('empty_task', GROUND, [17, BREAK, NOOP], [(0, -1, -2, 3), (1, 0, 1, 4)], start=[(0, -1, -2, 3), (1, 0, 1, 4)]),
    ]


def _levels():
    tower = [(0, y, 0, 1) for y in range(-1, 8)]
    out = [
        # jump, place under the feet as soon as they are clear (four refused places first), land: nine times
        case('tower_climb', (0, -0.25, 0, 0, -90), ([JUMP] + [P1] * 5 + [NOOP] * 3) * 9, tower),
        # a pillar of start blocks of every colour broken from under the agent, level 8 down to level 0
        case('tower_descend', (0, 8.75, 0, 0, -90), ([BREAK] + [NOOP] * 7) * 9, [(1, -1, 0, 2)],
             start=[(0, y, 0, 1 + (y + 1) % 6) for y in range(-1, 8)]),
    ]
    for lv in range(9):     # a place against a floating start block (a vote on that level), the placed block broken, the
        y, c = lv - 1, 1 + lv % 6       # start block broken; the far block keeps the episode from ending
        out.append(case(f'level{lv}', (3, y, 0, 270, 0), [5 + c, BREAK, BREAK], [(0, y, 0, 2), (1, y, 0, c), (-4, y, -4, c)], start=[(0, y, 0, 2)]))
    return out


def _ids():
    six = row(-2, range(1, 7))
    return [
        case('place_every_colour', GROUND, [P3] + [YAW_L] * 4 + [P2] + [YAW_R] * 8 + [P4] + [YAW_L] * 13 + [UP, P1] +
             [YAW_R] * 18 + [P5] + [YAW_R] * 3 + [UP, P6], six),
        # the target lacks the six start blocks: ids -1..-6, each break is a right placement
        case('remove_every_colour', GROUND, [BREAK] + [YAW_L] * 3 + [BREAK] + [YAW_R] * 6 + [BREAK] + [YAW_L] * 11 + [UP, BREAK] +
             [YAW_R] * 15 + [UP, BREAK] + [YAW_R] * 3 + [BREAK], [(0, -1, 3, 1)], start=six),
        # target colour over start colour in twelve cells: the differences -5..5; two of them recoloured to match
        case('recolour_every_difference', GROUND, [BREAK, P4] + [YAW_R] * 4 + [BREAK, P5],
             row(-2, [2, 3, 4, 5, 6, 6]) + row(-3, [1, 1, 1, 1, 2, 5]), start=row(-2, [1, 1, 1, 1, 1, 5]) + row(-3, [6, 5, 4, 3, 3, 6])),
    ]


def _cache():
    st, tg = [(0, -1, -2, 1)], [(0, -1, -2, 2), (1, -1, -2, 3)]
    return [
        # break a start block, another colour there (no vote: the cache stays right), break that, the same colour back
        case('restore_start', GROUND, [BREAK, P5, BREAK, P3], [(0, -1, -2, 3), (4, -1, 4, 1)], start=[(0, -1, -2, 3)]),
        # the target wants colour 2 where the start holds colour 1: the recolour is a vote the cache misses, the next
        # place recounts and pays for both (+2, and the structure is complete)
        case('stale_then_catch_up', GROUND, [BREAK, P2] + [YAW_R] * 4 + [P3], tg, start=st),
        # ... and down again: the recoloured block broken (missed), the other one broken (-2)
        case('stale_then_catch_down', GROUND, [BREAK, P2] + [YAW_R] * 4 + [P3, YAW_L, BREAK, BREAK], tg + [(-4, -1, -4, 4)], start=st),
        # a cell whose ids before and after the change both occur on that level of the synthetic target
        case('stale_votes_both', GROUND, [BREAK, P2, BREAK, P2] + [YAW_R] * 4 + [P4, BREAK], [(0, -1, -2, 2), (4, -1, 4, 3)],
             start=[(0, -1, -2, 1), (2, -1, 2, 1)]),
        # colour 3 over a broken colour-1 start block is synthetic id 2: it matches the plain colour-2 target cell next to
        # it under translation although the real target wants colour 1 there (a cell that cancels out of the synthetic task)
        case('alias_difference', GROUND, [BREAK, P3, P6, BREAK], [(0, -1, -2, 1), (1, -1, -2, 2), (-4, -1, 4, 5)], start=[(0, -1, -2, 1)]),
    ]


def _best():
    return [
        case('tie_iteration_order', GROUND, [P1] + [YAW_R] * 4 + [P1], [(0, -1, 0, 1), (1, -1, 0, 1), (0, -1, 1, 1)]),
        case('drop_unique', GROUND, [P1] + [YAW_R] * 4 + [P2, BREAK, YAW_L, BREAK], PAIR + [(0, -1, 1, 3)]),
        # two blocks that each match the one blue target cell: breaking either leaves the maximum standing
        case('drop_shared', GROUND, [P1] + [YAW_R] * 15 + [DOWN, P1] + [YAW_L] * 12 + [BREAK] + [YAW_R] * 12 + [BREAK], [(0, -1, 0, 1), (3, -1, 3, 2)]),
        case('wrong_colour', GROUND, [P5, BREAK], PAIR),
    ]


def _admissible():
    return [
        case('full_level', GROUND, [P1, BREAK], FLOOR),                                   # 121 votes, only the identity
        case('full_level_but_start', GROUND, [BREAK, P1, P1], FLOOR, start=[(0, -1, -2, 1)]),
        case('spans_x', GROUND, [P1], [(-5, -1, 0, 1), (5, -1, 0, 2)]),
        case('spans_z', GROUND, [P2], [(1, -1, -5, 1), (1, -1, 5, 2)]),
        case('full_grid_narrows', GROUND, [P1] + [YAW_R] * 4 + [P2], PAIR, full=PAIR + [(-3, 2, 4, 6), (4, 0, -2, 5)]),
        case('not_invariant', GROUND, [P1, P2], PAIR, invariant=False),
    ]


def _size_reward():
    return [
        # the start already holds two blocks of the target: SizeReward pays GridWorld.max_int once, on the first step
        case('size_reward_pays', GROUND, [NOOP, P4], PAIR + [(0, -1, -2, 4)], start=PAIR, group='size'),
        case('size_reward_zero', GROUND, [P1] + [YAW_R] * 4 + [P2], PAIR, group='size'),
    ]


@functools.lru_cache(None)
def cases():
    out = _completions() + _levels() + _ids() + _cache() + _best() + _admissible() + _size_reward()
    names = [c['name'] for c in out]
    assert len(set(names)) == len(names) < 80
    for c in out:
        p = c['pose']
        assert abs(p[0]) <= 10 and abs(p[2]) <= 10 and abs(p[1]) <= 64 and (p[3:] % 5 == 0).all(), c['name']
        assert len(c['actions']) < 120 and c['start'].max() <= 6 and c['target'].max() <= 6
    return tuple(out)


GROUPS = ('main', 'size', 'short')
SHORT_MAX_STEPS, SHORT_T = 6, 21


@functools.lru_cache(None)
def batch(group):
    """The cases of one group as one batch: dict(names, kw, targets, starts, fulls, invariant, poses, actions [T, n], T).
    Every script is padded with no-ops to T = max_steps + 3 steps, max_steps being the longest script, so every env runs
    into the time limit once and takes its first steps of a second episode; complete_at_max_steps is padded in front, so
    that its structure is complete on step max_steps.  'short' is the main group with max_steps = 6 over 21 steps: the
    six-step scripts complete on the time limit, longer ones are cut into episodes."""
    cs = [c for c in cases() if c['group'] == ('main' if group == 'short' else group)]
    longest = max(len(c['actions']) for c in cs)
    max_steps, T = (SHORT_MAX_STEPS, SHORT_T) if group == 'short' else (longest, longest + 3)
    actions = np.zeros((T, len(cs)), np.int32)
    for i, c in enumerate(cs):
        a = c['actions'][:T]
        lead = max_steps - len(a) if c['name'] == 'complete_at_max_steps' else 0
        actions[lead:lead + len(a), i] = a
    full = np.stack([c['target'] if c['full'] is None else c['full'] for c in cs])   # (its own target: as without one)
    return dict(names=[c['name'] for c in cs], kw=dict(size_reward=group == 'size', max_steps=max_steps),
                targets=np.stack([c['target'] for c in cs]), starts=np.stack([c['start'] for c in cs]), fulls=full,
                has_full=np.array([c['full'] is not None for c in cs]), invariant=np.array([c['invariant'] for c in cs]),
                poses=np.stack([c['pose'] for c in cs]), actions=actions, T=T)


def make_oracle(O, b, idx=None):
    """An OracleBatch of module O over the batch's envs idx (repeats allowed), tasks and poses set, reset."""
    idx = np.arange(len(b['names'])) if idx is None else np.asarray(idx)
    ob = O.OracleBatch(len(idx), **b['kw'])
    for e, i in zip(ob.envs, idx):
        e.set_task(b['targets'][i], b['starts'][i], b['fulls'][i] if b['has_full'][i] else None, invariant=bool(b['invariant'][i]))
        e.set_initial_pose(b['poses'][i])
    ob.reset()
    return ob


def task_state(ob):
    """The synthetic task's state of every env: dict of int64 [n] (OracleEnv.task_state)."""
    ts = [e.task_state() for e in ob.envs]
    return {k: np.array([t[k] for t in ts], np.int64) for k in ts[0]}


def run_oracle(O, b, idx=None):
    """Steps the batch on the oracle module O with the in-step auto-reset.  Yields (t, OracleBatch) after every step."""
    idx = np.arange(len(b['names'])) if idx is None else np.asarray(idx)
    ob = make_oracle(O, b, idx)
    for t in range(b['T']):
        ob.step_walking(b['actions'][t][idx], autoreset=True)
        yield t, ob


def user_task_truth(O, b):
    """O.task_eval of every case's user task (target, full grid, invariance) on its start grid -- what reset() leaves
    in GridWorld.max_int: dict(max_int [n], argmax [n, 3], target_size [n])."""
    rows = [O.task_eval(b['targets'][i], b['starts'][i], b['fulls'][i] if b['has_full'][i] else None, bool(b['invariant'][i]))
            for i in range(len(b['names']))]
    return dict(max_int=np.array([r['max_int'] for r in rows], np.int32), argmax=np.stack([r['argmax'] for r in rows]).astype(np.int32),
                target_size=np.array([r['target_size'] for r in rows], np.int32))


STATE_KEYS = ('syn_max_int', 'syn_prev_size', 'step_no', 'size', 'dirty')


def record(O, b):
    """Every step's outputs, float64 internals and task state of the batch on oracle module O: arrays over [T, n, ...].
    `dirty` restates the kernels' stale-cache bit: set by a step that changed the synthetic grid without changing its
    block count (the task keeps its cached max_int), cleared by a recount and by a reset."""
    keys = ('agentPos', 'inventory', 'compass', 'reward', 'done', 'grid')
    out = {k: [] for k in keys + ('internal',) + STATE_KEYS}
    n = len(b['names'])
    dirty, grid, size = np.zeros(n, np.int64), b['starts'].reshape(n, -1).copy(), np.zeros(n, np.int64)
    for t, ob in run_oracle(O, b):
        for k in keys:
            out[k].append(getattr(ob, k).copy())
        out['internal'].append(ob.internals())
        ts = task_state(ob)
        done = ob.done.astype(bool)
        # (after an auto-reset the oracle shows the new episode's grid: a finished env is clean whatever it did)
        changed = (ob.grid != grid).any(1) & ~done
        recount = ts['syn_prev_size'] != size
        dirty = np.where(done | recount, 0, np.where(changed, 1, dirty))
        grid, size = ob.grid.copy(), ts['syn_prev_size']
        for k in STATE_KEYS[:-1]:
            out[k].append(ts[k])
        out['dirty'].append(dirty)
    return {k: np.stack(v) for k, v in out.items()}


FIXTURE = 'golden/s15_reward_cases.npz'


def against_fixture(O, group, fixture):
    """The oracle (module O) through the batch of `group` the way the reference was recorded (one env per case, an
    episode that ended is reset before the next step): every field of tests/golden/s15_reward_cases.npz bit for bit.
    Returns the number of env-steps compared."""
    b = batch(group)
    fx = {k[len(group) + 1:]: fixture[k] for k in fixture.files if k.startswith(group + '_')}
    grids = unpack_grids(b, fx)
    for i, name in enumerate(b['names']):
        env = O.OracleEnv(**b['kw'])
        env.set_task(b['targets'][i], b['starts'][i], b['fulls'][i] if b['has_full'][i] else None, invariant=bool(b['invariant'][i]))
        env.set_initial_pose(b['poses'][i])
        env.reset()
        assert env.task_state()['env_max_int'] == fx['env_max_int'][i], name + ' GridWorld.max_int'
        done = False
        for t in range(b['T']):
            where = f'{group} {name} step {t}'
            assert bool(fx['reset_before'][i, t]) == done, where + ' episode boundary'
            if done:
                env.reset()
            obs, reward, done, _ = env.step(int(b['actions'][t, i]))
            assert np.float64(reward).tobytes() == fx['reward'][i, t].tobytes() and done == bool(fx['done'][i, t]), \
                where + f" reward / done {reward} {done} vs {fx['reward'][i, t]} {fx['done'][i, t]}"
            assert env.task_state()['syn_max_int'] == fx['syn_max_int'][i, t], where + ' cached max_int'
            assert np.array_equal(obs['grid'].reshape(-1), grids[i, t]), where + ' grid'
            assert np.array_equal(obs['inventory'], fx['inventory'][i, t]), where + ' inventory'
            assert obs['agentPos'].tobytes() == fx['agentPos'][i, t].tobytes(), where + ' agentPos'
            assert obs['compass'][0].tobytes() == fx['compass'][i, t].tobytes(), where + ' compass'
            assert env.internal().tobytes() == fx['internal'][i, t].tobytes(), where + ' internals'
    return len(b['names']) * b['T']


def pack_grids(b, grids):
    """grids int8 [n, T, 1089] of the batch -> the change list the fixture stores: int16 [k, 4] rows (case, step, cell,
    value) of every cell that differs from the step before (from the start grid at step 0)."""
    n, T = grids.shape[:2]
    prev = np.concatenate([b['starts'].reshape(n, 1, -1), grids[:, :-1]], axis=1)
    i, t, c = np.nonzero(grids != prev)
    return np.stack([i, t, c, grids[i, t, c]], axis=1).astype(np.int16)


def unpack_grids(b, fx):
    n, T = len(b['names']), b['T']
    out = np.zeros((n, T, 1089), np.int8)
    cur = b['starts'].reshape(n, -1).copy()
    rows = fx['grid_changes'].astype(np.int64)
    by_step = {}
    for i, t, c, v in rows:
        by_step.setdefault(t, []).append((i, c, v))
    for t in range(T):
        for i, c, v in by_step.get(t, ()):
            cur[i, c] = v
        out[:, t] = cur
    return out
