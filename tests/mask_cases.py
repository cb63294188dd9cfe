"""The cases the action-mask tests share (tests/test_query_cpu.py, tests/test_gpu_action_mask.py) and their truth,
computed from the CPU oracle alone.

The oracle has no clone.  For a checkpoint t_c a batch of 9 * E oracle envs -- the base and eight probes, block j in rows
[j * E, (j + 1) * E) -- is stepped through the case's first t_c actions; then probe j takes PROBES[j] (the base a no-op):
  place / break / hotbar-with-select_and_place bits   the probe's grid row changed; the changed cell is `look`
  jump bit                                             internals() dy == 0
  pitch bits                                           pitch > -90 / pitch < 90
  hotbar bits without select_and_place                 active_block != k
  bits 0..4, 12, 13                                    1
Episodes never end inside a case's window except by completing the target (max_steps = 250, no auto-reset: stepping on
after `done` is what the reference does too)."""
import functools
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
E, T = 32, 48
CHECKPOINTS = (0, 1, 5, 12, 25, 40)
PROBES = (6, 7, 8, 9, 10, 11, 16, 17)
KW = dict(size_reward=False, max_steps=250)
FLOOR = 20   # the coverage floor: every conditional bit is 0 in >= FLOOR (env, checkpoint) pairs and 1 in >= FLOOR
CONDITIONAL = (5, 6, 7, 8, 9, 10, 11, 14, 15, 16, 17)


def stream(seed, down=9, place=0.40, brk=0.15, n=E):
    """int32 [T, n]: `down` times action 14 (the agent then looks at the ground in front of it), after that per env and
    step 40 % place / hotbar (17 and 6..11), 15 % break, the rest moves, jumps and camera actions."""
    rng = np.random.RandomState(seed)
    u = rng.uniform(size=(T, n))
    placing = rng.choice([6, 7, 8, 9, 10, 11, 17, 17, 17], size=(T, n))
    other = rng.choice([0, 1, 2, 3, 4, 5, 12, 13, 14, 15], size=(T, n))
    a = np.where(u < place, placing, np.where(u < place + brk, 16, other))
    a[:down] = 14
    return a.astype(np.int32)


def _rt20(seed):
    from gridworld_amd import workloads
    return workloads.rt20(E, seed=seed).numpy().astype(np.int8)


def _towers():
    """CDM targets with two thirds of each target's blocks already standing: blocks to break, walls to hit."""
    goals = np.load(os.path.join(HERE, 'golden', 'cdm_goals.npz'))['dense'].astype(np.int8)
    rng = np.random.RandomState(11)
    targets = goals[rng.choice(len(goals), E, replace=False)]
    starts = np.zeros_like(targets)
    for i in range(E):
        cells = np.flatnonzero(targets[i])
        keep = rng.permutation(cells)[:(2 * len(cells)) // 3]
        starts[i].reshape(-1)[keep] = targets[i].reshape(-1)[keep]
    return targets, starts


def _one_colour_start():
    """A starting grid of 20 blocks of colour 1 + i % 6 (a 4 x 5 patch on the lowest level, beside the agent): that
    colour's inventory is 0 at reset."""
    starts = np.zeros((E, 9, 11, 11), np.int8)
    for i in range(E):
        starts[i, 0, 7:11, 6:11] = 1 + i % 6
    return starts


def _script():
    """SURVEY Appendix B's sequence -- look down, land, place, a second place rejected by the agent's overlap, break,
    a break on the ground, the hotbar placing -- env i starting it i % 16 steps late, so that every checkpoint sees
    the envs at sixteen different points of it."""
    seq = [14] * 9 + [0] * 3 + [17, 17, 16, 16, 17, 0, 17, 16, 8, 17, 16, 16, 0, 5, 17, 0, 16, 10]
    a = np.zeros((T, E), np.int32)
    for i in range(E):
        s = i % 16
        n = min(len(seq), T - s)
        a[s:s + n, i] = seq[:n]
    target = np.zeros((E, 9, 11, 11), np.int8)
    target[:, 0, 5, 3] = target[:, 0, 5, 4] = 1
    return target, a


def _poses():
    """Poses on the step's own lattice (yaw, pitch multiples of 5: what Discrete(18) reaches from the default pose, and
    where the oracle's libm and the device's table agree bit for bit), eight envs each at pitch -90 and +90; some start
    in the air."""
    rng = np.random.RandomState(17)
    pitch = 5.0 * rng.randint(-14, 5, E)
    pitch[:8], pitch[8:16] = -90.0, 90.0
    return np.stack([rng.uniform(-4, 4, E), rng.choice([0.0, 0.0, 2.0], E), rng.uniform(-4, 4, E),
                     5.0 * rng.randint(-36, 37, E), pitch], 1)


@functools.lru_cache(None)
def cases():
    """name -> dict(kw (env keyword arguments), targets, starts, poses (None: default), actions int32 [T, E])."""
    tw_t, tw_s = _towers()
    sc_t, sc_a = _script()
    pose_a = stream(6, down=0)
    pose_a[:, :16] = np.where(np.isin(pose_a[:, :16], (14, 15)), 12, pose_a[:, :16])   # these keep their pitch of +-90
    mk = lambda targets, actions, starts=None, poses=None, **kw: dict(  # noqa: E731
        kw=dict(KW, **kw), targets=targets, starts=starts, poses=poses, actions=actions)
    return {'looking_down': mk(_rt20(1), stream(1)),
            'towers': mk(tw_t, stream(2, down=4), starts=tw_s),
            'empty_inventory': mk(_rt20(3), stream(3), starts=_one_colour_start()),
            'appendix_b': mk(sc_t, sc_a),
            'select_only': mk(_rt20(4), stream(4), select_and_place=False),
            'init_pose': mk(_rt20(5), pose_a, poses=_poses())}


def oracle_batch(case, blocks=1):
    """An OracleBatch of `blocks` copies of the case's envs, reset."""
    from oracle import oracle as O
    ob = O.OracleBatch(blocks * len(case['targets']), **case['kw'])
    tile = lambda a: None if a is None else np.concatenate([a] * blocks)  # noqa: E731
    ob.set_tasks(tile(case['targets']), tile(case['starts']))
    if case['poses'] is not None:
        ob.set_initial_pose(tile(case['poses']))
    ob.reset()
    return ob


def truth_of(case, checkpoints=CHECKPOINTS):
    """(mask uint8 [C, E, 18], look int16 [C, E, 2]) of a case (of any number of envs E) at the checkpoints, from the
    oracle alone."""
    E = len(case['targets'])
    masks = np.zeros((len(checkpoints), E, 18), np.uint8)
    looks = np.full((len(checkpoints), E, 2), -1, np.int16)
    for c, tc in enumerate(checkpoints):
        ob = oracle_batch(case, 9)
        for t in range(tc):
            ob.step_walking(np.tile(case['actions'][t], 9), nthreads=8)
        state = ob.internals()[:E]   # x, y, z, yaw, pitch, dy, time_int_steps, active_block
        before = ob.grid.copy()
        assert all(np.array_equal(before[:E], before[j * E:(j + 1) * E]) for j in range(9))
        ob.step_walking(np.concatenate([np.zeros(E, np.int32)] + [np.full(E, p, np.int32) for p in PROBES]))
        assert np.array_equal(ob.grid[:E], before[:E])
        m = masks[c]
        m[:, [0, 1, 2, 3, 4, 12, 13]] = 1
        m[:, 5] = state[:, 5] == 0.0
        m[:, 14], m[:, 15] = state[:, 4] > -90.0, state[:, 4] < 90.0
        for j, p in enumerate(PROBES):
            diff = ob.grid[(j + 1) * E:(j + 2) * E] != before[:E]
            assert (diff.sum(1) <= 1).all()
            m[:, p] = diff.any(1)
            if p >= 16:
                looks[c, :, p - 16] = np.where(diff.any(1), diff.argmax(1), -1)
        if not case['kw'].get('select_and_place', True):
            for k in range(1, 7):
                assert not m[:, 5 + k].any()   # a hotbar action alone never changes the grid
                m[:, 5 + k] = state[:, 7] != k
    return masks, looks


@functools.lru_cache(None)
def truth(name):
    """truth_of the named case at CHECKPOINTS (read-only, computed once)."""
    masks, looks = truth_of(cases()[name])
    masks.setflags(write=False)
    looks.setflags(write=False)
    return masks, looks
