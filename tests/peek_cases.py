"""The cases the peek tests share (tests/test_peek_cpu.py, tests/test_gpu_peek.py) and their truth, computed from the CPU
oracle alone.

The oracle has no clone.  For a case, a checkpoint t_c and a set of K candidates of H actions, a batch of K * E oracle
envs -- copy k of the case's envs in rows [k * E, (k + 1) * E) -- is stepped through the case's first t_c actions in
every copy; then copy k plays candidate k's H actions with autoreset=False.  Per step: ob.reward, ob.done, the one grid
cell that differs from the step before, ob.agentPos.  Everything after a candidate's first `done` is blanked.  The
binary64 reward behind a float32 one is looked up among the products the step can form (reward64); `ret` is summed from
those in numpy, in the order the header states.

Cases: the six of tests/mask_cases.py, `recolour` of tests/goal_cases.py and `short` (looking_down's actions on other
targets with max_steps = 28, so that the step limit falls inside a candidate), at checkpoints 0, 12 and 25.
Candidate sets: `tree2` (all 324 pairs of the 18 actions, shared by the envs), `random` (K = 70 sequences of 16 per env:
a 64-candidate chunk and a partial one) and `directed` (H = 32, shared; see DIRECTED)."""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import goal_cases as GC
import mask_cases as MC

E = MC.E
CHECKPOINTS = (0, 12, 25)
SETS = ('tree2', 'random', 'directed')
GAMMAS = (1.0, 0.97)
FLOOR = MC.FLOOR
THREADS = min(16, os.cpu_count() or 1)
SHORT_STEPS = 28


def _pad(seq, h=32):
    assert len(seq) <= h
    return list(seq) + [0] * (h - len(seq))


DOWN = [14] * 9   # from the default pose: the agent then looks at the ground in front of it
# H = 32, written for what only a private future gets right (what they do from the default pose of checkpoint 0; from
# the later checkpoints they are further candidates)
DIRECTED = {
    # place in front, jump and walk onto the block, place again from on top of it, walk on and fall off it
    'own_block': DOWN + [17, 5] + [1] * 7 + [17] + [1] * 5 + [17],
    'own_block_late': DOWN + [17, 0, 5] + [1] * 6 + [0, 17, 16] + [1] * 6,
    # place, then break the same cell (the colour comes from the list, the inventory is refunded), twice, two colours
    'place_break': DOWN + [17, 16, 17, 16, 8, 16, 17, 16, 16],
    # walk into the block just placed: the collision with it stops the agent
    'walk_into': DOWN + [17] + [1] * 12,
    # break a starting block, place another colour there (wrong == 0), place on the next cell: `recolour`'s own script,
    # and the last placement is paid from the cache the recolouring left stale
    'recolour': DOWN + [0] * 3 + [16, 7] + [13] * 9 + [17, 16, 17],
    'recolour_now': [16, 7, 15, 15, 17, 13, 13, 17, 14, 17, 9, 16, 16, 8, 12, 12, 12, 12, 17, 16, 10],
    # a jump on the spot (its way down is faster than 5 per second: 4 sub-steps), one with a placement under way
    'jump': [5] + [0] * 15 + [5, 14, 14, 14, 17] + [0] * 11,
    # place two blocks in a row, jump and walk towards them: the candidate ends above its own blocks
    'stair': DOWN + [17, 15, 15, 17, 14, 14, 5] + [1] * 4 + [5] + [1] * 10,
    # one colour until its inventory is empty (a hotbar action places with select_and_place)
    'same_colour': DOWN + [6, 13] * 11 + [6],
    'same_colour_4': [9, 12] * 16,
    # placements at several pitches, a break, a placement again
    'pitch_sweep': DOWN + [17, 15, 15, 15, 17, 15, 17, 14, 14, 14, 14, 14, 17, 16, 17],
    # two blocks of a colour side by side: `appendix_b`'s target, complete before the sequence ends
    'complete_side': DOWN + [17] + [13] * 5 + [17] + [13] * 4 + [17] + [12] * 3 + [17],
    # actions outside 0..17 are no-ops
    'no_ops': [18, -1, 14, 14, 100, 14, 14, -7, 14, 14, 14, 14, 14, 17, 1 << 30, 16, -(1 << 31), 17, 18, 5],
    'nothing': [],
}
DIRECTED_NAMES = tuple(DIRECTED)


def _short():
    base = MC.cases()['looking_down']
    return dict(base, kw=dict(base['kw'], max_steps=SHORT_STEPS), targets=MC._rt20(9))


@functools.lru_cache(None)
def cases():
    return dict(GC.cases(), short=_short())


def random_candidates(seed, n=E, k=70, h=16):
    """int32 [n, k, h]: per env, candidate and step 30 % place / hotbar, 20 % break, 8 % jump, 12 % look down, the rest
    moves and camera actions."""
    rng = np.random.RandomState(seed)
    u = rng.uniform(size=(n, k, h))
    placing = rng.choice([6, 7, 8, 9, 10, 11, 17, 17, 17, 17], size=(n, k, h))
    other = rng.choice([0, 1, 2, 3, 4, 12, 13, 15], size=(n, k, h))
    a = np.where(u < 0.30, placing, np.where(u < 0.50, 16, np.where(u < 0.58, 5, np.where(u < 0.70, 14, other))))
    return a.astype(np.int32)


@functools.lru_cache(None)
def candidates(name):
    """The named set: int32 [K, H] (shared by the envs) or [E, K, H]."""
    if name == 'tree2':
        a = np.array([[i, j] for i in range(18) for j in range(18)], np.int32)
    elif name == 'random':
        a = random_candidates(31)
    elif name == 'ghost':   # `directed` with its first place (action 17) replaced by a no-op: see own_block_hits
        a = candidates('directed').copy()
        for row in a:
            hit = np.flatnonzero(row == 17)
            if len(hit):
                row[hit[0]] = 0
    else:
        a = np.array([_pad(DIRECTED[k]) for k in DIRECTED_NAMES], np.int32)
    a.setflags(write=False)
    return a


def oracle_batch(case, blocks):
    """An OracleBatch of `blocks` copies of the case's envs, reset (mask_cases.oracle_batch with Task.__init__ and the
    reset of every env in a thread pool: the oracle's envs share nothing and its calls release the interpreter lock)."""
    from oracle import oracle as O
    n = len(case['targets'])
    rows, starts, poses = blocks * n, case['starts'], case['poses']
    ob, lib = O.OracleBatch(rows, **case['kw']), O.lib()

    def prepare(lo):
        for r in range(lo, min(lo + 64, rows)):
            i, e = r % n, ob.envs[r]
            e.set_task(case['targets'][i], None if starts is None else starts[i])
            if poses is not None:
                e.set_initial_pose(poses[i])
            lib.igo_reset(e.h)
            if starts is not None:
                ob.grid[r] = starts[i].reshape(-1)
    with ThreadPoolExecutor(THREADS) as pool:
        list(pool.map(prepare, range(0, rows, 64)))
    return ob


def reward64(r32, right_scale=GC.RIGHT, wrong_scale=GC.WRONG):
    """The binary64 reward the step computed for each float32 reward it returned: wrong * wrong_scale for wrong in
    -1, 0, 1 (a step changes one cell) or right * right_scale for a non-zero right (|right| <= 121 * 9)."""
    table = {}
    for v in [float(w) * wrong_scale for w in (-1, 0, 1)] + [float(r) * right_scale for r in range(-1089, 1090) if r]:
        key = np.float32(v).tobytes()
        assert table.setdefault(key, v) == v, 'two rewards share a float32'
    flat = np.ascontiguousarray(r32, np.float32).reshape(-1)
    return np.array([table[x.tobytes()] for x in flat], np.float64).reshape(np.shape(r32))


def returns(r64, gamma):
    """float32 [...]: R_0 = +0.0, R_{h+1} = R_h + g_h * r_h, g_0 = 1, g_{h+1} = g_h * gamma in binary64 (blanked steps
    hold +0.0, which leaves the sum as it is)."""
    acc, g = np.zeros(r64.shape[:-1], np.float64), 1.0
    for h in range(r64.shape[-1]):
        acc = acc + g * r64[..., h]
        g = g * gamma
    return acc.astype(np.float32)


def truth_of(case, tc, cand, autoreset=False):
    """The five outputs of a peek of `cand` (int32 [K, H] or [E, K, H]) on the case's envs after its first `tc` actions:
    reward float32 [E, K, H], ends int16 [E, K], change int16 [E, K, H], pose float32 [E, K, 5], ret {gamma: float32
    [E, K]}; and for the coverage floors `drop` float32 [E, K, H], how far the agent's y fell in each executed step.
    `autoreset`: of the prefix (the candidates' own steps never reset)."""
    n = len(case['targets'])
    K, H = cand.shape[-2:]
    ob = oracle_batch(case, K)
    for t in range(tc):
        ob.step_walking(np.tile(case['actions'][t], K), autoreset=autoreset, nthreads=THREADS)
    rows = K * n
    reward, change = np.zeros((rows, H), np.float32), np.full((rows, H), -1, np.int16)
    ends, pose, drop = np.zeros(rows, np.int16), np.zeros((rows, 5), np.float32), np.zeros((rows, H), np.float32)
    live, before, ar = np.ones(rows, bool), ob.grid.copy(), np.arange(rows)
    if tc == 0:   # (a reset's observation shows zeros, not the pose)
        y = np.tile(np.array([e.internal()[1] for e in ob.envs[:n]], np.float32), K)
    else:
        y = ob.agentPos[:, 1].copy()
    for h in range(H):
        a = cand[:, :, h].T.reshape(-1) if cand.ndim == 3 else np.repeat(cand[:, h], n)
        ob.step_walking(a, autoreset=False, nthreads=THREADS)
        diff = ob.grid != before
        assert (diff.sum(1) <= 1).all()
        cell = diff.argmax(1)
        code = np.where(diff.any(1), (ob.grid[ar, cell].astype(np.int32) << 11) | cell, -1)
        reward[live, h], change[live, h] = ob.reward[live], code[live]
        pose[live] = ob.agentPos[live]
        drop[live, h] = (y - ob.agentPos[:, 1])[live]
        y = ob.agentPos[:, 1].copy()
        ended = live & (ob.done != 0)
        ends[ended] = h + 1
        live &= ~ended
        before = ob.grid.copy()
    by_env = lambda x: np.ascontiguousarray(np.swapaxes(x.reshape((K, n) + x.shape[1:]), 0, 1))  # noqa: E731
    res = dict(reward=by_env(reward), ends=by_env(ends), change=by_env(change), pose=by_env(pose), drop=by_env(drop))
    r64 = reward64(res['reward'], case['kw'].get('right_placement_scale', GC.RIGHT),
                   case['kw'].get('wrong_placement_scale', GC.WRONG))
    res['ret'] = {g: returns(r64, g) for g in GAMMAS}
    return res


@functools.lru_cache(None)
def truth(name, tc, cset):
    """truth_of the named case at checkpoint tc for the named candidate set (read-only, computed once)."""
    res = truth_of(cases()[name], tc, candidates(cset))
    for v in list(res.values()) + list(res['ret'].values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res


def max_steps_of(case):
    return case['kw'].get('max_steps', 250)


def coverage(name, tc, cset):
    """Per situation the number of candidates (env, k) of truth(name, tc, cset) in it."""
    t, case = truth(name, tc, cset), cases()[name]
    change, reward, ends = t['change'].astype(np.int32), t['reward'], t['ends'].astype(np.int32)
    H = change.shape[-1]
    cell = np.where(change >= 0, change & 0x7ff, -1)
    placed, broke = change >= 2048, (change >= 0) & (change < 2048)
    again = np.zeros(change.shape[:2], bool)
    unpaid_then_paid = np.zeros(change.shape[:2], bool)
    for h in range(1, H):
        earlier = (cell[..., :h] == cell[..., h:h + 1]) & (cell[..., h:h + 1] >= 0)
        again |= earlier.any(-1)
        unpaid = ((change[..., :h] >= 0) & (reward[..., :h] == 0)).any(-1)
        unpaid_then_paid |= unpaid & placed[..., h] & (reward[..., h] != 0)
    limit = (ends > 0) & (tc + ends == max_steps_of(case))
    # a step in which y fell by more than 0.3 ended faster than 5 per second (the speed only grows while falling: its
    # last value is at least its mean 0.3 / 0.05 = 6), so the step after it, if the candidate played one, took 4 or more
    fast = (t['drop'][..., :-1] > 0.3) & ((ends[..., None] == 0) | (np.arange(1, H) < ends[..., None]))
    return {'candidates': int(change.shape[0] * change.shape[1]),
            'a place': int(placed.any(-1).sum()), 'a break': int(broke.any(-1).sum()),
            'two or more changes': int(((change >= 0).sum(-1) >= 2).sum()),
            'a cell changed again': int(again.sum()),
            'an unpaid change, then a paid placement': int(unpaid_then_paid.sum()),
            'an end by completion': int(((ends > 0) & ~limit).sum()), 'an end by max_steps': int(limit.sum()),
            'more than 2 sub-steps': int(fast.any(-1).sum()),
            'right > 0': int((reward >= 0.5).any(-1).sum()), 'right < 0': int((reward <= -0.5).any(-1).sum()),
            'wrong > 0': int(((reward > 0) & (reward < 0.5)).any(-1).sum()),
            'wrong < 0': int(((reward < 0) & (reward > -0.5)).any(-1).sum())}


def own_block_hits(name, tc):
    """Candidates (env, k) of the directed set whose future depends on a block they placed themselves: some step after
    the first place action changes another cell or none, or the final pose differs, when that place is replaced by a
    no-op (the `ghost` set) -- the agent collided with, stood on or aimed at its own block."""
    a, g = truth(name, tc, 'directed'), truth(name, tc, 'ghost')
    cand = candidates('directed')
    n = 0
    for k in range(cand.shape[0]):
        hit = np.flatnonzero(cand[k] == 17)
        if not len(hit):
            continue
        h0 = hit[0]
        placed = a['change'][:, k, h0] >= 0
        later = (a['change'][:, k, h0 + 1:] != g['change'][:, k, h0 + 1:]).any(-1)
        moved = (a['pose'][:, k].view(np.uint32) != g['pose'][:, k].view(np.uint32)).any(-1)
        n += int((placed & (later | moved)).sum())
    return n
