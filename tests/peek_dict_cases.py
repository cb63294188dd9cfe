"""The cases the peek_dict tests share (tests/test_peek_dict_cpu.py, tests/test_gpu_peek_dict.py) and their truth, computed
from the CPU oracle alone, the way tests/peek_cases.py does it for the Discrete(18) space.

Spaces: 'flying' and 'walking_dict'.  Cases: the eight of peek_cases (the six of mask_cases, `recolour`, `short` with
max_steps = 28), their envs, targets, starting grids and poses re-created in the space, their Discrete(18) action
streams translated into it (from_discrete) as the prefix that leads to checkpoints 0, 12 and 25.

For a space, a case, a checkpoint t_c and a set of K candidates of H actions, a batch of K * E oracle envs -- copy k of
the case's envs in rows [k * E, (k + 1) * E) -- is stepped through the first t_c actions in every copy; then copy k plays
candidate k with autoreset=False.  Per step: ob.reward, ob.done, the one grid cell that differs from the step before,
ob.agentPos.  Everything after a candidate's first `done` is blanked; `ret` is summed in numpy in the header's order.
The oracle runs in device-trig mode (oracle.use_device_trig(True)) -- the general sin / cos / atan2 are then the
kernels' own, so every output word is exact -- and the mode is restored afterwards.

The oracle has the reference's semantics for an invalid action component (it raises there, or carries a NaN into the
pose); the step and peek_dict run such a component as a no-op (include/igw_peek_dict.h).  sanitise() applies that one
rule to the actions the oracle is handed; nothing else of the truth knows about it.

Candidate sets per space: `random` (K = 70 per env: a 64-candidate chunk and a partial one, H = 16; camera deltas within
+-5 degrees for the even candidates, +-90 for the odd ones), `shared` (K = 3, H = 1) and `directed` (H = 32, shared; see
FLY_DIRECTED / DICT_DIRECTED)."""
import functools

import numpy as np

import peek_cases as PC

E = PC.E
CHECKPOINTS = PC.CHECKPOINTS
SPACES = ('flying', 'walking_dict')
SETS = ('random', 'shared', 'directed')
GAMMAS = PC.GAMMAS
THREADS = PC.THREADS
SHORT_STEPS = PC.SHORT_STEPS
CAMERA_MAX = 1e6
KW = {'flying': dict(action_space='flying'), 'walking_dict': dict(action_space='walking', discretize=False)}
# key -> (dtype, shape behind [.., K, H]) in the order of the step's arguments
FIELDS = {'flying': (('movement', np.float32, (3,)), ('camera', np.float32, (2,)), ('inventory', np.int32, ()),
                     ('placement', np.int32, ())),
          'walking_dict': (('buttons', np.uint8, (8,)), ('camera', np.float32, (2,)))}
NAN, INF = float('nan'), float('inf')


# ---- actions -------------------------------------------------------------------------------------------------------------
def fly(mv=(0, 0, 0), cam=(0, 0), inv=0, pl=0):
    """One flying action: movement (strafe[0]: -1 forward, strafe[1]: -1 left, dy: 1 up), camera (yaw, pitch),
    inventory, placement."""
    return dict(movement=mv, camera=cam, inventory=inv, placement=pl)


def btn(fwd=0, back=0, left=0, right=0, jump=0, attack=0, use=0, hotbar=0, cam=(0, 0)):
    """One walking Dict action."""
    return dict(buttons=(fwd, back, left, right, jump, attack, use, hotbar), camera=cam)


def pack(space, seqs, h=None):
    """Sequences (lists of fly() / btn() actions) as the space's dict of arrays [K, H, ...], padded with no-ops."""
    h = h or max(len(s) for s in seqs)
    noop = fly() if space == 'flying' else btn()
    out = {}
    for key, dt, _ in FIELDS[space]:
        out[key] = np.array([[a[key] for a in list(s) + [noop] * (h - len(s))] for s in seqs], dt)
    return out


def from_discrete(space, a):
    """A Discrete(18) action array (any shape) as the space's dict of arrays of that leading shape: 1..4 moves, 5 jump /
    fly up, 6..11 hotbar, 12 / 13 yaw -+5, 14 / 15 pitch -+5, 16 break, 17 place; anything else a no-op."""
    a = np.asarray(a)
    cam = np.zeros(a.shape + (2,), np.float32)
    cam[..., 0] = np.where(a == 12, -5, np.where(a == 13, 5, 0))
    cam[..., 1] = np.where(a == 14, -5, np.where(a == 15, 5, 0))
    hot = np.where((a >= 6) & (a <= 11), a - 5, 0)
    if space == 'flying':
        mv = np.zeros(a.shape + (3,), np.float32)
        mv[..., 0] = np.where(a == 1, -1, np.where(a == 2, 1, 0))
        mv[..., 1] = np.where(a == 3, -1, np.where(a == 4, 1, 0))
        mv[..., 2] = a == 5
        return dict(movement=mv, camera=cam, inventory=hot.astype(np.int32),
                    placement=np.where(a == 17, 1, np.where(a == 16, 2, 0)).astype(np.int32))
    b = np.stack([a == 1, a == 2, a == 3, a == 4, a == 5, a == 16, a == 17, hot], -1).astype(np.uint8)
    return dict(buttons=b, camera=cam)


def invalid_kinds(space, act):
    """kind -> bool array over the actions' leading shape: where the action has an invalid component of that kind."""
    cam = act['camera'].astype(np.float64)
    kinds = {'a camera that is not finite': ~np.isfinite(cam).all(-1),
             'a camera beyond the limit': (np.isfinite(cam) & (np.abs(cam) > CAMERA_MAX)).any(-1)}
    if space == 'flying':
        kinds['a movement that is not finite'] = ~np.isfinite(act['movement']).all(-1)
        kinds['an inventory outside 0..6'] = (act['inventory'] < 0) | (act['inventory'] > 6)
        kinds['a placement outside 0..2'] = (act['placement'] < 0) | (act['placement'] > 2)
    else:
        kinds['a hotbar byte above 6'] = act['buttons'][..., 7] > 6
    return kinds


def sanitise(space, act):
    """The actions with every invalid component replaced by its no-op (include/igw_peek_dict.h, "Invalid actions")."""
    out = {k: np.array(v) for k, v in act.items()}
    cam = out['camera']
    cam[~(np.abs(cam.astype(np.float64)) <= CAMERA_MAX)] = 0     # (NaN compares false)
    if space == 'flying':
        out['movement'][~np.isfinite(out['movement'])] = 0
        out['inventory'][(out['inventory'] < 0) | (out['inventory'] > 6)] = 0
        out['placement'][(out['placement'] < 0) | (out['placement'] > 2)] = 0
    else:
        hot = out['buttons'][..., 7]
        hot[hot > 6] = 0
    return out


# ---- candidate sets ------------------------------------------------------------------------------------------------------
_D = PC.DIRECTED
FLY_DOWN = [fly(cam=(0, -45))]   # from the default pose: the agent then looks at the ground in front of it
FLY_DIRECTED = {
    # fly up and place from above
    'from_above': [fly(mv=(0, 0, 1))] * 3 + [fly(cam=(0, -90))] + [fly(pl=1), fly(mv=(0, 0, -1), pl=1), fly(pl=1)],
    # place, then break the same cell (the colour comes from the list, the inventory is refunded), two colours
    'place_break': FLY_DOWN + [fly(pl=1), fly(pl=2), fly(pl=1), fly(pl=2), fly(inv=3, pl=2), fly(pl=1), fly(pl=2), fly(pl=2)],
    # walk into the block just placed: the collision with it stops the agent
    'walk_into': FLY_DOWN + [fly(pl=1), fly(cam=(0, 45))] + [fly(mv=(-1, 0, 0))] * 8,
    'walk_into_side': FLY_DOWN + [fly(pl=1, cam=(90, 0)), fly(pl=1, cam=(-90, 45))] + [fly(mv=(-0.5, 0.25, 0))] * 10,
    # fly past |x| = 7 and |z| = 7: the padded-zone gate stops the agent
    'leave_x': [fly(cam=(90, 0))] + [fly(mv=(-1, 0, 0))] * 31,
    'leave_z': [fly(mv=(1, 0.5, 0))] * 20 + [fly(mv=(0, 0, 1))] * 12,
    'leave_up': [fly(mv=(0, 0, 1))] * 32,
    # pitch driven past +-90
    'pitch_clamp': [fly(cam=(0, 60))] * 3 + [fly(pl=1)] + [fly(cam=(0, -70))] * 4 + [fly(pl=1), fly(cam=(0, 35.5), pl=1)],
    # yaw driven past 360 and below 0 by one large camera value, and by small ones
    'yaw_wrap': [fly(cam=(1000.5, -40)), fly(pl=1), fly(cam=(-2500.25, 0)), fly(pl=1), fly(cam=(359.75, 0)), fly(pl=1),
                 fly(cam=(-0.125, 0))] * 2 + [fly(cam=(999999.0, 0), pl=1), fly(cam=(-1e6, 0), pl=1)],
    # inventory = 0 with placement = 1, a hotbar change alone, one with a break (select_and_place cancels it)
    'select': FLY_DOWN + [fly(inv=0, pl=1), fly(inv=3, cam=(45, 0)), fly(inv=4, pl=2, cam=(45, 0)), fly(inv=0, pl=2),
                          fly(inv=5, pl=1, cam=(45, 0)), fly(inv=0, pl=2), fly(inv=2, pl=2)],
    # one colour, place after place: where the case starts with few or none of it (`empty_inventory`: none of colour
    # 1 + i % 6) the stock is empty inside the candidate
    'same_colour': FLY_DOWN + [fly(inv=1, pl=1, cam=(11, 0))] * 31,
    'same_colour_4': [fly(cam=(0, -60))] + [fly(inv=4, pl=1, cam=(-17, 0.5))] * 31,
    # two blocks of a colour side by side: `appendix_b`'s target, complete before the sequence ends
    'complete_side': None,
    # every kind of invalid action, each with valid components beside it that still act
    'invalid': FLY_DOWN + [fly(mv=(NAN, 0, 0), pl=1), fly(mv=(-1, INF, 0)), fly(mv=(0, 0, -INF), cam=(10, 0)),
                           fly(cam=(NAN, -5), pl=2), fly(cam=(15, INF), pl=1), fly(cam=(2e6, 0), pl=1),
                           fly(cam=(10, -1.5e6), pl=1), fly(inv=7, pl=0, cam=(10, 0)), fly(inv=-1, pl=1, cam=(10, 0)),
                           fly(inv=1 << 20, pl=2), fly(inv=2, pl=3, cam=(10, 0)), fly(inv=0, pl=-1), fly(pl=1 << 16),
                           fly(mv=(NAN, NAN, NAN), cam=(NAN, NAN), inv=9, pl=7), fly(pl=1)],
    'nothing': [],
}
DICT_DOWN = [btn(cam=(0, -45))]
DICT_DIRECTED = {
    # two movement buttons at once: the general strafe heading; opposite buttons cancel
    'two_buttons': [btn(fwd=1, left=1)] * 4 + [btn(back=1, right=1)] * 3 + [btn(fwd=1, back=1)] * 2 + [btn(fwd=1, right=1, jump=1)] * 4 +
                   [btn(left=1, right=1, back=1)] * 3,
    # jump with forward onto an own block
    'jump_onto': DICT_DOWN + [btn(use=1), btn(jump=1, fwd=1)] + [btn(fwd=1)] * 6 + [btn(use=1)] + [btn(fwd=1)] * 5 + [btn(use=1)],
    'walk_into': DICT_DOWN + [btn(use=1)] + [btn(fwd=1)] * 12,
    # attack and use together: a no-op; with a hotbar byte under select_and_place a placement
    'attack_use': DICT_DOWN + [btn(attack=1, use=1), btn(use=1), btn(attack=1, use=1), btn(attack=1),
                               btn(attack=1, use=1, hotbar=2), btn(attack=1), btn(attack=1, hotbar=3), btn(attack=1)],
    # a hotbar byte with `use`
    'hotbar_use': DICT_DOWN + [btn(use=1, hotbar=5), btn(cam=(25, 0)), btn(use=1, hotbar=6), btn(hotbar=1, cam=(25, 0)), btn(use=1)],
    # a fractional camera: off the 5-degree lattice, the general sin / cos
    'fractional': [btn(cam=(0.3, -44.7)), btn(use=1), btn(cam=(17.45, 3.125), use=1), btn(fwd=1, cam=(-0.1, 0)), btn(fwd=1, left=1),
                   btn(use=1, cam=(33.3, -1.1)), btn(attack=1), btn(cam=(-400.6, 0), use=1), btn(cam=(1234.56, -100)), btn(use=1)],
    'same_colour': DICT_DOWN + [btn(hotbar=1, use=1, cam=(11, 0))] * 31,
    'invalid': DICT_DOWN + [btn(hotbar=7, use=1), btn(hotbar=255, cam=(10, 0)), btn(hotbar=9, attack=1), btn(cam=(NAN, -5), use=1),
                            btn(cam=(15, INF), use=1), btn(cam=(2e6, 0), fwd=1), btn(cam=(10, -1.5e6), use=1),
                            btn(hotbar=8, cam=(NAN, NAN), jump=1), btn(use=1)],
}


def _directed(space):
    if space == 'flying':
        seqs = dict(FLY_DIRECTED)
        seqs['complete_side'] = None
        packed = pack(space, [s or [] for s in seqs.values()], 32)
        side = from_discrete(space, np.array(PC._pad(_D['complete_side']), np.int32))
        for key in packed:
            packed[key][list(seqs).index('complete_side')] = side[key]
        return tuple(seqs), packed
    # the Dict space first plays peek_cases' own directed sequences, translated: the same physics, the other parser
    names = tuple('discrete_' + k for k in PC.DIRECTED_NAMES) + tuple(DICT_DIRECTED)
    a = from_discrete(space, np.array([PC._pad(_D[k]) for k in PC.DIRECTED_NAMES], np.int32))
    b = pack(space, list(DICT_DIRECTED.values()), 32)
    return names, {key: np.concatenate([a[key], b[key]]) for key in a}


def directed_names(space):
    return _directed(space)[0]


def random_candidates(space, seed, n=E, k=70, h=16):
    """The space's dict of arrays [n, k, h, ...]: per env, candidate and step a place in 30 %, a break in 20 %, a hotbar
    change in 25 %, movement in half the steps, camera deltas within +-5 degrees (even candidates) or +-90 (odd ones)."""
    rng = np.random.RandomState(seed)
    shape = (n, k, h)
    u = rng.uniform(size=shape)
    place, brk = u < 0.30, (u >= 0.30) & (u < 0.50)
    hot = np.where(rng.uniform(size=shape) < 0.25, rng.randint(1, 7, shape), 0)
    span = np.where(np.arange(k) % 2 == 0, 5.0, 90.0)[None, :, None, None]
    cam = (rng.uniform(-1, 1, shape + (2,)) * span).astype(np.float32)
    cam[rng.uniform(size=shape) < 0.3] = 0
    moving = rng.uniform(size=shape) < 0.5
    if space == 'flying':
        mv = rng.uniform(-1, 1, shape + (3,)).astype(np.float32)
        mv[..., 2] = np.where(rng.uniform(size=shape) < 0.3, mv[..., 2], 0)
        mv[rng.uniform(size=shape + (3,)) < 0.3] = 0
        mv[~moving] = 0
        return dict(movement=mv, camera=cam, inventory=hot.astype(np.int32),
                    placement=np.where(place, 1, np.where(brk, 2, 0)).astype(np.int32))
    b = np.zeros(shape + (8,), np.uint8)
    for j, pr in enumerate((0.5, 0.2, 0.25, 0.25)):
        b[..., j] = moving & (rng.uniform(size=shape) < pr)
    b[..., 4] = rng.uniform(size=shape) < 0.1
    b[..., 5], b[..., 6], b[..., 7] = brk, place, hot
    return dict(buttons=b, camera=cam)


@functools.lru_cache(None)
def candidates(space, name):
    """The named set of the space: a dict of read-only arrays [K, H, ...] (shared by the envs) or [E, K, H, ...]."""
    if name == 'random':
        a = random_candidates(space, 31)
    elif name == 'shared':
        if space == 'flying':
            a = pack(space, [[fly(mv=(-1, 0, 0), cam=(12.5, -50), inv=2)], [fly(pl=1)], [fly(pl=2, cam=(0, -30))]])
        else:
            a = pack(space, [[btn(fwd=1, right=1, cam=(12.5, -50), hotbar=2)], [btn(use=1)], [btn(attack=1, cam=(0, -30))]])
    elif name == 'ghost':   # `directed` with its first place by `placement` / `use` alone made a no-op: own_block_hits
        a = {k: v.copy() for k, v in candidates(space, 'directed').items()}
        for row, h0 in enumerate(first_places(space)):
            if h0 >= 0:
                if space == 'flying':
                    a['placement'][row, h0] = 0
                else:
                    a['buttons'][row, h0, 6] = 0
    else:
        a = _directed(space)[1]
    for v in a.values():
        v.setflags(write=False)
    return a


def first_places(space):
    """Per directed sequence the first step that asks for a place with no hotbar change and no break beside it (-1: none)."""
    a = candidates(space, 'directed')
    if space == 'flying':
        ask = (a['placement'] == 1) & (a['inventory'] == 0)
    else:
        ask = (a['buttons'][..., 6] != 0) & (a['buttons'][..., 5] == 0) & (a['buttons'][..., 7] == 0)
    return [int(np.flatnonzero(r)[0]) if r.any() else -1 for r in ask]


# ---- truth ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def cases(space):
    """peek_cases' cases with the space's env keyword arguments."""
    return {name: dict(c, kw=dict(c['kw'], **KW[space])) for name, c in PC.cases().items()}


def _step(ob, space, act):
    act = sanitise(space, act)
    if space == 'flying':
        ob.step_flying(act['movement'], act['camera'], act['inventory'], act['placement'], autoreset=False, nthreads=THREADS)
    else:
        ob.step_walking_dict(act['buttons'], act['camera'], autoreset=False, nthreads=THREADS)


def truth_of(space, case, tc, cand, trig_after=False):
    """The five outputs of a peek_dict of `cand` (the space's dict of arrays [K, H, ...] or [E, K, H, ...]) on the case's
    envs after its first `tc` actions: reward float32 [E, K, H], ends int16 [E, K], change int16 [E, K, H], pose float32
    [E, K, 5], ret {gamma: float32 [E, K]}.  The oracle's trig mode can be set but not read: `trig_after` is the mode to
    leave it in -- libm, the default every other test assumes, unless the caller runs in device-trig mode itself."""
    from oracle import oracle as O
    n = len(case['targets'])
    first = FIELDS[space][0]
    per_env = cand[first[0]].ndim == 3 + len(first[2])
    K, H = cand[first[0]].shape[1:3] if per_env else cand[first[0]].shape[:2]
    rows = K * n
    O.use_device_trig(True)
    try:
        ob = PC.oracle_batch(case, K)
        prefix = from_discrete(space, case['actions'][:tc])
        for t in range(tc):
            _step(ob, space, {k: np.concatenate([v[t]] * K) for k, v in prefix.items()})
        reward, change = np.zeros((rows, H), np.float32), np.full((rows, H), -1, np.int16)
        ends, pose = np.zeros(rows, np.int16), np.zeros((rows, 5), np.float32)
        live, before, ar = np.ones(rows, bool), ob.grid.copy(), np.arange(rows)
        for h in range(H):
            if per_env:   # row k * n + i plays candidate k of env i
                act = {k: np.swapaxes(v[:, :, h], 0, 1).reshape((rows,) + v.shape[3:]) for k, v in cand.items()}
            else:
                act = {k: np.repeat(v[:, h], n, axis=0) for k, v in cand.items()}
            _step(ob, space, act)
            diff = ob.grid != before
            assert (diff.sum(1) <= 1).all()
            cell = diff.argmax(1)
            code = np.where(diff.any(1), (ob.grid[ar, cell].astype(np.int32) << 11) | cell, -1)
            reward[live, h], change[live, h] = ob.reward[live], code[live]
            pose[live] = ob.agentPos[live]
            ended = live & (ob.done != 0)
            ends[ended] = h + 1
            live &= ~ended
            before = ob.grid.copy()
    finally:
        O.use_device_trig(trig_after)
    by_env = lambda x: np.ascontiguousarray(np.swapaxes(x.reshape((K, n) + x.shape[1:]), 0, 1))  # noqa: E731
    res = dict(reward=by_env(reward), ends=by_env(ends), change=by_env(change), pose=by_env(pose))
    r64 = PC.reward64(res['reward'], case['kw'].get('right_placement_scale', PC.GC.RIGHT),
                      case['kw'].get('wrong_placement_scale', PC.GC.WRONG))
    res['ret'] = {g: PC.returns(r64, g) for g in GAMMAS}
    return res


@functools.lru_cache(None)
def truth(space, name, tc, cset):
    """truth_of the named case of the space at checkpoint tc for the named candidate set (read-only, computed once)."""
    res = truth_of(space, cases(space)[name], tc, candidates(space, cset))
    for v in list(res.values()) + list(res['ret'].values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res


def executed(space, name, tc, cset):
    """bool [E, K, H]: the steps the candidates of truth(space, name, tc, cset) executed."""
    ends = truth(space, name, tc, cset)['ends'].astype(np.int32)
    H = truth(space, name, tc, cset)['change'].shape[-1]
    return (ends[..., None] == 0) | (np.arange(H) < ends[..., None])


def census(space, name, tc, cset):
    """Per situation the number of candidates (env, k) of truth(space, name, tc, cset) in it; per kind of invalid action
    the number of executed steps with one."""
    t, case = truth(space, name, tc, cset), cases(space)[name]
    change, ends = t['change'].astype(np.int32), t['ends'].astype(np.int32)
    limit = (ends > 0) & (tc + ends == PC.max_steps_of(case))
    got = {'candidates': int(change.shape[0] * change.shape[1]),
           'a place': int((change >= 2048).any(-1).sum()),
           'a break': int(((change >= 0) & (change < 2048)).any(-1).sum()),
           'an end by completion': int(((ends > 0) & ~limit).sum()), 'an end by max_steps': int(limit.sum())}
    run = executed(space, name, tc, cset)
    for kind, where in invalid_kinds(space, candidates(space, cset)).items():
        got[kind] = int((np.broadcast_to(where, run.shape) & run).sum())
    return got


def own_block_hits(space, name, tc):
    """Candidates (env, k) of the directed set whose future depends on a block they placed themselves: some step after
    their first place changes another cell or none, or the final pose differs, when that place is made a no-op (the
    `ghost` set) -- the agent collided with, stood on or aimed at its own block."""
    a, g = truth(space, name, tc, 'directed'), truth(space, name, tc, 'ghost')
    n = 0
    for k, h0 in enumerate(first_places(space)):
        if h0 < 0:
            continue
        placed = a['change'][:, k, h0] >= 0
        later = (a['change'][:, k, h0 + 1:] != g['change'][:, k, h0 + 1:]).any(-1)
        moved = (a['pose'][:, k].view(np.uint32) != g['pose'][:, k].view(np.uint32)).any(-1)
        n += int((placed & (later | moved)).sum())
    return n


def own_block_collisions(space, name, tc):
    """... and those among them whose POSITION differs: the agent's body met the block (a collision or a landing)."""
    a, g = truth(space, name, tc, 'directed'), truth(space, name, tc, 'ghost')
    n = 0
    for k, h0 in enumerate(first_places(space)):
        if h0 >= 0:
            placed = a['change'][:, k, h0] >= 0
            moved = (a['pose'][:, k, :3].view(np.uint32) != g['pose'][:, k, :3].view(np.uint32)).any(-1)
            n += int((placed & moved).sum())
    return n
