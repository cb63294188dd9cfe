"""The relabel query (igw_relabel, G.relabel, VecGridWorld.relabel, EpisodeLogger.relabel) on the GPU.
Yardsticks, exact (0 mismatches): the stepped CPU oracle under every goal (tests/relabel_cases.py) for the real logs of
the eight shared cases, and the numpy model of tests/relabel_model.py -- which tests/test_relabel_cpu.py pins to that
oracle -- for what the physics never writes and for the return."""
import numpy as np
import pytest
import torch

from gridworld_amd import relabel as _feature  # noqa: F401  (without the query nothing in this file can run)

import mask_cases as MC
import relabel_cases as RC
import relabel_model as RM

pytestmark = pytest.mark.gpu

E, T = RC.E, RC.T
ROW, CAP = 1104, 64          # the logs of this file hold 64 steps per slot: L = 64 > T, so every row ends in padding
GAMMA = 0.9
ALL = ('reward', 'done', 'progress', 'end', 'ret', 'target_size', 'target')


def _logged(case, n=E, capacity=CAP, steps=T, **kw):
    """A batch of the case's first n envs with the trajectory log on, reset and stepped `steps` times."""
    from gridworld_amd import VecGridWorld
    env = VecGridWorld(n, **dict(case['kw'], **kw))
    pose = None if case['poses'] is None else case['poses'][:n]
    env.set_tasks(case['targets'][:n], None if case['starts'] is None else case['starts'][:n], init_pose=pose)
    rec, heads = env.enable_trajectory_log(n, capacity)
    env.reset()
    acts = torch.from_numpy(case['actions'][:, :n]).to(env.device)
    for t in range(steps):
        env.step(acts[t])
    return env, rec, heads


def _episodes(heads, cap):
    """(first int64 [n], length int32 [n]) device tensors of the slot of every env that holds more steps."""
    h = heads.cpu().numpy()
    slot = h[:, :, 1].argmax(1)
    n = len(h)
    first = (np.arange(n) * 2 + slot) * cap
    return (torch.from_numpy(first.astype(np.int64)).to(heads.device),
            torch.from_numpy(h[np.arange(n), slot, 1].astype(np.int32)).to(heads.device))


def _rows(a, dev):
    """int8 numpy [..., 1089] -> device tensor [..., 1104]."""
    out = np.zeros(a.shape[:-1] + (ROW,), np.int8)
    out[..., :1089] = a
    return torch.from_numpy(out).to(dev)


def _raw_target(t):
    e, g = t.shape[:2]
    return torch.as_strided(t, (e, g, ROW), (g * ROW, ROW, 1), t.storage_offset()).cpu().numpy()


def _same(got, want, where=''):
    """Every word of every output named in `want` (numpy) equals `got` (the dict relabel returned)."""
    for k, w in want.items():
        g = _raw_target(got[k]) if k == 'target' else got[k].cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (where, k, g.dtype, g.shape, w.dtype, w.shape)
        bits = (lambda a: a.view(np.uint32)) if w.dtype == np.float32 else (lambda a: a)
        bad = int((bits(g) != bits(w)).sum())
        assert bad == 0, f'{where} {k}: {bad} of {w.size} elements differ'


@pytest.fixture(scope='module')
def logs():
    """name -> (env, records, heads, first, length) of the case's real log, made once."""
    made = {}

    def get(name):
        if name not in made:
            env, rec, heads = _logged(RC.cases()[name])
            made[name] = (env, rec, heads) + _episodes(heads, CAP)
        return made[name]
    return get


def _want(name, goals, gamma=GAMMA):
    """The oracle's truth of the named case for the goal columns `goals`, padded to CAP steps; ret from the model."""
    b, t, grids = RC.base(name), RC.truth(name), RC.goal_grids(name)
    pad = lambda a: np.concatenate([a[:, goals], np.zeros((E, len(goals), CAP - T), a.dtype)], 2)  # noqa: E731
    ms = RC.cases()[name]['kw']['max_steps']
    ret = np.array([[RM.episode(b['starts'][i], b['change'][i], grids[i, g], RC.RIGHT, RC.WRONG, ms, gamma)['ret']
                     for g in goals] for i in range(E)], np.float32)
    target = np.zeros((E, len(goals), ROW), np.int8)
    target[..., :1089] = grids[:, goals]
    size = np.count_nonzero(grids[:, goals] - b['starts'][:, None], axis=2).astype(np.int16)
    return dict(reward=pad(t['reward']), done=pad(t['done']), progress=pad(t['progress']),
                end=RC.end_of(t['done'][:, goals]), ret=ret, target_size=size, target=target)


# ---- 1. real logs against the stepped oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(RC.cases()))
def test_the_real_log_relabelled_equals_the_oracle_stepped_under_every_goal(name, logs):
    import gridworld_amd as G
    env, rec, heads, first, length = logs(name)
    assert (length == T).all()
    b, grids = RC.base(name), RC.goal_grids(name)
    # the log holds the change words the oracle's grids imply
    words = rec.view(E, 2, CAP, 64)[:, :, :, 40:42].contiguous().view(torch.int16).cpu().numpy().view(np.uint16)[..., 0]
    slot = (first.cpu().numpy() // CAP) % 2
    assert np.array_equal(words[np.arange(E), slot, :T], b['change'])
    starts = _rows(b['starts'], env.device)
    given = [RC.GOALS.index(k) for k in ('own', 'rolled')]                   # user targets
    entries = [RC.GOALS.index(k) for k in ('final', 'at24', 'at5', 'at0')]   # entries of the episode itself
    kw = dict(right_scale=RC.RIGHT, wrong_scale=RC.WRONG, max_steps=RC.cases()[name]['kw']['max_steps'], gamma=GAMMA,
              outputs=ALL)
    res = G.relabel(rec, first, length, starts, targets=_rows(grids[:, given], env.device), **kw)
    assert list(res) == list(ALL) and tuple(res['reward'].shape) == (E, 2, CAP)
    assert tuple(res['target'].shape) == (E, 2, 9, 11, 11) and res['target'].stride() == (2 * ROW, ROW, 121, 11, 1)
    _same(res, _want(name, given), name + ' targets')
    at = torch.tensor([[RC.AT[RC.GOALS[g]] for g in entries]] * E, dtype=torch.int32, device=env.device)
    res = G.relabel(rec, first, length, starts, at=at, **kw)
    _same(res, _want(name, entries), name + ' at')
    # all six in one launch, as targets (two blocks per episode, the second half empty)
    res = G.relabel(rec, first, length, starts, targets=_rows(grids, env.device), **kw)
    _same(res, _want(name, list(range(6))), name + ' six')


@pytest.mark.parametrize('name', ['towers', 'recolour', 'unbuild'])
def test_the_own_target_reproduces_the_logs_reward_and_done(name, logs):
    import gridworld_amd as G
    env, rec, heads, first, length = logs(name)
    own = (env.task_target + env.task_start)[:, None, :].contiguous()
    res = G.relabel(rec, first, length, env.task_start, targets=own, outputs=('reward', 'done'), pad=T)
    r = rec.view(E, 2, CAP, 64)
    slot = ((first // CAP) % 2).long()
    mine = r[torch.arange(E, device=rec.device), slot, :T]
    logged_reward = mine[:, :, 20:24].contiguous().view(torch.int32)[..., 0]
    assert torch.equal(res['reward'][:, 0].contiguous().view(torch.int32), logged_reward)
    assert torch.equal(res['done'][:, 0], mine[:, :, 42])
    assert int((logged_reward != 0).sum()) >= 20


# ---- 2. what the physics never writes, against the model --------------------------------------------------------------------
def _hand_written(seed=3, n_rec=1000, L=300):
    rng = np.random.RandomState(seed)
    cells = np.array([y * 121 + x * 11 + z for y in (0, 1) for x in range(3, 8) for z in range(3, 8)])
    word = np.where(rng.uniform(size=n_rec) < 0.3, rng.choice(cells, n_rec) | rng.randint(0, 7, n_rec) << 11, 0xffff)
    odd = rng.uniform(size=n_rec)
    word = np.where(odd < 0.03, rng.randint(1089, 2048, n_rec) | rng.randint(0, 8, n_rec) << 11, word)   # cells >= 1089
    word = np.where((odd >= 0.03) & (odd < 0.06), rng.choice(cells, n_rec) | 7 << 11, word)              # colour 7
    rec = rng.randint(0, 256, (n_rec, 64)).astype(np.uint8)        # every other field of a record is noise
    rec[:, 40:42] = word.astype(np.uint16).view(np.uint8).reshape(-1, 2)
    #                 whole   1   0   L-1  chunk+1 chunk  64  65  63  clamped  <0  aliases ....  out of the buffer ....
    first = np.array([0,     5,  9,  700, 100,   100,  300, 300, 300, 650,  20,  0,   1,  700, 701, 999, 1000, -1, 1 << 40])
    length = np.array([300,  1,  0,  299, 257,   256,  64,  65,  63,  400,  -3,  300, 300, 300, 300, 1,   1,    5,  5], np.int32)
    e = len(first)
    starts = np.zeros((e, ROW), np.int8)
    targets = np.zeros((e, 5, ROW), np.int8)
    for i in range(e):
        starts[i, rng.choice(cells, 6, replace=False)] = rng.randint(1, 7, 6)
        for g in range(5):
            targets[i, g, rng.choice(cells, 12, replace=False)] = rng.randint(1, 8, 12)
    targets[:, 4] = starts                                          # an empty synthetic target
    at = np.stack([rng.randint(0, 301, (e,)), np.full(e, -5), np.full(e, 1 << 20), length, np.zeros(e, np.int64)], 1).astype(np.int32)
    return rec, first, length, starts, targets, at, L


@pytest.mark.parametrize('mode', ['targets', 'at'])
def test_hand_written_records_equal_the_model(mode):
    """Lengths 0, 1, L and beyond, the 64- and 256-record boundaries, changes to cells >= 1089, colour 7, episodes out of
    the buffer, entries out of range, episodes that share records; G = 5 (a block with one goal), scales of both signs
    (a quiet step is paid -0.0), a discount."""
    import gridworld_amd as G
    rec, first, length, starts, targets, at, L = _hand_written()
    dev = torch.device('cuda:0')
    goal = dict(targets=targets) if mode == 'targets' else dict(at=at)
    kw = dict(right_scale=0.3, wrong_scale=-0.7, max_steps=120, gamma=0.95)
    want = RM.relabel(rec, first, length, starts, L=L, **goal, **kw)
    res = G.relabel(torch.from_numpy(rec).to(dev), first, length, torch.from_numpy(starts).to(dev), outputs=ALL, pad=L,
                    **{k: torch.from_numpy(v).to(dev) for k, v in goal.items()}, **kw)
    _same(res, want, mode)
    n = np.clip(length, 0, L)
    inside = (first >= 0) & (first + n <= len(rec))
    assert (want['end'][inside & (n >= 120)] > 0).all() and (want['end'][~inside] == 0).all()
    assert int((want['reward'] > 0).sum()) >= 20 and int((want['reward'] < 0).sum()) >= 20
    assert int((want['reward'].view(np.uint32) == 0x80000000).sum()) >= 20      # -0.0: a quiet step under wrong_scale < 0
    assert int(((want['done'][..., :-1] == 1) & (want['done'][..., 1:] == 0)).sum()) >= 20
    assert (want['target'][~inside] == 0).all() and (want['target_size'][inside, 4] == 0).all()


# ---- 3. the env's own call, under auto-reset --------------------------------------------------------------------------------
def _oracle_episodes(targets, actions, kw, n):
    """The oracle stepped without auto-reset and reset by hand where it is done: per env the list of its finished episodes
    as change-word arrays, and the steps of the running one."""
    from oracle import oracle as O
    ob = O.OracleBatch(n, **kw)
    ob.set_tasks(targets)
    ob.reset()
    prev = ob.grid.copy()
    words, done_eps = [[] for _ in range(n)], [[] for _ in range(n)]
    for a in actions:
        ob.step_walking(a, nthreads=8)
        w = RC.words_of(np.stack([prev, ob.grid]))[:, 0]
        for i in range(n):
            words[i].append(w[i])
            if ob.done[i]:
                done_eps[i].append(np.array(words[i], np.uint16))
                words[i] = []
        if ob.done.any():
            ob.reset(ob.done.astype(bool))
        prev = ob.grid.copy()
    return done_eps, ob


def test_env_relabel_final_under_autoreset_equals_the_oracles_episodes():
    from gridworld_amd import VecGridWorld, workloads
    n, logged, kw = 40, 32, dict(size_reward=False, max_steps=40)
    targets = workloads.rt20(n, seed=21).numpy().astype(np.int8)
    a = np.concatenate([MC.stream(31, n=n), MC.stream(32, n=n), MC.stream(33, n=n)])[:100]
    env = VecGridWorld(n, autoreset=True, **kw)
    env.set_tasks(targets)
    rec, heads = env.enable_trajectory_log(logged)
    env.reset()
    acts = torch.from_numpy(a).to(env.device)
    for t in range(10):
        env.step(acts[t])
    none = env.relabel('final', outputs=ALL)
    assert not none['valid'].any() and not none['length'].any() and tuple(none['reward'].shape) == (logged, 1, 40)
    for k in ALL:
        assert not none[k].any(), k
    for t in range(10, 100):
        env.step(acts[t])
    eps, ob = _oracle_episodes(targets, a, kw, n)
    assert np.array_equal(env.grid.cpu().numpy().reshape(n, -1), ob.grid)
    last = [eps[i][-1] for i in range(logged)]
    # warm (the library is loaded, the allocator has its blocks), then captured: nothing in the call waits for the device
    eager = env.relabel('final', gamma=GAMMA, outputs=ALL)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = env.relabel('final', gamma=GAMMA, outputs=ALL)
    graph.replay()
    torch.cuda.synchronize()
    assert res['valid'].all() and res['valid'].dtype == torch.uint8 and res['length'].dtype == torch.int32
    assert res['length'].tolist() == [len(w) for w in last]
    zero = np.zeros(1089, np.int8)
    for i in range(logged):
        goal = RM.grids_of(zero, last[i])[-1]
        m = RM.episode(zero, last[i], goal, 1.0, 0.1, 40, GAMMA, L=40)
        for k in ('reward', 'done', 'progress'):
            assert np.array_equal(res[k][i, 0].cpu().numpy(), m[k]), (i, k)
        assert int(res['end'][i, 0]) == m['end'] and int(res['target_size'][i, 0]) == m['target_size']
        assert res['ret'][i, 0].cpu().numpy().view(np.uint32) == m['ret'].view(np.uint32)
        assert np.array_equal(res['target'][i, 0].cpu().numpy().reshape(-1), goal)
        assert m['end'] > 0      # what an episode ended with, it completes (or it was empty: done on every step)
    for k in res:
        assert torch.equal(res[k], eager[k]), k
    # entries of the episode: HER's "future" draws, and the same entries as a tensor of targets
    import gridworld_amd as G
    fut = G.relabel_future(res['length'], 3, seed=9)
    assert fut.device == res['length'].device and (fut >= 1).all() and (fut <= res['length'][:, None]).all()
    by_entry = env.relabel(fut, outputs=ALL)
    by_target = env.relabel(by_entry['target'].clone(), outputs=ALL)
    for k in ALL:
        assert torch.equal(by_entry[k], by_target[k]), k
    i, g = 5, 2
    m = RM.episode(zero, last[i], RM.grids_of(zero, last[i])[int(fut[i, g])], 1.0, 0.1, 40, 1.0, L=40)
    assert np.array_equal(by_entry['reward'][i, g].cpu().numpy(), m['reward']) and int(by_entry['end'][i, g]) == m['end']


# ---- 4. the other action spaces: relabel reads only `change` -----------------------------------------------------------------
@pytest.mark.parametrize('space', ['flying', 'walking_dict'])
def test_a_flying_and_a_walking_dict_log_answer(space):
    from gridworld_amd import VecGridWorld, workloads
    from oracle import oracle as O
    n, steps = 32, 30
    kw = dict(size_reward=False, max_steps=steps, **(dict(action_space='flying') if space == 'flying' else dict(discretize=False)))
    targets = workloads.rt20(n, seed=15).numpy().astype(np.int8)
    env = VecGridWorld(n, **kw)
    env.set_tasks(targets)
    env.enable_trajectory_log(n)
    env.reset()
    ob = O.OracleBatch(n, **kw)
    ob.set_tasks(targets)
    ob.reset()
    rng = np.random.RandomState(15)
    grids = [ob.grid.copy()]
    O.use_device_trig(True)
    try:
        for t in range(steps):
            cam = rng.uniform(-5, 5, (n, 2)).astype(np.float32)
            cam[:, 1] = np.where(t < 8, -5.0, cam[:, 1])   # (look down first: something to build on)
            if space == 'flying':
                mv = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
                inv, plc = rng.randint(0, 7, n).astype(np.int32), rng.choice([0, 1, 1, 2], n).astype(np.int32)
                env.step(dict(movement=mv, camera=cam, inventory=inv, placement=plc))
                ob.step_flying(mv, cam, inv, plc)
            else:
                b = (rng.rand(n, 8) < 0.3).astype(np.uint8)
                b[:, 7] = rng.randint(0, 7, size=n) * (rng.rand(n) < 0.3)
                env.step(dict(buttons=b, camera=cam))
                ob.step_walking_dict(b, cam)
            grids.append(ob.grid.copy())
    finally:
        O.use_device_trig(False)
    assert np.array_equal(env.grid.cpu().numpy().reshape(n, -1), ob.grid)
    words = RC.words_of(np.stack(grids))
    final, own = env.relabel('final', outputs=ALL), env.relabel('own', outputs=ALL)
    assert final['valid'].all() and (final['length'] == steps).all()
    zero, changed = np.zeros(1089, np.int8), 0
    for i in range(n):
        changed += int((words[i] != 0xffff).sum())
        for res, goal in ((final, grids[-1][i]), (own, targets[i].reshape(-1))):
            m = RM.episode(zero, words[i], goal, 1.0, 0.1, steps, 1.0)
            for k in ('reward', 'done', 'progress'):
                assert np.array_equal(res[k][i, 0].cpu().numpy(), m[k]), (space, i, k)
            assert int(res['end'][i, 0]) == m['end'] and np.array_equal(res['target'][i, 0].cpu().numpy().reshape(-1), goal)
    print(f'{space}: {changed} logged steps changed a cell')
    assert changed >= 32


# ---- 5. the query moves nothing ---------------------------------------------------------------------------------------------
def test_state_log_and_counters_are_untouched_and_the_next_step_is_that_of_an_env_that_never_asked():
    case = dict(RC.cases()['towers'])
    case['kw'] = dict(case['kw'], max_steps=25)
    (env, rec, heads), (other, rec2, heads2) = _logged(case, steps=25), _logged(case, steps=25)
    before, stats = env.state_dict(), env.stats_tensor().clone()
    log = (rec.clone(), heads.clone())
    res = env.relabel('final', outputs=ALL)
    env.relabel('own')
    torch.cuda.synchronize()
    assert res['valid'].all() and (res['length'] == 25).all()
    after = env.state_dict()
    assert set(after) == set(before)
    for k, v in before.items():
        assert torch.equal(v, after[k]) if torch.is_tensor(v) else v == after[k], k
    assert torch.equal(stats, env.stats_tensor()) and torch.equal(rec, log[0]) and torch.equal(heads, log[1])
    a = torch.from_numpy(case['actions'][25]).to(env.device)
    o1, r1, d1, _ = env.step(a)
    o2, r2, d2, _ = other.step(a)
    assert torch.equal(r1.view(torch.int32), r2.view(torch.int32)) and torch.equal(d1, d2)
    for k in o2:
        assert torch.equal(o1[k].contiguous().view(torch.uint8), o2[k].contiguous().view(torch.uint8)), k
    s1, s2 = env.state_dict(), other.state_dict()
    for k, v in s1.items():
        assert torch.equal(v, s2[k]) if torch.is_tensor(v) else v == s2[k], k
    assert torch.equal(rec, rec2) and torch.equal(heads, heads2)


# ---- 6. out=, single outputs, E = 1, sub-batches, the facade, the logger, the errors ------------------------------------------
def test_out_writes_in_place_past_canary_rows_and_allocates_nothing(logs):
    import gridworld_amd as G
    env, rec, heads, first, length = logs('appendix_b')
    dev, g = env.device, 3
    at = torch.tensor([[T, 24, 0]] * E, dtype=torch.int32, device=dev)
    starts = env.task_start
    ref = G.relabel(rec, first, length, starts, at=at, outputs=ALL)
    specs = G.relabel._specs(E, g, CAP)      # name -> (shape, strides, dtype, alignment, ...)
    base = {k: torch.full((E + 2, strides[0]), 0x55, dtype=dt, device=dev) for k, (_, strides, dt, *_) in specs.items()}
    out = {k: torch.as_strided(base[k], shape, strides, base[k].stride(0)) for k, (shape, strides, *_) in specs.items()}
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated(dev)
    again = G.relabel(rec, first, length, starts, at=at, outputs=ALL, out=out)
    assert torch.cuda.memory_allocated(dev) == held
    torch.cuda.synchronize()
    for k in ALL:
        assert again[k] is out[k]
        assert torch.equal(again[k], ref[k]), k
        assert bool((base[k][0] == 0x55).all()) and bool((base[k][-1] == 0x55).all()), k    # nothing before or behind
    assert bool((_raw_t(out['target'])[..., 1089:] == 0).all())
    some = G.relabel(rec, first, length, starts, at=at, outputs=('end', 'ret'), out={'end': out['end']})
    assert some['end'] is out['end'] and list(some) == ['end', 'ret'] and torch.equal(some['ret'], ref['ret'])


def _raw_t(t):
    e, g = t.shape[:2]
    return torch.as_strided(t, (e, g, ROW), (g * ROW, ROW, 1), t.storage_offset())


def test_a_single_output_a_single_episode_and_no_episode_work(logs):
    import gridworld_amd as G
    env, rec, heads, first, length = logs('towers')
    at = torch.tensor([[T, 5]] * E, dtype=torch.int32, device=env.device)
    ref = G.relabel(rec, first, length, env.task_start, at=at, outputs=ALL)
    for k in ALL:
        one = G.relabel(rec, first, length, env.task_start, at=at, outputs=k)
        assert list(one) == [k] and torch.equal(one[k], ref[k]), k
    i = 7
    one = G.relabel(rec, first[i:i + 1], length[i:i + 1], env.task_start[i:i + 1], at=at[i:i + 1], outputs=ALL)
    for k in ALL:
        assert torch.equal(one[k], ref[k][i:i + 1]), k
    none = G.relabel(rec, first[:0], length[:0], env.task_start[:0], at=at[:0], outputs=ALL)
    assert tuple(none['reward'].shape) == (0, 2, CAP) and tuple(none['target'].shape) == (0, 2, 9, 11, 11)


def test_sub_batches_the_facade_and_the_logger_answer():
    import gridworld_amd as G
    from gridworld_amd.wrappers import EpisodeLogger, Logged
    case = dict(RC.cases()['looking_down'])
    case['kw'] = dict(case['kw'], max_steps=T)
    env, rec, heads = _logged(case)
    whole = env.relabel('final', gamma=GAMMA, outputs=ALL)
    assert whole['valid'].all()
    torch.cuda.synchronize()
    h = E // 2
    for k, s in enumerate(env.split(2)):
        part = s.relabel('final', gamma=GAMMA, outputs=ALL)
        s.synchronize()
        for key in whole:
            assert torch.equal(part[key].contiguous(), whole[key][k * h:(k + 1) * h].contiguous()), key
    b, grids = RC.base('looking_down'), RC.goal_grids('looking_down')
    # the logger: the episodes collect() returns, relabelled from their own grid sequences
    from gridworld_amd import VecGridWorld
    vec = VecGridWorld(E, **case['kw'])
    vec.set_tasks(case['targets'])
    log = EpisodeLogger(vec, n_envs=4, capacity=CAP)
    vec.reset()
    acts = torch.from_numpy(case['actions']).to(vec.device)
    for t in range(T):
        vec.step(acts[t])
    eps = log.collect(dump=False)
    assert len(eps) == 4 and log.relabel(goals='final', gamma=GAMMA, outputs=ALL) is not None
    fin = RC.GOALS.index('final')
    for ep in eps:
        i = ep['env']
        m = RM.episode(b['starts'][i], b['change'][i], grids[i, fin], RC.RIGHT, RC.WRONG, T, GAMMA)
        assert ep['reward_relabel'].shape == (1, T) and np.array_equal(ep['reward_relabel'][0], m['reward'])
        assert np.array_equal(ep['done_relabel'][0], m['done']) and ep['end_relabel'][0] == m['end']
        assert ep['ret_relabel'].view(np.uint32)[0] == m['ret'].view(np.uint32)
        assert np.array_equal(ep['target_relabel'][0].reshape(-1), grids[i, fin])
        assert np.array_equal(whole['reward'][i, 0, :T].cpu().numpy(), m['reward'])
    log.relabel(eps[:2], goals='own', outputs=('reward',))
    assert np.array_equal(eps[0]['reward_relabel'][0], eps[0]['reward'].astype(np.float32))
    log.relabel(eps[:2], goals=[5, 24], outputs=('end',))
    assert eps[1]['end_relabel'].shape == (2,)
    # the facade: its one env, its last finished episode
    col = 3
    f = Logged(G.make('IGLUGridworldVector-v0', size_reward=False, max_steps=T))
    f.set_task(G.Task('', case['targets'][col].astype(np.int32)))
    f.reset()
    for t in range(T):
        _, _, done, _ = f.step(int(case['actions'][t, col]))
    assert done
    got = f.unwrapped.relabel('final', gamma=GAMMA)
    m = RM.episode(b['starts'][col], b['change'][col], grids[col, fin], RC.RIGHT, RC.WRONG, T, GAMMA)
    assert list(got) == ['reward', 'done', 'end', 'ret', 'length', 'valid'] and got['valid'] == 1 and got['length'] == T
    assert got['reward'].shape == (1, T) and np.array_equal(got['reward'][0], m['reward']) and got['end'][0] == m['end']
    two = f.unwrapped.relabel([5, T], outputs=('end', 'target_size'))
    assert two['end'].shape == (2,) and two['end'][1] == m['end']


def test_the_value_errors_are_raised():
    from gridworld_amd import VecGridWorld
    case = RC.cases()['looking_down']
    env, rec, heads = _logged(case, n=8, steps=2)
    dev = env.device
    for outputs in ((), ('gain',), ('reward', 'word'), 'rewards'):
        with pytest.raises(ValueError):
            env.relabel('final', outputs=outputs)
    for goals in ('last', torch.zeros((7, 2), dtype=torch.int32, device=dev), torch.zeros((8, 2)), torch.zeros((8, 2, 7), dtype=torch.int8),
                  torch.zeros((8, 257), dtype=torch.int32), torch.zeros((8,), dtype=torch.int32)):
        with pytest.raises(ValueError):
            env.relabel(goals)
    with pytest.raises(ValueError):
        env.relabel('final', out={'reward': torch.zeros((8, 1, CAP - 1), device=dev)})
    with pytest.raises(ValueError):
        env.relabel('final', outputs=('end',), out={'reward': torch.zeros((8, 1, CAP), device=dev)})
    with pytest.raises(ValueError):
        env.relabel('final', gamma=float('inf'))
    ok = env.relabel('final')
    assert not ok['valid'].any() and tuple(ok['reward'].shape) == (8, 1, CAP)
    parts = env.split(2)
    env.disable_trajectory_log()
    with pytest.raises(ValueError, match='episode log'):
        env.relabel('final')
    env.enable_trajectory_log(2)
    with pytest.raises(ValueError, match='logged'):
        parts[1].relabel('final')            # envs 4..7: the log holds the first two
    assert tuple(parts[0].relabel('final')['reward'].shape) == (2, 1, 250)
    sized = VecGridWorld(2, size_reward=True)
    sized.set_tasks(case['targets'][:2])
    sized.enable_trajectory_log(2)
    with pytest.raises(ValueError, match='size_reward=True'):
        sized.relabel('final')
