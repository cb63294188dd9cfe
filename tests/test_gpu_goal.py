"""The goal query (igw_goal, VecGridWorld.goal, obs['align'] / ['fit'] / ['todo']) on the GPU.
One yardstick, exact (0 mismatches; gain as float32 bit patterns): the CPU oracle -- its stateless Task evaluation for
the alignment, the aligned target and what is left of it, its own step for the reward and `done` of every action
(tests/goal_cases.py).

Against the oracle: 7 cases x 6 checkpoints x 32 envs, and 2,049 auto-resetting envs (whole wavefronts and a tail) at
three points of a random rollout, the rewards there against nine oracle blocks."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import goal_cases as GC
import mask_cases as MC

pytestmark = pytest.mark.gpu

E = GC.E
KEYS = ('align', 'fit', 'want', 'todo', 'gain', 'ends')


def _gpu_env(case, **kw):
    from gridworld_amd import VecGridWorld
    env = VecGridWorld(E, **dict(case['kw'], **kw))
    env.set_tasks(case['targets'], case['starts'], init_pose=case['poses'])
    return env


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def _mismatches(got, want, keys=KEYS):
    """Per output the number of elements that differ (gain: as bit patterns)."""
    bad = {}
    for k in keys:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (k, a.shape, b.shape, a.dtype, b.dtype)
        if k == 'gain':
            a, b = a.view(np.uint32), b.view(np.uint32)
        bad[k] = int((a != b).sum())
    return bad


# ---- 1. against the oracle, case by case ------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(GC.cases()))
def test_all_six_outputs_equal_the_oracle_truth(name):
    case, truth = GC.cases()[name], GC.truth(name)
    env = _gpu_env(case)
    env.reset()
    acts = torch.from_numpy(case['actions']).to(env.device)
    t, total = 0, dict.fromkeys(KEYS, 0)
    for c, tc in enumerate(GC.CHECKPOINTS):
        while t < tc:
            env.step(acts[t])
            t += 1
        res = env.goal(want=True, todo=True, gain=True)
        assert list(res) == list(KEYS)
        assert res['align'].dtype == torch.int8 and tuple(res['align'].shape) == (E, 3)
        assert res['fit'].dtype == torch.int16 and tuple(res['fit'].shape) == (E, 4)
        assert res['want'].dtype == torch.int8 and tuple(res['todo'].shape) == (E, 9, 11, 11)
        assert res['want'].stride() == env.grid.stride() == res['todo'].stride()
        assert res['gain'].dtype == torch.float32 and res['ends'].dtype == torch.uint8
        assert tuple(res['gain'].shape) == tuple(res['ends'].shape) == (E, 18)
        for k, v in _mismatches(_np(res), {k: truth[k][c] for k in KEYS}).items():
            total[k] += v
    print(f'{name}: elements that differ from the oracle: {total}')
    assert not any(total.values())


# ---- 2. whole wavefronts and a tail, auto-reset, against the oracle model -----------------------------------------------
B = 2049
THREADS = min(16, os.cpu_count() or 1)


def _oracle_blocks(targets, blocks, **kw):
    """An OracleBatch of `blocks` copies of the envs of `targets` (no starting grids), reset: Task.__init__ and reset of
    every env in a thread pool (the oracle's envs share nothing; its calls release the interpreter lock)."""
    from oracle import oracle as O
    n = blocks * len(targets)
    ob, lib = O.OracleBatch(n, **kw), O.lib()

    def prepare(lo):
        for i in range(lo, min(lo + 128, n)):
            ob.envs[i].set_task(targets[i % len(targets)])
            lib.igo_reset(ob.envs[i].h)
    with ThreadPoolExecutor(THREADS) as pool:
        list(pool.map(prepare, range(0, n, 128)))
    return ob     # (ob.grid is the empty grid the reset left)


def _oracle_rows(ob, targets, starts, rows):
    out = dict(align=np.zeros((len(rows), 3), np.int8), fit=np.zeros((len(rows), 4), np.int16),
               want=np.zeros((len(rows), 9, 11, 11), np.int8), todo=np.zeros((len(rows), 9, 11, 11), np.int8))
    for k, i in enumerate(rows):
        out['align'][k], out['fit'][k], out['want'][k], out['todo'][k] = GC.env_truth(
            targets[i], starts[i], ob.grid[i].reshape(9, 11, 11), ob.envs[i].task_state()['syn_max_int'])
    return out


def test_a_stepped_autoreset_batch_equals_the_oracle_model():
    from gridworld_amd import VecGridWorld, workloads
    kw = dict(size_reward=False, max_steps=40)
    targets = workloads.rt20(B, seed=14).numpy().astype(np.int8)
    starts = np.zeros_like(targets)
    env = VecGridWorld(B, autoreset=True, **kw)
    env.set_tasks(targets)
    env.reset()
    ob = _oracle_blocks(targets, 9, **kw)
    # the looking-down stream (40 % place, 15 % break) with the look-down actions again after the time limit's reset
    a = MC.stream(21, n=B)
    a = np.concatenate([a[:40], a[:20]])
    acts = torch.from_numpy(a).to(env.device)
    bad = {}
    for t in range(61):
        if t in (0, 20, 60):
            got = _np(env.goal(want=True))
            bad[t] = _mismatches(got, _oracle_rows(ob, targets, starts, range(B)), ('align', 'fit', 'want', 'todo'))
            print(f'step {t}: live max_int > 0 in {int((got["fit"][:, 0] > 0).sum())} envs, aligned off the origin in '
                  f'{int(got["align"].any(1).sum())}; elements that differ: {bad[t]}')
        if t < 60:
            env.step(acts[t])
            ob.step_walking(np.tile(a[t], 9), autoreset=True, nthreads=THREADS)
    got = _np(env.goal(todo=False, gain=True))
    assert list(got) == ['align', 'fit', 'gain', 'ends']
    ob.step_walking(np.concatenate([np.zeros(B, np.int32)] + [np.full(B, p, np.int32) for p in GC.PROBES]), nthreads=THREADS)
    gain, ends = np.repeat(ob.reward[:B, None], 18, 1), np.repeat(ob.done[:B, None], 18, 1)
    for j, p in enumerate(GC.PROBES):
        gain[:, p], ends[:, p] = ob.reward[(j + 1) * B:(j + 2) * B], ob.done[(j + 1) * B:(j + 2) * B]
    bad['gain'] = _mismatches(got, dict(gain=gain, ends=ends), ('gain', 'ends'))
    print(f'step 60: {int((gain != 0).sum())} of {gain.size} rewards are not 0; elements that differ: {bad["gain"]}')
    assert (gain != 0).sum() >= 1000 and (got['fit'][:, 0] > 0).sum() >= 200
    assert not any(v for d in bad.values() for v in d.values())


def test_a_flying_batch_answers_the_action_free_outputs():
    from gridworld_amd import VecGridWorld, workloads
    from oracle import oracle as O
    n, kw = 64, dict(size_reward=False, max_steps=40, action_space='flying')
    targets = workloads.rt20(n, seed=15).numpy().astype(np.int8)
    env = VecGridWorld(n, autoreset=True, **kw)
    env.set_tasks(targets)
    env.reset()
    ob = O.OracleBatch(n, **kw)
    ob.set_tasks(targets)
    ob.reset()
    rng = np.random.RandomState(15)
    O.use_device_trig(True)
    try:
        for t in range(30):
            mv = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
            cam = rng.uniform(-5, 5, (n, 2)).astype(np.float32)
            cam[:, 1] = np.where(t < 8, -5.0, cam[:, 1])   # (look down first: something to build on)
            inv, plc = rng.randint(0, 7, n).astype(np.int32), rng.choice([0, 1, 1, 2], n).astype(np.int32)
            env.step(dict(movement=mv, camera=cam, inventory=inv, placement=plc))
            ob.step_flying(mv, cam, inv, plc, autoreset=True)
    finally:
        O.use_device_trig(False)
    assert np.array_equal(env.grid.cpu().numpy().reshape(n, -1), ob.grid)
    got = _np(env.goal(want=True))
    bad = _mismatches(got, _oracle_rows(ob, targets, np.zeros_like(targets), range(n)), ('align', 'fit', 'want', 'todo'))
    print(f'flying: {int((got["fit"][:, 2] > 0).sum())} envs have built; elements that differ: {bad}')
    assert (got['fit'][:, 2] > 0).sum() >= 8 and not any(bad.values())


# ---- 3. the observation tensors follow the state ---------------------------------------------------------------------
def _fresh_equals_held(env, held):
    fresh = env.goal(want='want' in held, todo='todo' in held, gain='gain' in held)
    assert list(fresh) == list(held)
    for k in held:
        assert fresh[k].data_ptr() != held[k].data_ptr()
        a, b = fresh[k].contiguous(), held[k].contiguous()
        assert torch.equal(a.view(torch.int32) if k == 'gain' else a, b.view(torch.int32) if k == 'gain' else b), k


def test_obs_goal_follows_reset_step_rollout_load_and_replay():
    case = GC.cases()['looking_down']
    env = _gpu_env(case, autoreset=True, goal=('want', 'todo', 'gain'), max_steps=30)
    acts = torch.from_numpy(case['actions']).to(env.device)
    obs = env.reset()
    held = {k: obs[k] for k in KEYS}
    assert held['todo'].stride() == env.grid.stride() and tuple(held['align'].shape) == (E, 3)
    _fresh_equals_held(env, held)
    seen = 0
    for t in range(34):   # the time limit ends every episode at step 30: the tensors then show the new episode's state
        obs, _, done, _ = env.step(acts[t])
        assert all(obs[k] is held[k] for k in KEYS)
        _fresh_equals_held(env, held)
        seen = max(seen, int((held['fit'][:, 0] > 0).sum()))
        if t == 29:
            assert done.all() and int(held['fit'][:, 2].abs().sum()) == 0 and not bool(held['align'].any())
    assert seen >= 8
    env.rollout_actions(acts[34:40].contiguous())
    _fresh_equals_held(env, held)
    state = env.state_dict()
    before = {k: v.clone() for k, v in held.items()}
    env.step(acts[40])
    env.step(acts[41])
    env.load_state_dict(state)
    for k in KEYS:
        assert torch.equal(before[k].contiguous().view(torch.uint8), held[k].contiguous().view(torch.uint8)), k
    for chains in (1, 2):
        g = env.capture_steps(acts[40:46].contiguous(), chains=chains)
        obs, _, _, _ = g.replay()
        assert all(obs[k] is held[k] for k in KEYS)
        _fresh_equals_held(env, held)
        env.step(acts[46])
        g.replay()
        _fresh_equals_held(env, held)
        del g
    # the default, goal=True: align, fit and todo
    env2 = _gpu_env(case, goal=True)
    obs = env2.reset()
    assert {'align', 'fit', 'todo'} <= set(obs) and not {'want', 'gain', 'ends'} & set(obs)


def test_sub_batches_query_their_own_rows_on_their_own_stream():
    case = GC.cases()['towers']
    env = _gpu_env(case, goal=('todo', 'gain'))
    env.reset()
    acts = torch.from_numpy(case['actions']).to(env.device)
    for t in range(12):
        env.step(acts[t])
    whole = env.goal(gain=True)
    subs = env.split(2)
    h = E // 2
    for k, s in enumerate(subs):
        part = s.goal(gain=True)
        s.synchronize()
        rows = slice(k * h, (k + 1) * h)
        for key in whole:
            assert torch.equal(part[key].contiguous().view(torch.uint8), whole[key][rows].contiguous().view(torch.uint8)), key
        assert s.obs()['todo'].data_ptr() == env.obs()['todo'][rows].data_ptr()
    for k, s in enumerate(subs):                    # stepped on its own: its rows of the held tensors follow
        s.step_walking_ptr(acts[12, k * h:(k + 1) * h].contiguous())
        s.join()
    _fresh_equals_held(env, {k: env.obs()[k] for k in ('align', 'fit', 'todo', 'gain', 'ends')})


# ---- 4. out= -------------------------------------------------------------------------------------------------------------
def test_out_writes_in_place_and_allocates_nothing():
    case = GC.cases()['appendix_b']
    env = _gpu_env(case)
    env.reset()
    acts = torch.from_numpy(case['actions']).to(env.device)
    for t in range(25):
        env.step(acts[t])
    keys = ('agent_buf', 'occ_buf', 'grid_buf', 'aux_buf', 'out_buf', 'hist_buf', 'task_target', 'task_start',
            'task_meta', 'task_index')
    before = {k: getattr(env, k).clone() for k in keys}
    first = env.goal(want=True, gain=True)
    torch.cuda.synchronize()
    for k in keys:                                   # the query writes nothing but its outputs
        assert torch.equal(getattr(env, k), before[k]), k
    out = {k: torch.full_like(v, 85) for k, v in first.items()}   # (full_like keeps the strides of the views)
    out['align'] = torch.as_strided(torch.full((E, 4), 85, dtype=torch.int8, device=env.device), (E, 3), (4, 1))
    out['want'] = torch.as_strided(torch.full((E, 1104), 85, dtype=torch.int8, device=env.device), (E, 9, 11, 11),
                                   (1104, 121, 11, 1))
    out['todo'] = torch.as_strided(torch.full((E, 1104), 85, dtype=torch.int8, device=env.device), (E, 9, 11, 11),
                                   (1104, 121, 11, 1))
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated(env.device)
    again = env.goal(want=True, gain=True, out=out)
    assert torch.cuda.memory_allocated(env.device) == held
    for k in first:
        assert again[k] is out[k]
        assert torch.equal(again[k].contiguous().view(torch.uint8), first[k].contiguous().view(torch.uint8)), k
    # the pad bytes of both rows are written as 0
    for k in ('want', 'todo'):
        raw = torch.as_strided(out[k], (E, 1104), (1104, 1))
        assert not bool(raw[:, 1089:].any()), k
    some = env.goal(out={'fit': out['fit']})         # the rest is allocated
    assert some['fit'] is out['fit'] and some['todo'] is not out['todo']
    with pytest.raises(ValueError):
        env.goal(out={'fit': torch.zeros((E, 3), dtype=torch.int16, device=env.device)})
    with pytest.raises(ValueError):
        env.goal(out={'todo': torch.zeros((E, 9, 11, 11), dtype=torch.int8, device=env.device)})   # not the rows' stride
    with pytest.raises(ValueError):
        env.goal(todo=False, out={'todo': out['todo']})


# ---- 5. the facade ---------------------------------------------------------------------------------------------------------
def test_the_facade_answers_for_its_one_env():
    import gridworld_amd as G
    from gridworld_amd import VecGridWorld
    case, col = GC.cases()['recolour'], 0
    vec = VecGridWorld(1, **case['kw'])
    vec.set_tasks(case['targets'][:1], case['starts'][:1])
    vec.reset()
    env = G.make('IGLUGridworldVector-v0', size_reward=False)
    start = [(x - 5, y - 1, z - 5, int(case['starts'][col, y, x, z]))
             for y, x, z in zip(*np.nonzero(case['starts'][col]))]
    env.set_task(G.Task('', case['targets'][col].astype(np.int32), starting_grid=start))
    env.reset()
    for t in range(26):
        got, want = env.unwrapped.goal(), _np(vec.goal(want=True, gain=True))
        assert list(got) == list(KEYS) and got['ends'].dtype == np.bool_
        for k in KEYS:
            assert isinstance(got[k], np.ndarray) and np.array_equal(got[k], want[k][0].astype(got[k].dtype)), (t, k)
        a = int(case['actions'][t, col])
        obs, reward, done, info = env.step(a)
        assert info == {} and not set(obs) & set(KEYS)   # obs and info stay the reference's
        assert np.float32(reward) == got['gain'][a] and done == got['ends'][a]   # the prediction, one step on
        vec.step(torch.tensor([a], dtype=torch.int32))
    truth = GC.truth('recolour')
    assert np.array_equal(got['gain'].view(np.uint32), truth['gain'][4, col].view(np.uint32))   # step 25 is a checkpoint
    # goal_world: the block ids wanted, from want + start (here the target sits one cell off its own frame: the block
    # that matches is the second of its row)
    start = vec.task_start[vec.env_task.long()][:, :1089].reshape(1, 9, 11, 11)
    fresh = vec.goal(want=True)
    world, wanted = G.goal_world(fresh['want'], start).cpu().numpy(), fresh['want'].cpu().numpy()
    w = wanted.astype(np.int16) + start.cpu().numpy()
    assert np.array_equal(world, np.where((w >= 0) & (w <= 6), w, -1)) and world.dtype == np.int8
    assert sorted(world[wanted != 0].tolist()) == [1, 2, 3] and fresh['align'][0].tolist() == [0, -1, 0]


# ---- 6. errors -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kw', [dict(action_space='flying'), dict(discretize=False), dict(size_reward=True)])
def test_gain_raises_where_it_is_not_defined(kw):
    import gridworld_amd as G
    from gridworld_amd import VecGridWorld, workloads
    kw = dict(dict(size_reward=False), **kw)
    env = VecGridWorld(4, **kw)
    env.set_tasks(workloads.rt20(4, seed=1).numpy())
    env.reset()
    with pytest.raises(ValueError):
        env.goal(gain=True)
    with pytest.raises(ValueError):
        VecGridWorld(4, goal=('gain',), **kw)
    with pytest.raises(ValueError):
        VecGridWorld(4, goal=('reward',), **kw)
    res = env.goal(want=True)                        # the action-free outputs work everywhere
    assert list(res) == ['align', 'fit', 'want', 'todo']
    if not kw['size_reward']:
        one = G.make('IGLUGridworldVector-v0', **kw)
        one.set_task(G.Task('', workloads.rt20(1, seed=1).numpy()[0].astype(np.int32)))
        one.reset()
        assert list(one.unwrapped.goal()) == ['align', 'fit', 'want', 'todo']
