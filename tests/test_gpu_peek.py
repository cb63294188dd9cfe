"""The peek query (igw_peek, VecGridWorld.peek) on the GPU.  Every word of every output is compared,
reward, pose and ret as bit patterns.  Yardsticks: the CPU oracle (tests/peek_cases.py), the step path itself (a
second batch of E * K rows stepped H times), goal(gain=True) and action_mask(look=True) for H = 1, and the state's own
tensors before and after."""
import numpy as np
import pytest
import torch

import mask_cases as MC
import peek_cases as PC

pytestmark = pytest.mark.gpu

KEYS = ('reward', 'ends', 'change', 'pose', 'ret')
DTYPES = dict(reward=torch.float32, ends=torch.int16, change=torch.int16, pose=torch.float32, ret=torch.float32)


def _gpu_env(case, **kw):
    from gridworld_amd import VecGridWorld
    env = VecGridWorld(len(case['targets']), **dict(case['kw'], **kw))
    env.set_tasks(case['targets'], case['starts'], init_pose=case['poses'])
    return env


def _dev(a, env):
    return torch.from_numpy(np.array(a)).to(env.device)


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _mismatches(got, want, keys=KEYS):
    """Per output the number of elements that differ (float32 as bit patterns)."""
    bad = {}
    for k in keys:
        a, b = _bits(got[k]), _bits(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (k, a.shape, b.shape, a.dtype, b.dtype)
        bad[k] = int((a != b).sum())
    return bad


def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k].view(torch.int32 if a[k].dtype == torch.float32 else a[k].dtype),
                           b[k].view(torch.int32 if b[k].dtype == torch.float32 else b[k].dtype)), k


# ---- 1. against the oracle, case by case ------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(PC.cases()))
def test_all_five_outputs_equal_the_oracle_truth(name):
    total = dict.fromkeys(KEYS, 0)
    case, n = PC.cases()[name], PC.E
    env = _gpu_env(case)
    env.reset()
    acts = torch.from_numpy(case['actions']).to(env.device)
    t = 0
    for tc in PC.CHECKPOINTS:
        while t < tc:
            env.step(acts[t])
            t += 1
        for cset in PC.SETS:
            cand = _dev(PC.candidates(cset), env)
            K, H = cand.shape[-2:]
            truth = PC.truth(name, tc, cset)
            for gamma in PC.GAMMAS:
                res = env.peek(cand, gamma=gamma)
                assert list(res) == list(KEYS)
                for k, shape in dict(reward=(n, K, H), ends=(n, K), change=(n, K, H), pose=(n, K, 5), ret=(n, K)).items():
                    assert res[k].dtype == DTYPES[k] and tuple(res[k].shape) == shape and res[k].is_contiguous(), k
                bad = _mismatches(_np(res), dict(truth, ret=truth['ret'][gamma]))
                if any(bad.values()):
                    print(f'{name} {cset} checkpoint {tc} gamma {gamma}: {bad}')
                for k, v in bad.items():
                    total[k] += v
    print(f'{name}: elements that differ from the oracle: {total}')
    assert not any(total.values())


# ---- 2. against the step path --------------------------------------------------------------------------------------------
def test_peek_equals_the_step_path_on_replicated_rows():
    """37 envs x 70 random candidates x 32 steps against a second batch of 37 * 70 rows (row k * 37 + i = copy k of env
    i: the same tasks, the same 12-step prefix) stepped 32 times through env.step() without auto-reset."""
    from gridworld_amd import VecGridWorld, workloads
    E, K, H, T0 = 37, 70, 32, 12
    kw = dict(size_reward=False, max_steps=250, autoreset=False)
    targets = workloads.rt20(E, seed=5).numpy().astype(np.int8)
    env, big = VecGridWorld(E, **kw), VecGridWorld(E * K, **kw)
    env.set_tasks(targets)
    big.set_tasks(np.tile(targets, (K, 1, 1, 1)))
    env.reset()
    big.reset()
    prefix = torch.from_numpy(MC.stream(8, n=E)[:T0]).to(env.device)
    for t in range(T0):
        env.step(prefix[t])
        big.step(prefix[t].repeat(K))
    cand_np = PC.random_candidates(77, n=E, k=K, h=H)
    cand = torch.from_numpy(cand_np).to(env.device)
    got = _np(env.peek(cand))
    rows = E * K
    reward, change = np.zeros((rows, H), np.float32), np.full((rows, H), -1, np.int16)
    ends, pose = np.zeros(rows, np.int16), np.zeros((rows, 5), np.float32)
    live, ar = np.ones(rows, bool), np.arange(rows)
    before = big.grid.reshape(rows, -1).cpu().numpy()
    for h in range(H):
        big.step(cand[:, :, h].t().reshape(-1))
        grid = big.grid.reshape(rows, -1).cpu().numpy()
        diff = grid != before
        assert (diff.sum(1) <= 1).all()
        cell = diff.argmax(1)
        code = np.where(diff.any(1), (grid[ar, cell].astype(np.int32) << 11) | cell, -1)
        reward[live, h], change[live, h] = big.reward.cpu().numpy()[live], code[live]
        pose[live] = big.agent_pos.cpu().numpy()[live]
        ended = live & (big.done.cpu().numpy() != 0)
        ends[ended] = h + 1
        live &= ~ended
        before = grid
    by_env = lambda x: np.ascontiguousarray(np.swapaxes(x.reshape((K, E) + x.shape[1:]), 0, 1))  # noqa: E731
    want = dict(reward=by_env(reward), ends=by_env(ends), change=by_env(change), pose=by_env(pose))
    bad = _mismatches(got, want, ('reward', 'ends', 'change', 'pose'))
    print(f'{int((want["change"] >= 0).sum())} changes, {int((want["reward"] != 0).sum())} rewards that are not 0, '
          f'{int((want["ends"] > 0).sum())} candidates end; elements that differ from the step path: {bad}')
    assert (want['change'] >= 0).sum() >= 1000 and (want['reward'] != 0).sum() >= 1000
    assert not any(bad.values())


# ---- 3. H = 1 against goal(gain=True) and action_mask(look=True) -----------------------------------------------------------
@pytest.mark.parametrize('name', ['looking_down', 'towers', 'recolour', 'select_only'])
def test_one_step_of_each_action_equals_goal_and_action_mask(name):
    case = PC.cases()[name]
    env = _gpu_env(case)
    env.reset()
    acts = torch.from_numpy(case['actions']).to(env.device)
    cand = torch.arange(18, dtype=torch.int32, device=env.device).reshape(18, 1)
    t = 0
    for tc in PC.CHECKPOINTS:
        while t < tc:
            env.step(acts[t])
            t += 1
        p = _np(env.peek(cand))
        g = _np(env.goal(todo=False, gain=True))
        mask, look = (x.cpu().numpy() for x in env.action_mask(look=True))
        known = ~np.isnan(g['gain'])
        assert known.sum() >= 17 * PC.E
        assert np.array_equal(p['reward'][:, :, 0].view(np.uint32)[known], g['gain'].view(np.uint32)[known])
        assert np.array_equal(p['ends'] != 0, g['ends'] != 0)
        change = p['change'][:, :, 0].astype(np.int32)
        cell = np.where(change >= 0, change & 0x7ff, -1)
        assert np.array_equal(cell[:, 16], look[:, 0]) and np.array_equal(cell[:, 17], look[:, 1])
        assert (cell[mask == 0] == -1).all()
        assert (cell[:, [0, 1, 2, 3, 4, 5, 12, 13, 14, 15]] == -1).all()
        if case['kw'].get('select_and_place', True):
            assert np.array_equal(cell[:, 6:12] >= 0, mask[:, 6:12] != 0)
        else:
            assert (cell[:, 6:12] == -1).all()


# ---- 4. the state is untouched ---------------------------------------------------------------------------------------------
def test_peek_leaves_the_state_as_it_was():
    case = PC.cases()['towers']
    env, ref = _gpu_env(case), _gpu_env(case)
    acts = torch.from_numpy(case['actions']).to(env.device)
    env.reset()
    ref.reset()
    for t in range(14):
        env.step(acts[t])
        ref.step(acts[t])
    torch.cuda.synchronize()
    state = {k: v.clone() for k, v in env.state_dict().items() if torch.is_tensor(v)}
    stats = env.stats_tensor().clone()
    assert len(state) >= 5
    env.peek(_dev(PC.candidates('random'), env))
    env.peek(_dev(PC.candidates('directed'), env), gamma=0.5)
    torch.cuda.synchronize()
    after = env.state_dict()
    for k, v in state.items():
        assert torch.equal(v.contiguous().view(torch.uint8), after[k].contiguous().view(torch.uint8)), k
    assert torch.equal(stats, env.stats_tensor())
    env.step(acts[14])
    ref.step(acts[14])
    torch.cuda.synchronize()
    a, b = env.state_dict(), ref.state_dict()
    for k in state:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(env.reward, ref.reward) and torch.equal(env.done, ref.done)
    assert torch.equal(env.agent_pos.view(torch.int32), ref.agent_pos.view(torch.int32))


# ---- 5. layouts ----------------------------------------------------------------------------------------------------------
def _stepped(name='looking_down', steps=14, **kw):
    case = PC.cases()[name]
    env = _gpu_env(case, **kw)
    env.reset()
    acts = torch.from_numpy(case['actions']).to(env.device)
    for t in range(steps):
        env.step(acts[t])
    return env


def test_shared_candidates_equal_the_same_candidates_per_env():
    env = _stepped()
    cand = _dev(PC.candidates('directed'), env)
    _same(env.peek(cand), env.peek(cand.unsqueeze(0).expand(PC.E, -1, -1)))
    _same(env.peek(cand), env.peek(PC.candidates('directed').astype(np.int64)))


def test_wide_actions_outside_the_range_are_no_ops():
    """An int64 value that would wrap into 0..17 when narrowed to int32 (17 + 2^32, 16 - 2^32, 5 + 2^40) is the no-op the
    contract says, in a tensor and in an array."""
    env = _stepped()
    wide = torch.tensor([[17 + (1 << 32), 16 - (1 << 32), 5 + (1 << 40), 17, -1, 18, 1 << 31, 16]], dtype=torch.int64)
    same = torch.tensor([[-1, -1, -1, 17, -1, -1, -1, 16]], dtype=torch.int32, device=env.device)
    want = env.peek(same)
    assert int((want['change'] >= 0).sum()) > 0
    _same(env.peek(wide.to(env.device)), want)
    _same(env.peek(wide), want)
    _same(env.peek(wide.numpy()), want)


@pytest.mark.parametrize('K', [1, 63, 64, 65])
@pytest.mark.parametrize('H', [1, 32])
def test_chunk_and_step_boundaries(K, H):
    """K around the 64 candidates of a block, H at its ends: a candidate's answers do not depend on its neighbours."""
    env = _stepped('towers')
    full = torch.from_numpy(PC.random_candidates(5, k=65, h=32)).to(env.device)
    whole = env.peek(full)
    part = env.peek(full[:, :K, :H].contiguous())
    ended = (whole['ends'][:, :K] > 0) & (whole['ends'][:, :K] <= H)
    assert torch.equal(part['reward'].view(torch.int32), whole['reward'][:, :K, :H].view(torch.int32))
    assert torch.equal(part['change'], whole['change'][:, :K, :H])
    assert torch.equal(part['ends'], torch.where(ended, whole['ends'][:, :K], torch.zeros_like(part['ends'])))
    if H == 32:
        assert torch.equal(part['pose'].view(torch.int32), whole['pose'][:, :K].view(torch.int32))
        assert torch.equal(part['ret'].view(torch.int32), whole['ret'][:, :K].view(torch.int32))


def test_a_subset_of_outputs_and_out_in_place_with_canaries():
    env = _stepped()
    dev = env.device
    cand = _dev(PC.candidates('random'), env)
    n, K, H = cand.shape
    whole = env.peek(cand, gamma=0.97)
    some = env.peek(cand, gamma=0.97, outputs=('ret', 'ends'))
    assert list(some) == ['ends', 'ret']
    _same(some, {k: whole[k] for k in ('ends', 'ret')})
    # out=: rows [0, n) of longer buffers, canary rows behind them
    sizes = dict(reward=K * H, ends=K, change=K * H, pose=K * 5, ret=K)
    shapes = dict(reward=(n, K, H), ends=(n, K), change=(n, K, H), pose=(n, K, 5), ret=(n, K))
    bufs = {k: torch.full((n + 2, sizes[k]), 0x55, dtype=torch.uint8, device=dev).repeat(1, DTYPES[k].itemsize).view(DTYPES[k])
            for k in KEYS}
    out = {k: bufs[k][:n].view(shapes[k]) for k in KEYS}
    canary = {k: bufs[k][n:].clone() for k in KEYS}
    res = env.peek(cand, gamma=0.97, out=out)
    for k in KEYS:
        assert res[k].data_ptr() == out[k].data_ptr()
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated(dev)
    res = env.peek(cand, gamma=0.97, out=out)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(dev) == held
    _same(res, whole)
    for k in KEYS:
        assert torch.equal(bufs[k][n:].view(torch.uint8), canary[k].view(torch.uint8)), k


def test_a_sub_batch_on_its_own_stream_equals_the_parents_rows():
    env = _stepped('towers')
    cand = _dev(PC.candidates('random'), env)
    whole = env.peek(cand)
    torch.cuda.synchronize()
    lo = 0
    for sub in env.split(2):
        n = sub.num_envs
        part = sub.peek(cand[lo:lo + n].contiguous())
        sub.synchronize()
        _same(part, {k: v[lo:lo + n] for k, v in whole.items()})
        shared = sub.peek(_dev(PC.candidates('directed'), env), outputs=('ret',))
        sub.synchronize()
        assert tuple(shared['ret'].shape) == (n, len(PC.DIRECTED_NAMES))
        lo += n
    assert lo == PC.E


def test_errors():
    from gridworld_amd import VecGridWorld
    env = _stepped(steps=0)
    dev = env.device
    ok = torch.zeros((4, 3), dtype=torch.int32, device=dev)
    bad = [dict(actions=torch.zeros(3, dtype=torch.int32, device=dev)), dict(actions=torch.zeros((2, 2, 2, 2), dtype=torch.int32, device=dev)),
           dict(actions=torch.zeros((PC.E + 1, 4, 3), dtype=torch.int32, device=dev)), dict(actions=torch.zeros((4, 33), dtype=torch.int32, device=dev)),
           dict(actions=torch.zeros((4097, 1), dtype=torch.int32, device=dev)), dict(actions=torch.zeros((0, 3), dtype=torch.int32, device=dev)),
           dict(actions=torch.zeros((4, 0), dtype=torch.int32, device=dev)), dict(actions=torch.zeros((4, 3), device=dev)),
           dict(actions=ok, outputs=()), dict(actions=ok, outputs=('ret', 'gain')),
           dict(actions=ok, out=dict(gain=torch.zeros((PC.E, 4), device=dev))),
           dict(actions=ok, outputs=('ret',), out=dict(ends=torch.zeros((PC.E, 4), dtype=torch.int16, device=dev))),
           dict(actions=ok, out=dict(ret=torch.zeros((PC.E, 5), device=dev))),
           dict(actions=ok, out=dict(ret=torch.zeros((PC.E, 4), dtype=torch.float64, device=dev))),
           dict(actions=ok, out=dict(ret=torch.zeros((PC.E, 4)))),
           dict(actions=ok, out=dict(ret=torch.zeros((PC.E, 8), device=dev)[:, ::2]))]
    for kw in bad:
        with pytest.raises(ValueError):
            env.peek(**kw)
    assert tuple(env.peek(ok)['ret'].shape) == (PC.E, 4)
    for kw in (dict(action_space='flying'), dict(action_space='walking', discretize=False), dict(size_reward=True)):
        other = VecGridWorld(4, **dict(dict(size_reward=False), **kw))
        with pytest.raises(ValueError):
            other.peek(ok)


def test_the_facade_and_the_helpers():
    import gridworld_amd as G
    env = _stepped('towers')
    cand = _dev(PC.candidates('random'), env)
    res = env.peek(cand)
    cell, colour = G.peek_decode(res['change'])
    change = res['change'].to(torch.int32)
    assert torch.equal(cell, torch.where(change < 0, change, change & 0x7ff)) and torch.equal(colour, torch.where(change < 0, change, change >> 11))
    best = G.peek_best(res['ret'])
    ret = res['ret'].cpu().numpy()
    assert np.array_equal(best.cpu().numpy(), ret.argmax(1))
    one = G.make('IGLUGridworldVector-v0', size_reward=False)
    one.set_task(G.dummy_task())
    one.reset()
    got = one.unwrapped.peek(PC.candidates('directed'))
    assert sorted(got) == sorted(KEYS) and all(isinstance(v, np.ndarray) for v in got.values())
    assert got['reward'].shape == (len(PC.DIRECTED_NAMES), 32) and got['pose'].shape == (len(PC.DIRECTED_NAMES), 5)


# ---- 6. whole wavefronts and a tail, auto-reset, against the oracle ----------------------------------------------------------
B = 2049


def test_a_stepped_autoreset_batch_equals_the_oracle():
    """2,049 auto-resetting rt20 envs at steps 0, 20 and 60 of a random rollout: the 18 one-step candidates against nine
    oracle blocks (a no-op and the eight actions that can change the grid: every other action is paid and ends as the
    no-op does and changes nothing; its pose is not compared) and eight random 8-step candidates per env against eight,
    all five outputs."""
    from gridworld_amd import VecGridWorld, workloads
    kw = dict(size_reward=False, max_steps=40)
    targets = workloads.rt20(B, seed=14).numpy().astype(np.int8)
    a = MC.stream(21, n=B)
    a = np.concatenate([a[:40], a[:20]])     # the look-down actions again after the time limit's reset
    case = dict(kw=kw, targets=targets, starts=None, poses=None, actions=a)
    env = VecGridWorld(B, autoreset=True, **kw)
    env.set_tasks(targets)
    env.reset()
    acts = torch.from_numpy(a).to(env.device)
    one = torch.arange(18, dtype=torch.int32, device=env.device).reshape(18, 1)
    rnd_np = PC.random_candidates(41, n=B, k=8, h=8)
    rnd = torch.from_numpy(rnd_np).to(env.device)
    probes = np.array([[0]] + [[p] for p in MC.PROBES], np.int32)
    got = {}
    for t in range(61):
        if t in (0, 20, 60):
            got[t] = (_np(env.peek(one, outputs=('reward', 'ends', 'change'))), _np(env.peek(rnd)))
        if t < 60:
            env.step(acts[t])
    bad = {}
    for tc in (0, 20, 60):
        nine = PC.truth_of(case, tc, probes, autoreset=True)
        want = {k: np.repeat(nine[k][:, :1], 18, 1) for k in ('reward', 'ends', 'change')}
        for j, p in enumerate(MC.PROBES):
            for k in want:
                want[k][:, p] = nine[k][:, j + 1]
        assert (want['change'][:, [0, 1, 2, 3, 4, 5, 12, 13, 14, 15]] == -1).all()
        eight = PC.truth_of(case, tc, rnd_np, autoreset=True)
        bad[tc] = (_mismatches(got[tc][0], want, ('reward', 'ends', 'change')),
                   _mismatches(got[tc][1], dict(eight, ret=eight['ret'][1.0])))
        print(f'step {tc}: {int((want["reward"] != 0).sum())} of {want["reward"].size} one-step rewards and '
              f'{int((eight["reward"] != 0).sum())} of {eight["reward"].size} 8-step rewards are not 0, '
              f'{int((eight["ends"] > 0).sum())} candidates end; elements that differ: {bad[tc]}')
    assert (eight['reward'] != 0).sum() >= 1000
    assert not any(v for pair in bad.values() for d in pair for v in d.values())
