"""The peek query of the flying and walking Dict spaces (igw_peek_flying, igw_peek_walking_dict, VecGridWorld.peek_dict;
DESIGN.md section 15) on the GPU.  Every word of every output is compared, reward, pose and ret as bit patterns.
Yardsticks: the CPU oracle in device-trig mode (tests/peek_dict_cases.py), the step path itself (a second batch of
E * K rows, loaded with copies of the live state and stepped H times), and the state's own tensors before and after."""
import numpy as np
import pytest
import torch

import mask_cases as MC
import peek_dict_cases as DC

pytestmark = pytest.mark.gpu

KEYS = ('reward', 'ends', 'change', 'pose', 'ret')
DTYPES = dict(reward=torch.float32, ends=torch.int16, change=torch.int16, pose=torch.float32, ret=torch.float32)
ROW_KEYS = ('grid_buf', 'occ_buf', 'hist_buf', 'agent_buf', 'aux_buf', 'out_buf')


def _gpu_env(case, n=None, **kw):
    from gridworld_amd import VecGridWorld
    reps = 1 if n is None else n // len(case['targets'])
    tile = lambda a: None if a is None else np.concatenate([a] * reps)  # noqa: E731
    env = VecGridWorld(reps * len(case['targets']), **dict(case['kw'], **kw))
    env.set_tasks(tile(case['targets']), tile(case['starts']), init_pose=tile(case['poses']))
    return env


def _dev(actions, env):
    return {k: torch.from_numpy(np.array(v)).to(env.device) for k, v in actions.items()}


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


def _stepped(space, name='looking_down', steps=14, **kw):
    case = DC.cases(space)[name]
    env = _gpu_env(case, **kw)
    env.reset()
    prefix = _dev(DC.from_discrete(space, case['actions'][:steps]), env)
    for t in range(steps):
        env.step({k: v[t] for k, v in prefix.items()})
    return env


# ---- 1. against the oracle, case by case ------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(DC.PC.cases()))
@pytest.mark.parametrize('space', DC.SPACES)
def test_all_five_outputs_equal_the_oracle_truth(space, name):
    """Every case, checkpoint and candidate set, both gammas: `random` per env, `shared` and `directed` shared by the
    envs -- and, at the last checkpoint, `directed` once more expanded to the per-env layout and through two
    SubBatches."""
    total = dict.fromkeys(KEYS, 0)
    case, n = DC.cases(space)[name], DC.E
    env = _gpu_env(case)
    env.reset()
    prefix = _dev(DC.from_discrete(space, case['actions'][:max(DC.CHECKPOINTS)]), env)
    t = 0
    for tc in DC.CHECKPOINTS:
        while t < tc:
            env.step({k: v[t] for k, v in prefix.items()})
            t += 1
        for cset in DC.SETS:
            cand = _dev(DC.candidates(space, cset), env)
            first = cand[DC.FIELDS[space][0][0]]
            K, H = first.shape[1:3] if cset == 'random' else first.shape[:2]
            truth = DC.truth(space, name, tc, cset)
            for gamma in DC.GAMMAS:
                res = env.peek_dict(cand, gamma=gamma)
                assert list(res) == list(KEYS)
                for k, shape in dict(reward=(n, K, H), ends=(n, K), change=(n, K, H), pose=(n, K, 5), ret=(n, K)).items():
                    assert res[k].dtype == DTYPES[k] and tuple(res[k].shape) == shape and res[k].is_contiguous(), k
                bad = _mismatches(_np(res), dict(truth, ret=truth['ret'][gamma]))
                if any(bad.values()):
                    print(f'{space} {name} {cset} checkpoint {tc} gamma {gamma}: {bad}')
                for k, v in bad.items():
                    total[k] += v
    # the other layout and the SubBatch path, against the same truth
    cand = _dev(DC.candidates(space, 'directed'), env)
    truth = DC.truth(space, name, max(DC.CHECKPOINTS), 'directed')
    want = dict(truth, ret=truth['ret'][1.0])
    per_env = {k: v.unsqueeze(0).expand(n, *v.shape).contiguous() for k, v in cand.items()}
    for k, v in _mismatches(_np(env.peek_dict(per_env)), want).items():
        total[k] += v
    torch.cuda.synchronize()
    lo = 0
    for sub in env.split(2):
        m = sub.num_envs
        part = sub.peek_dict({k: v[lo:lo + m].contiguous() for k, v in per_env.items()})
        sub.synchronize()
        for k, v in _mismatches(_np(part), {k: v[lo:lo + m] for k, v in want.items()}).items():
            total[k] += v
        shared = sub.peek_dict(cand, outputs=('ret',))
        sub.synchronize()
        total['ret'] += int((_bits(shared['ret'].cpu().numpy()) != _bits(want['ret'][lo:lo + m])).sum())
        lo += m
    assert lo == n
    print(f'{space} {name}: elements that differ from the oracle: {total}')
    assert not any(total.values())


# ---- 2. against the step path --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('space,name', [('flying', 'towers'), ('walking_dict', 'looking_down')])
def test_peek_dict_equals_the_step_path_on_replicated_rows(space, name):
    """The `random` set (32 envs x 70 candidates x 16 steps) against a second batch of 32 * 70 rows whose state rows are
    copies of the live ones (row k * 32 + i = copy k of env i, through state_dict / load_state_dict), stepped 16 times
    through env.step() without auto-reset."""
    E, T0 = DC.E, 12
    case = DC.cases(space)[name]
    cand_np = DC.candidates(space, 'random')
    K, H = cand_np['camera'].shape[1:3]
    env = _stepped(space, name, T0, autoreset=False)
    big = _gpu_env(case, n=E * K, autoreset=False)
    big.reset()
    torch.cuda.synchronize()
    live, state = env.state_dict(), big.state_dict()
    for key in ROW_KEYS:
        state[key] = live[key].repeat(K, *([1] * (live[key].dim() - 1)))
    big.load_state_dict(state)
    cand = _dev(cand_np, env)
    got = _np(env.peek_dict(cand))
    rows = E * K
    reward, change = np.zeros((rows, H), np.float32), np.full((rows, H), -1, np.int16)
    ends, pose = np.zeros(rows, np.int16), np.zeros((rows, 5), np.float32)
    alive, ar = np.ones(rows, bool), np.arange(rows)
    before = big.grid.reshape(rows, -1).cpu().numpy()
    for h in range(H):
        big.step({k: v[:, :, h].transpose(0, 1).reshape((rows,) + tuple(v.shape[3:])).contiguous() for k, v in cand.items()})
        grid = big.grid.reshape(rows, -1).cpu().numpy()
        diff = grid != before
        assert (diff.sum(1) <= 1).all()
        cell = diff.argmax(1)
        code = np.where(diff.any(1), (grid[ar, cell].astype(np.int32) << 11) | cell, -1)
        reward[alive, h], change[alive, h] = big.reward.cpu().numpy()[alive], code[alive]
        pose[alive] = big.agent_pos.cpu().numpy()[alive]
        ended = alive & (big.done.cpu().numpy() != 0)
        ends[ended] = h + 1
        alive &= ~ended
        before = grid
    by_env = lambda x: np.ascontiguousarray(np.swapaxes(x.reshape((K, E) + x.shape[1:]), 0, 1))  # noqa: E731
    want = dict(reward=by_env(reward), ends=by_env(ends), change=by_env(change), pose=by_env(pose))
    bad = _mismatches(got, want, ('reward', 'ends', 'change', 'pose'))
    print(f'{space}: {int((want["change"] >= 0).sum())} changes, {int((want["reward"] != 0).sum())} rewards that are not 0, '
          f'{int((want["ends"] > 0).sum())} candidates end; elements that differ from the step path: {bad}')
    assert (want['change'] >= 0).sum() >= 1000 and (want['reward'] != 0).sum() >= 1000
    assert not any(bad.values())


# ---- 3. the state is untouched ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('space', DC.SPACES)
def test_peek_dict_leaves_the_state_the_counters_and_the_log_as_they_were(space):
    env = _stepped(space, 'towers', 10)
    rec, heads = env.enable_trajectory_log(n_envs=4)
    prefix = _dev(DC.from_discrete(space, DC.cases(space)['towers']['actions'][10:14]), env)
    for t in range(4):
        env.step({k: v[t] for k, v in prefix.items()})
    torch.cuda.synchronize()
    state = {k: v.clone() for k, v in env.state_dict().items() if torch.is_tensor(v)}
    stats, log = env.stats_tensor().clone(), (rec.clone(), heads.clone())
    assert len(state) >= 5 and int(heads.abs().sum()) > 0
    for cset in DC.SETS:   # (`directed` holds every kind of invalid action: nothing is counted)
        env.peek_dict(_dev(DC.candidates(space, cset), env), gamma=0.5)
    torch.cuda.synchronize()
    after = env.state_dict()
    for k, v in state.items():
        assert torch.equal(v.contiguous().view(torch.uint8), after[k].contiguous().view(torch.uint8)), k
    assert torch.equal(stats, env.stats_tensor())
    assert torch.equal(log[0], rec) and torch.equal(log[1], heads)


# ---- 4. output selection, out=, capture --------------------------------------------------------------------------------------
@pytest.mark.parametrize('space', DC.SPACES)
def test_a_subset_of_outputs_and_out_in_place_with_guard_rows(space):
    env = _stepped(space)
    dev = env.device
    cand = _dev(DC.candidates(space, 'random'), env)
    n, K, H = cand['camera'].shape[:3]
    whole = env.peek_dict(cand, gamma=0.97)
    some = env.peek_dict(cand, gamma=0.97, outputs=('ret', 'ends'))
    assert list(some) == ['ends', 'ret']
    _same(some, {k: whole[k] for k in ('ends', 'ret')})
    # out=: rows [0, n) of longer buffers, guard rows behind them; an output that is not asked for is not written
    sizes = dict(reward=K * H, ends=K, change=K * H, pose=K * 5, ret=K)
    shapes = dict(reward=(n, K, H), ends=(n, K), change=(n, K, H), pose=(n, K, 5), ret=(n, K))
    bufs = {k: torch.full((n + 2, sizes[k]), 0x55, dtype=torch.uint8, device=dev).repeat(1, DTYPES[k].itemsize).view(DTYPES[k])
            for k in KEYS}
    out = {k: bufs[k][:n].view(shapes[k]) for k in KEYS}
    fresh = {k: v.clone() for k, v in bufs.items()}
    res = env.peek_dict(cand, gamma=0.97, outputs=('pose', 'change'), out={k: out[k] for k in ('pose', 'change')})
    assert list(res) == ['change', 'pose'] and all(res[k] is out[k] for k in res)
    _same(res, {k: whole[k] for k in ('change', 'pose')})
    for k in ('reward', 'ends', 'ret'):
        assert torch.equal(bufs[k].view(torch.uint8), fresh[k].view(torch.uint8)), k
    res = env.peek_dict(cand, gamma=0.97, out=out)
    for k in KEYS:
        assert res[k] is out[k]
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated(dev)
    res = env.peek_dict(cand, gamma=0.97, out=out)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(dev) == held
    _same(res, whole)
    for k in KEYS:
        assert torch.equal(bufs[k][n:].view(torch.uint8), fresh[k][n:].view(torch.uint8)), k


@pytest.mark.parametrize('space', DC.SPACES)
def test_a_captured_call_replayed_after_a_step_equals_a_fresh_call(space):
    """With every output passed in `out` and the actions device tensors of the ABI dtypes, a captured call allocates
    nothing and records one kernel launch on the capturing stream and nothing on any other: asserted as no change of
    the allocator's counters over the captured calls and, on replay, as the answers of fresh calls.  Two calls captured one
    after the other are therefore two nodes of a single chain."""
    env = _stepped(space, 'towers', 12)
    cand = _dev(DC.candidates(space, 'random'), env)
    out = {k: torch.empty_like(v) for k, v in env.peek_dict(cand, gamma=0.97).items()}
    ends2 = {k: torch.empty_like(out[k]) for k in ('ends', 'ret')}
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        before = torch.cuda.memory_stats(env.device)     # (inside: beginning a capture allocates the generator's state)
        res = env.peek_dict(cand, gamma=0.97, out=out)
        res2 = env.peek_dict(cand, outputs=('ends', 'ret'), out=ends2)
        after = torch.cuda.memory_stats(env.device)
    assert all(res[k] is out[k] for k in out) and all(res2[k] is ends2[k] for k in ends2)
    for key in ('allocation.all.allocated', 'allocated_bytes.all.allocated', 'segment.all.allocated'):
        assert after[key] == before[key], key                               # the two calls allocated nothing
    prefix = _dev(DC.from_discrete(space, DC.cases(space)['towers']['actions'][12:16]), env)
    for t in range(4):
        env.step({k: v[t] for k, v in prefix.items()})
    for v in list(out.values()) + list(ends2.values()):
        v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    _same(out, env.peek_dict(cand, gamma=0.97))
    _same(ends2, env.peek_dict(cand, outputs=('ends', 'ret')))
    assert int((out['change'] >= 0).sum()) > 100


# ---- 5. edges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [1, 65])
@pytest.mark.parametrize('H', [1, 32])
@pytest.mark.parametrize('space', DC.SPACES)
def test_chunk_and_step_boundaries(space, K, H):
    """K = 1 and K = 65 (a 64-chunk plus one candidate), H = 1 and H = 32: a candidate's answers depend neither on its
    neighbours nor on the steps that follow (H = 32 against the oracle: the `directed` sets and one_env_h32 below)."""
    env = _stepped(space, 'towers')
    full = _dev(DC.random_candidates(space, 5, k=70, h=32), env)
    whole = env.peek_dict(full)
    part = env.peek_dict({k: v[:, :K, :H].contiguous() for k, v in full.items()})
    ended = (whole['ends'][:, :K] > 0) & (whole['ends'][:, :K] <= H)
    assert torch.equal(part['reward'].view(torch.int32), whole['reward'][:, :K, :H].view(torch.int32))
    assert torch.equal(part['change'], whole['change'][:, :K, :H])
    assert torch.equal(part['ends'], torch.where(ended, whole['ends'][:, :K], torch.zeros_like(part['ends'])))
    if H == 32:
        assert torch.equal(part['pose'].view(torch.int32), whole['pose'][:, :K].view(torch.int32))
        assert torch.equal(part['ret'].view(torch.int32), whole['ret'][:, :K].view(torch.int32))


def test_discrete_actions_through_peek_and_through_the_walking_dict_entry_agree_bitwise():
    """One kernel body serves igw_peek and igw_peek_walking_dict: three envs of `towers` after 12 steps, K = 65 (a
    64-chunk plus one candidate) per-env sequences of H = 4 random Discrete(18) actions through env.peek, the same
    actions as buttons and camera through peek_dict of a walking Dict batch in the same state.  All five outputs, float32
    as bit patterns."""
    n, K, H, T0 = 3, 65, 4, 12
    acts = np.random.default_rng(2365).integers(0, 18, (n, K, H)).astype(np.int32)
    res = {}
    for space in ('discrete', 'walking_dict'):
        c = (DC.PC.cases() if space == 'discrete' else DC.cases(space))['towers']
        cut = lambda a: None if a is None else a[:n]  # noqa: E731
        env = _gpu_env(dict(c, targets=c['targets'][:n], starts=cut(c['starts']), poses=cut(c['poses'])))
        env.reset()
        for t in range(T0):
            a = c['actions'][t, :n]
            env.step(torch.from_numpy(np.array(a)).to(env.device) if space == 'discrete' else _dev(DC.from_discrete(space, a), env))
        res[space] = env.peek(torch.from_numpy(acts).to(env.device), gamma=0.97) if space == 'discrete' else \
            env.peek_dict(_dev(DC.from_discrete(space, acts), env), gamma=0.97)
        assert tuple(res[space]['reward'].shape) == (n, K, H)
    a, b = _np(res['discrete']), _np(res['walking_dict'])
    bad = _mismatches(a, b)
    print(f'{int((a["change"] >= 0).sum())} changes, {int((a["reward"] != 0).sum())} rewards that are not 0; elements that differ: {bad}')
    assert (a['change'] >= 0).sum() >= 20 and (a['reward'] != 0).sum() >= 20
    assert not any(bad.values())


def _edge(space, n, seed, steps, k, h, shared=False):
    """(env, candidates, truth) of n rt20 envs of the space after `steps` steps of a random stream."""
    from gridworld_amd import workloads
    case = dict(kw=dict(MC.KW, **DC.KW[space]), targets=workloads.rt20(n, seed=seed).numpy().astype(np.int8), starts=None,
                poses=None, actions=MC.stream(seed, n=n))
    cand = DC.random_candidates(space, seed + 1, n=n, k=k, h=h)
    if shared:
        cand = {key: v[0] for key, v in cand.items()}
    env = _gpu_env(case)
    env.reset()
    prefix = _dev(DC.from_discrete(space, case['actions'][:steps]), env)
    for t in range(steps):
        env.step({key: v[t] for key, v in prefix.items()})
    return env, cand, DC.truth_of(space, case, steps, cand)


@pytest.mark.parametrize('space', DC.SPACES)
@pytest.mark.parametrize('n,k,h,shared', [(1, 70, 32, False), (67, 5, 32, False), (2, 4096, 2, True), (2, 4096, 2, False)],
                         ids=['one_env_h32', '67_envs', 'k4096_shared', 'k4096_per_env'])
def test_odd_batches_and_the_largest_k_equal_the_oracle(space, n, k, h, shared):
    """N = 1 with H = 32 and K = 70, N = 67, and K = 4096 at two envs with H = 2 in both layouts, against the oracle;
    guard rows behind row n - 1 of every output keep their sentinel."""
    env, cand, truth = _edge(space, n, 40 + n, 12, k, h, shared)
    sizes = dict(reward=k * h, ends=k, change=k * h, pose=k * 5, ret=k)
    shapes = dict(reward=(n, k, h), ends=(n, k), change=(n, k, h), pose=(n, k, 5), ret=(n, k))
    bufs = {key: torch.full((n + 2, sizes[key]), 0x5a, dtype=torch.uint8, device=env.device).repeat(1, DTYPES[key].itemsize).view(DTYPES[key])
            for key in KEYS}
    res = env.peek_dict(_dev(cand, env), out={key: bufs[key][:n].view(shapes[key]) for key in KEYS})
    bad = _mismatches(_np(res), dict(truth, ret=truth['ret'][1.0]))
    print(f'{space} n = {n}, K = {k}, H = {h}: {int((truth["change"] >= 0).sum())} changes; elements that differ: {bad}')
    assert (truth['change'] >= 0).sum() >= 20
    assert not any(bad.values())
    for key in KEYS:
        assert (bufs[key][n:].view(torch.uint8) == 0x5a).all(), key


# ---- 6. errors and the existing behaviour ------------------------------------------------------------------------------------
@pytest.mark.parametrize('space', DC.SPACES)
def test_errors(space):
    from gridworld_amd import VecGridWorld
    env = _stepped(space, steps=0)
    dev = env.device
    zeros = lambda lead: {k: torch.zeros(tuple(lead) + shape, dtype=getattr(torch, np.dtype(dt).name), device=dev)  # noqa: E731
                          for k, dt, shape in DC.FIELDS[space]}
    ok = zeros((4, 3))
    other = 'walking_dict' if space == 'flying' else 'flying'
    bad = [dict(actions={k: v for k, v in ok.items() if k != 'camera'}), dict(actions=dict(ok, more=ok['camera'])),
           dict(actions=_dev(DC.candidates(other, 'shared'), env)), dict(actions=ok['camera']),
           dict(actions=dict(ok, camera=ok['camera'][:3])), dict(actions=dict(ok, camera=ok['camera'][:, :2])),
           dict(actions=zeros((DC.E + 1, 4, 3))), dict(actions=zeros((4, 33))), dict(actions=zeros((4097, 1))),
           dict(actions=zeros((0, 3))), dict(actions=zeros((4, 0))), dict(actions=zeros((3,))),
           dict(actions=ok, outputs=()), dict(actions=ok, outputs=('ret', 'gain')),
           dict(actions=ok, out=dict(gain=torch.zeros((DC.E, 4), device=dev))),
           dict(actions=ok, outputs=('ret',), out=dict(ends=torch.zeros((DC.E, 4), dtype=torch.int16, device=dev))),
           dict(actions=ok, out=dict(ret=torch.zeros((DC.E, 5), device=dev))),
           dict(actions=ok, out=dict(ret=torch.zeros((DC.E, 4), dtype=torch.float64, device=dev))),
           dict(actions=ok, out=dict(ret=torch.zeros((DC.E, 4)))),
           dict(actions=ok, out=dict(ret=torch.zeros((DC.E, 8), device=dev)[:, ::2]))]
    for kw in bad:
        with pytest.raises(ValueError):
            env.peek_dict(**kw)
    assert tuple(env.peek_dict(ok)['ret'].shape) == (DC.E, 4)
    # host arrays, lists and other dtypes are converted; the answer is the device tensors'
    cand = DC.candidates(space, 'directed')
    _same(env.peek_dict(cand), env.peek_dict(_dev(cand, env)))
    _same(env.peek_dict({k: v.astype(np.float64) if v.dtype == np.float32 else v.astype(np.int64) for k, v in cand.items()}),
          env.peek_dict(_dev(cand, env)))
    # integer cameras and movements (whole degrees are a natural input) are the plain casts env.step() makes of them;
    # nested lists are accepted
    whole = {k: np.rint(v) if v.dtype == np.float32 else v for k, v in DC.candidates(space, 'random').items()}
    want = env.peek_dict(_dev(whole, env))
    assert int((want['change'] >= 0).sum()) > 1000
    _same(env.peek_dict({k: v.astype(np.int64) for k, v in whole.items()}), want)
    _same(env.peek_dict({k: torch.from_numpy(v.astype(np.int64)).to(dev) for k, v in whole.items()}), want)
    for few in ({k: v[:, :3, :4] for k, v in whole.items()}, {k: v[0, :3, :4] for k, v in whole.items()}):   # per env, shared
        _same(env.peek_dict({k: v.tolist() for k, v in few.items()}), env.peek_dict(_dev(few, env)))
    # env.peek still raises in these spaces, peek_dict in the Discrete(18) one and with size_reward=True
    with pytest.raises(ValueError, match='Discrete'):
        env.peek(torch.zeros((4, 3), dtype=torch.int32, device=dev))
    walking = VecGridWorld(4, size_reward=False)
    with pytest.raises(ValueError, match=r'env\.peek'):
        walking.peek_dict(ok)
    with pytest.raises(ValueError, match='size_reward'):
        VecGridWorld(4, **dict(DC.KW[space], size_reward=True)).peek_dict(ok)


def test_the_helpers_read_the_result():
    import gridworld_amd as G
    env = _stepped('flying', 'towers')
    res = env.peek_dict(_dev(DC.candidates('flying', 'random'), env))
    cell, colour = G.peek_decode(res['change'])
    change = res['change'].to(torch.int32)
    assert torch.equal(cell, torch.where(change < 0, change, change & 0x7ff)) and torch.equal(colour, torch.where(change < 0, change, change >> 11))
    assert np.array_equal(G.peek_best(res['ret']).cpu().numpy(), res['ret'].cpu().numpy().argmax(1))
