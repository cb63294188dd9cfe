"""The worth query (igw_worth, VecGridWorld.worth, worth_decode) on the GPU.  One yardstick, exact
(0 mismatches): the numpy model of tests/worth_model.py on the CPU oracle's states, which tests/test_worth_cpu.py pins to
the oracle's own step and to its stateless Task evaluation.

Against the model: 8 cases x 6 checkpoints x 32 envs (every word, the pad words included, and `best` ungated, under a
random gate, under aim()'s gate and -- empty_inventory -- stocked), 257 auto-resetting envs at three points of a random
rollout, a flying and a walking Dict batch.  Against the goal query: the words at the cells the acting actions change."""
import numpy as np
import pytest
import torch

import mask_cases as MC
import worth_cases as WC
import worth_model as WM

pytestmark = pytest.mark.gpu

E = WC.E
ROW = 1104


def _gpu_env(case, n=E, **kw):
    from gridworld_amd import VecGridWorld
    env = VecGridWorld(n, **dict(case['kw'], **kw))
    pose = None if case['poses'] is None else case['poses'][:n]
    env.set_tasks(case['targets'][:n], None if case['starts'] is None else case['starts'][:n], init_pose=pose)
    return env


def _stepped(name, tc, n=E, **kw):
    case = WC.cases()[name]
    env = _gpu_env(case, n, **kw)
    env.reset()
    acts = torch.from_numpy(case['actions'][:, :n]).to(env.device)
    for t in range(tc):
        env.step(acts[t])
    return env


def _raw(word):
    """int16 [N, 7, 1104] numpy: the rows behind the [N, 7, 9, 11, 11] view, pad words included."""
    n = word.shape[0]
    return torch.as_strided(word, (n, 7, ROW), (7 * ROW, ROW, 1)).cpu().numpy()


def _allow_rows(a, dev):
    """uint8 numpy [N, 2, 1104] -> the device tensor worth() takes."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(dev)


# ---- 1. against the model, case by case ---------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(WC.cases()))
def test_words_and_best_equal_the_model(name):
    from gridworld_amd import worth as W
    case, st, words = WC.cases()[name], WC.states(name), WC.words(name)
    rs, ws = WC.RIGHT, WC.WRONG
    env = _gpu_env(case)
    env.reset()
    acts = torch.from_numpy(case['actions']).to(env.device)
    rng = np.random.RandomState(7)
    t, bad, seen = 0, dict(word=0, best=0, gated=0, aimed=0, stocked=0), dict(best=set(), aimed=0, none=0)
    for c, tc in enumerate(WC.CHECKPOINTS):
        while t < tc:
            env.step(acts[t])
            t += 1
        res = env.worth()
        assert list(res) == ['word', 'best']
        assert res['word'].dtype == torch.int16 and tuple(res['word'].shape) == (E, 7, 9, 11, 11)
        assert res['word'].stride() == (7 * ROW, ROW, 121, 11, 1)
        assert res['best'].dtype == torch.int32 and tuple(res['best'].shape) == (E, 4)
        got = _raw(res['word'])
        bad['word'] += int((got != words[c]).sum())
        best = res['best'].cpu().numpy()
        bad['best'] += int((best != np.stack([WM.best_of(words[c, i], rs, ws) for i in range(E)])).sum())
        seen['best'] |= set(best[:, 0].tolist())
        # a random gate (a quarter of the cells open), an all-closed one for env 0
        gate = (rng.uniform(size=(E, 2, ROW)) < 0.25).astype(np.uint8)
        gate[0] = 0
        g = env.worth(outputs=('best',), allow=_allow_rows(gate, env.device))
        assert list(g) == ['best']
        g = g['best'].cpu().numpy()
        bad['gated'] += int((g != np.stack([WM.best_of(words[c, i], rs, ws, gate[i]) for i in range(E)])).sum())
        assert g[0].tolist() == [-1, -1, -1, 0]
        # aim()'s two planes as the gate: the best-paid edit the agent can reach by turning
        aim = env.aim()
        allow = W.allow_from_aim(aim)
        a = env.worth(outputs='best', allow=allow)['best'].cpu().numpy()
        an = torch.as_strided(allow, (E, 2, ROW), (2 * ROW, ROW, 1)).cpu().numpy()
        assert np.array_equal(an[:, 0, :1089].reshape(E, 9, 11, 11), aim['break'].cpu().numpy() >= 0)
        assert np.array_equal(an[:, 1, :1089].reshape(E, 9, 11, 11), aim['place'].cpu().numpy() >= 0)
        bad['aimed'] += int((a != np.stack([WM.best_of(words[c, i], rs, ws, an[i]) for i in range(E)])).sum())
        seen['aimed'] += int((a[:, 3] > 0).sum())
        seen['none'] += int((a[:, 3] == 0).sum())
        if name == 'empty_inventory':
            s = env.worth(outputs=('best',), stocked=True)['best'].cpu().numpy()
            inv = st['inventory'][c]
            assert np.array_equal(env.inventory.cpu().numpy().astype(np.int32), inv) and (inv <= 0).any(1).all()
            bad['stocked'] += int((s != np.stack([WM.best_of(words[c, i], rs, ws, None, inv[i]) for i in range(E)])).sum())
            assert (s[:, 3] < best[:, 3]).all()
    print(f'{name}: elements that differ from the model: {bad}; best planes seen {sorted(seen["best"])}; aim-gated '
          f'answers with / without a candidate: {seen["aimed"]} / {seen["none"]}')
    assert not any(bad.values())
    assert seen['aimed'] >= E   # the agent reaches something in at least one checkpoint's worth of env-checkpoints


# ---- 2. against the goal query --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['looking_down', 'towers', 'recolour', 'unbuild'])
def test_the_words_at_the_cells_the_actions_change_decode_to_the_goal_querys_gain(name):
    import gridworld_amd as G
    case = WC.cases()[name]
    env = _gpu_env(case)
    env.reset()
    acts = torch.from_numpy(case['actions']).to(env.device)
    t = n = 0
    for tc in (12, 25, 40):
        while t < tc:
            env.step(acts[t])
            t += 1
        goal = {k: v.cpu().numpy() for k, v in env.goal(gain=True).items()}
        mask, look = (x.cpu().numpy() for x in env.action_mask(look=True))
        d = G.worth_decode(_raw(env.worth(outputs=('word',))['word']), WC.RIGHT, WC.WRONG)
        active = env.internals()[:, 7].astype(np.int64)
        for i in range(E):
            for a in (6, 7, 8, 9, 10, 11, 16, 17):
                cell = int(look[i, 0] if a == 16 else look[i, 1])
                if not mask[i, a] or cell < 0:
                    continue
                plane = 0 if a == 16 else int(active[i]) if a == 17 else a - 5
                assert d['valid'][i, plane, cell], (tc, i, a)
                assert d['gain'][i, plane, cell:cell + 1].view(np.uint32)[0] == goal['gain'][i, a:a + 1].view(np.uint32)[0], (tc, i, a)
                assert bool(d['ends'][i, plane, cell]) == bool(goal['ends'][i, a]), (tc, i, a)
                n += 1
    print(f'{name}: {n} acting actions compared')
    assert n >= 100


# ---- 3. the query moves nothing ------------------------------------------------------------------------------------------
def test_the_state_is_untouched_and_the_next_step_is_that_of_an_env_that_never_asked():
    case = WC.cases()['towers']
    env, other = _stepped('towers', 25), _stepped('towers', 25)
    before, stats = env.state_dict(), env.stats_tensor().clone()
    env.worth()
    env.worth(outputs=('best',), stocked=True)
    torch.cuda.synchronize()
    after = env.state_dict()
    assert set(after) == set(before)
    for k, v in before.items():
        assert torch.equal(v, after[k]) if torch.is_tensor(v) else v == after[k], k
    assert torch.equal(stats, env.stats_tensor())
    a = torch.from_numpy(case['actions'][25]).to(env.device)
    o1, r1, d1, _ = env.step(a)
    o2, r2, d2, _ = other.step(a)
    assert torch.equal(r1.view(torch.int32), r2.view(torch.int32)) and torch.equal(d1, d2)
    for k in o2:
        assert torch.equal(o1[k].contiguous().view(torch.uint8), o2[k].contiguous().view(torch.uint8)), k
    s1, s2 = env.state_dict(), other.state_dict()
    for k, v in s1.items():
        assert torch.equal(v, s2[k]) if torch.is_tensor(v) else v == s2[k], k


# ---- 4. whole wavefronts and a tail, auto-reset -----------------------------------------------------------------------------
def _oracle_words(ob, targets, starts, max_steps):
    words, inv = [], []
    for i in range(len(targets)):
        st = ob.envs[i].task_state()
        words.append(WM.env_worth(targets[i], starts[i], ob.grid[i].reshape(9, 11, 11), st['syn_max_int'], st['step_no'],
                                  max_steps)['word'])
    return np.stack(words)


def _compare(env, words, rs=WC.RIGHT, ws=WC.WRONG):
    res = env.worth()
    best = np.stack([WM.best_of(w, rs, ws) for w in words])
    return int((_raw(res['word']) != words).sum()), int((res['best'].cpu().numpy() != best).sum())


def test_a_stepped_autoreset_batch_equals_the_model_on_the_oracles_states():
    """257 envs: 64 blocks of four wavefronts and one more env.  max_steps = 21, so that step 20 is the step before the
    time limit (every word ends) and the envs are in their third episode at step 60."""
    from gridworld_amd import VecGridWorld, workloads
    from oracle import oracle as O
    B, kw = 257, dict(size_reward=False, max_steps=21)
    targets = workloads.rt20(B, seed=14).numpy().astype(np.int8)
    starts = np.zeros_like(targets)
    env = VecGridWorld(B, autoreset=True, **kw)
    env.set_tasks(targets)
    env.reset()
    ob = O.OracleBatch(B, **kw)
    ob.set_tasks(targets)
    ob.reset()
    a = MC.stream(21, n=B)
    a = np.concatenate([a[:21], a[:21], a[:21]])
    acts = torch.from_numpy(a).to(env.device)
    bad = {}
    for t in range(61):
        if t in (0, 20, 60):
            words = _oracle_words(ob, targets, starts, 21)
            bad[t] = _compare(env, words)
            right, _, ends, valid = WM.decode(words[:, :, :1089])
            print(f'step {t}: {int((right > 0).sum())} words with right > 0, {int((right < 0).sum())} with right < 0, '
                  f'{int(ends.sum())} of {int(valid.sum())} end; elements that differ (word, best): {bad[t]}')
            if t == 20:
                assert ends[valid].all()
            if t == 60:
                assert (right < 0).sum() >= 20 and not ends[valid].all()
        if t < 60:
            env.step(acts[t])
            ob.step_walking(a[t], autoreset=True, nthreads=8)
    assert np.array_equal(env.grid.cpu().numpy().reshape(B, -1), ob.grid)
    assert not any(v for pair in bad.values() for v in pair)


# ---- 5. the other action spaces --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('space', ['flying', 'walking_dict'])
def test_the_other_action_spaces_answer(space):
    from gridworld_amd import VecGridWorld, workloads
    from oracle import oracle as O
    n = 32
    kw = dict(size_reward=False, max_steps=40, **(dict(action_space='flying') if space == 'flying' else dict(discretize=False)))
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
            cam = rng.uniform(-5, 5, (n, 2)).astype(np.float32)
            cam[:, 1] = np.where(t < 8, -5.0, cam[:, 1])   # (look down first: something to build on)
            if space == 'flying':
                mv = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
                inv, plc = rng.randint(0, 7, n).astype(np.int32), rng.choice([0, 1, 1, 2], n).astype(np.int32)
                env.step(dict(movement=mv, camera=cam, inventory=inv, placement=plc))
                ob.step_flying(mv, cam, inv, plc, autoreset=True)
            else:
                b = (rng.rand(n, 8) < 0.3).astype(np.uint8)
                b[:, 7] = rng.randint(0, 7, size=n) * (rng.rand(n) < 0.3)
                env.step(dict(buttons=b, camera=cam))
                ob.step_walking_dict(b, cam, autoreset=True)
    finally:
        O.use_device_trig(False)
    assert np.array_equal(env.grid.cpu().numpy().reshape(n, -1), ob.grid)
    built = int((ob.grid != 0).any(1).sum())
    bad = _compare(env, _oracle_words(ob, targets, np.zeros_like(targets), 40))
    print(f'{space}: {built} envs have built; elements that differ (word, best): {bad}')
    assert built >= 8 and bad == (0, 0)


# ---- 6. sub-batches, out=, single outputs, n = 1, the facade, the errors -----------------------------------------------
def test_sub_batches_answer_for_their_own_rows_on_their_own_stream():
    env = _stepped('towers', 12)
    whole = env.worth()
    h = E // 2
    for k, s in enumerate(env.split(2)):
        part = s.worth()
        s.synchronize()
        for key in whole:
            assert torch.equal(part[key].contiguous(), whole[key][k * h:(k + 1) * h].contiguous()), key


def test_out_writes_in_place_past_canary_rows_and_allocates_nothing():
    from gridworld_amd import worth as W
    env = _stepped('appendix_b', 25)
    first = env.worth()
    dev = env.device
    word_base = torch.full((E + 2, 7 * ROW), 0x5555, dtype=torch.int16, device=dev)
    best_base = torch.full((E + 2, 4), 0x55555555, dtype=torch.int32, device=dev)
    out = dict(word=torch.as_strided(word_base, (E, 7, 9, 11, 11), (7 * ROW, ROW, 121, 11, 1)), best=best_base[:E])
    allow = W.allow_from_aim(env.aim())
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated(dev)
    again = env.worth(out=out)
    gated = env.worth(outputs=('best',), allow=allow, stocked=True, out={'best': best_base[:E]})
    assert torch.cuda.memory_allocated(dev) == held
    assert again['word'] is out['word'] and again['best'] is out['best'] and gated['best'].data_ptr() == best_base.data_ptr()
    torch.cuda.synchronize()
    assert torch.equal(_t(again['word']), _t(first['word']))
    assert bool((word_base[E:] == 0x5555).all()) and bool((best_base[E:] == 0x55555555).all())   # nothing past row n
    raw = torch.as_strided(out['word'], (E, 7, ROW), (7 * ROW, ROW, 1))
    assert bool((raw[:, :, 1089:] == -1).all())
    env.worth(out=out)
    assert torch.equal(out['best'], first['best'])
    some = env.worth(out={'best': out['best']})      # the rest is allocated
    assert some['best'] is out['best'] and some['word'] is not out['word']
    # captured: every output given, nothing allocated
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.worth(out=out)
    out['best'].fill_(7)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out['best'], first['best'])


def _t(word):
    return torch.as_strided(word, (word.shape[0], 7, ROW), (7 * ROW, ROW, 1))


def test_a_single_output_and_a_single_env_work():
    env = _stepped('recolour', 25)
    both = env.worth()
    word, best = env.worth(outputs=('word',)), env.worth(outputs='best')
    assert list(word) == ['word'] and list(best) == ['best']
    assert torch.equal(_t(word['word']), _t(both['word'])) and torch.equal(best['best'], both['best'])
    one = _stepped('recolour', 25, n=1)
    res = one.worth()
    assert tuple(res['word'].shape) == (1, 7, 9, 11, 11) and tuple(res['best'].shape) == (1, 4)
    assert np.array_equal(_raw(res['word'])[0], WC.words('recolour')[4, 0])
    assert torch.equal(res['best'], both['best'][:1])


def test_the_facade_answers_for_its_one_env():
    import gridworld_amd as G
    case, col = WC.cases()['unbuild'], 0
    env = G.make('IGLUGridworldVector-v0', size_reward=False)
    start = [(x - 5, y - 1, z - 5, int(case['starts'][col, y, x, z])) for y, x, z in zip(*np.nonzero(case['starts'][col]))]
    env.set_task(G.Task('', case['targets'][col].astype(np.int32), starting_grid=start))
    env.reset()
    words = WC.words('unbuild')
    for t in range(26):
        if t in WC.CHECKPOINTS:
            c = WC.CHECKPOINTS.index(t)
            got = env.unwrapped.worth()
            assert list(got) == ['word', 'best'] and all(isinstance(v, np.ndarray) for v in got.values())
            assert got['word'].shape == (7, 9, 11, 11) and got['word'].dtype == np.int16 and got['best'].shape == (4,)
            assert np.array_equal(got['word'].reshape(7, -1), words[c, col, :, :1089])
            assert np.array_equal(got['best'], WM.best_of(words[c, col], WC.RIGHT, WC.WRONG))
            gate = np.zeros((2, 9, 11, 11), bool)
            gate[1, 0, 5, 4] = gate[0, 0, 5, 3] = True
            want = WM.best_of(words[c, col], WC.RIGHT, WC.WRONG, np.pad(gate.reshape(2, -1), ((0, 0), (0, 15))))
            assert np.array_equal(env.unwrapped.worth(allow=gate)['best'], want)
        env.step(int(case['actions'][t, col]))
    # at step 25 the extra block is gone: of "put colour 1 back" and "break the other extra block" the break pays
    assert want.tolist()[:2] == [0, 5 * 11 + 3] and G.worth_decode(want[2:3])['gain'][0] == 1.0
    with pytest.raises(ValueError):
        env.unwrapped.worth(allow=np.zeros((2, 1089), bool))


def test_the_value_errors_are_raised():
    env = _stepped('looking_down', 1, n=4)
    dev = env.device
    ok = env.worth()
    for outputs in ((), ('gain',), ('word', 'reward'), 'words'):
        with pytest.raises(ValueError):
            env.worth(outputs=outputs)
    with pytest.raises(ValueError):
        env.worth(out={'word': torch.zeros((4, 7, 9, 11, 11), dtype=torch.int16, device=dev)})   # not the rows' stride
    with pytest.raises(ValueError):
        env.worth(out={'best': torch.zeros((4, 4), dtype=torch.int64, device=dev)})
    with pytest.raises(ValueError):
        env.worth(out={'best': torch.zeros((3, 4), dtype=torch.int32, device=dev)})
    with pytest.raises(ValueError):
        env.worth(outputs=('best',), out={'word': ok['word']})
    with pytest.raises(ValueError):
        env.worth(out={'best': ok['best'].cpu()})
    for allow in (torch.zeros((4, 2, 9, 11, 11), dtype=torch.uint8, device=dev),       # not 1104-byte rows
                  torch.zeros((4, 2, ROW), dtype=torch.int8, device=dev),
                  torch.zeros((3, 2, ROW), dtype=torch.uint8, device=dev),
                  torch.zeros((4, 2, ROW), dtype=torch.uint8), np.zeros((4, 2, ROW), np.uint8)):
        with pytest.raises(ValueError):
            env.worth(allow=allow)
    assert list(env.worth(allow=torch.ones((4, 2, ROW), dtype=torch.uint8, device=dev))) == ['word', 'best']
