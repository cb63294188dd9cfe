"""The aim query (igw_aim, VecGridWorld.aim, aim_decode / aim_action) on the GPU.  Exact (0
mismatches) against the two yardsticks of tests/aim_cases.py: the model (every state of every case, four windows) and
the oracle probe directly (eight states on the lattice, eight off it); against the action mask where the two overlap;
and played through the public API: turn as aim_action says, place or break, and the grid changes in the cell named."""
import numpy as np
import pytest
import torch

import aim_cases as AC

pytestmark = pytest.mark.gpu

ROW, CELLS = AC.ROW, AC.CELLS
HERE = AC.code_of(0, 0)     # the direction the camera points in now


def _gpu_env(case, **kw):
    from gridworld_amd import VecGridWorld
    env = VecGridWorld(len(case['targets']), **dict(case['kw'], **kw))
    env.set_tasks(case['targets'], case['starts'], init_pose=case['poses'])
    return env


def _stepped(name, steps, **kw):
    case = AC.cases()[name]
    env = _gpu_env(case, **kw)
    env.reset()
    acts = torch.from_numpy(case['actions']).to(env.device)
    for t in range(steps):
        env.step(acts[t])
    return env


def _raw(plane):
    """The [N, 1104] rows a plane is a view of."""
    return torch.as_strided(plane, (plane.shape[0], ROW), (ROW, 1))


def _check_planes(res, n, env):
    for k in res:
        assert res[k].dtype == torch.int32 and tuple(res[k].shape) == (n, 9, 11, 11)
        assert res[k].stride() == (ROW, 121, 11, 1) and res[k].data_ptr() % 16 == 0
        assert env.grid.stride() == res[k].stride()      # a view of its rows, as `grid` is of its own


# ---- 1. kernel = model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(AC.cases()))
def test_both_planes_equal_the_model_on_every_state(name):
    case = AC.cases()[name]
    grids, _, inter = AC.states(name)
    E = grids.shape[1]
    env = _gpu_env(case)
    env.reset()
    acts = torch.from_numpy(case['actions']).to(env.device)
    t, bad, cells = 0, 0, 0
    for c, tc in enumerate(AC.CHECKPOINTS):
        while t < tc:
            env.step(acts[t])
            t += 1
        torch.cuda.synchronize()
        assert np.array_equal(env.grid.cpu().numpy(), grids[c])
        assert np.array_equal(env.internals().view(np.uint64), inter[c].view(np.uint64))
        for max_turns in (0, 1, 7, 72):
            res = env.aim(max_turns=max_turns)
            assert list(res) == ['place', 'break']
            _check_planes(res, E, env)
            place, brk = AC.truth(name, max_turns)
            got_p, got_b = _raw(res['place']).cpu().numpy(), _raw(res['break']).cpu().numpy()
            assert (got_p[:, CELLS:] == -1).all() and (got_b[:, CELLS:] == -1).all()
            bad += int((got_p != place[c]).sum()) + int((got_b != brk[c]).sum())
            cells += int((place[c] >= 0).sum()) + int((brk[c] >= 0).sum())
    print(f'{name}: {cells} reachable cells over {len(AC.CHECKPOINTS) * E} states and four windows, {bad} words differ')
    assert cells > 0 and bad == 0


# ---- 2. kernel = probe -----------------------------------------------------------------------------------------------------
def test_eight_states_equal_the_oracle_probe():
    bad = cells = 0
    for name, c, envs in (('towers', 2, (0, 5, 9, 17)), ('directed', 1, (0, 2, 3, 5))):
        grids, poses, _ = AC.states(name)
        env = _stepped(name, AC.CHECKPOINTS[c])
        res = env.aim(max_turns=5)
        got_p, got_b = _raw(res['place']).cpu().numpy()[:, :CELLS], _raw(res['break']).cpu().numpy()[:, :CELLS]
        for e in envs:
            place, brk = AC.probe(grids[c, e], poses[c, e], 5)
            bad += int((got_p[e] != place).sum()) + int((got_b[e] != brk).sum())
            cells += int((place >= 0).sum()) + int((brk >= 0).sum())
    print(f'eight states at five turns: {cells} reachable cells, {bad} differ from the probe')
    assert cells >= 8 and bad == 0


def test_off_the_lattice_equals_the_probe_with_the_device_trig():
    """Yaw and pitch that are no multiples of 5: the table misses, the general evaluation answers."""
    from gridworld_amd import VecGridWorld
    from oracle import oracle as O
    case = AC.cases()['towers']
    n = 8
    rng = np.random.RandomState(29)
    poses = np.stack([rng.uniform(-4, 4, n), np.zeros(n), rng.uniform(-4, 4, n),
                      np.array([12.3, -77.7, 181.05, 3.0, 359.9, -123.456, 44.0, 90.5]),
                      np.array([-7.75, -33.3, -61.2, -89.5, 12.5, -45.1, -20.25, 2.5])], 1)
    env = VecGridWorld(n, **case['kw'])
    env.set_tasks(case['targets'][:n], case['starts'][:n], init_pose=poses)
    env.reset()
    torch.cuda.synchronize()
    assert np.array_equal(env.internals()[:, :5], poses)
    res = env.aim(max_turns=4)
    got_p, got_b = _raw(res['place']).cpu().numpy()[:, :CELLS], _raw(res['break']).cpu().numpy()[:, :CELLS]
    bad = cells = 0
    O.use_device_trig(True)
    try:
        for e in range(n):
            place, brk = AC.probe(case['starts'][e], poses[e], 4)
            bad += int((got_p[e] != place).sum()) + int((got_b[e] != brk).sum())
            cells += int((place >= 0).sum()) + int((brk >= 0).sum())
    finally:
        O.use_device_trig(False)
    print(f'off the lattice: {cells} reachable cells, {bad} differ from the probe')
    assert cells >= 8 and bad == 0


# ---- 3. max_turns = 0 against the action mask ---------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['towers', 'looking_down', 'empty_inventory'])
def test_no_turn_names_the_cells_of_the_action_mask(name):
    env = _stepped(name, 25)
    _, look = env.action_mask(look=True)
    res = env.aim(max_turns=0)
    look = look.cpu().numpy().astype(np.int64)
    n = look.shape[0]
    planes = {k: _raw(v).cpu().numpy()[:, :CELLS] for k, v in res.items()}
    for k in planes:
        assert ((planes[k] == HERE) | (planes[k] == -1)).all() and ((planes[k] == HERE).sum(1) <= 1).all()
    cell = {k: np.where((p == HERE).any(1), (p == HERE).argmax(1), -1) for k, p in planes.items()}
    assert np.array_equal(cell['break'], look[:, 0])
    active = env.internals()[:, 7].astype(np.int64)
    stocked = env.inventory.cpu().numpy()[np.arange(n), active - 1] > 0
    assert np.array_equal(cell['place'][stocked], look[stocked, 1])
    assert (look[~stocked, 1] == -1).all()
    print(f'{name}: {int((cell["break"] >= 0).sum())} break cells, {int((cell["place"] >= 0).sum())} place cells, '
          f'{int((~stocked).sum())} envs without stock')
    assert (cell['break'] >= 0).sum() + (cell['place'] >= 0).sum() >= 8


# ---- 4. played ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,last', [('place', 17), ('break', 16)])
def test_turning_as_aim_action_says_touches_the_cell_named(kind, last):
    import gridworld_amd as G
    env = _stepped('towers', 25)
    n, dev = env.num_envs, env.device
    noop = torch.zeros(n, dtype=torch.int32, device=dev)
    env.step(noop)
    pos = env.internals()[:, :3].copy()
    env.step(noop)
    state = env.internals()
    still = (state[:, :3] == pos).all(1) & (state[:, 5] == 0.0)
    before = env.grid.clone()
    code = _raw(env.aim(max_turns=6)[kind])[:, :CELLS]
    # per env the reachable cell that takes the most turns
    cells = torch.where((code >= 0).any(1), code.argmax(1), torch.full((n,), -1, device=dev))
    active = state[:, 7].astype(np.int64)
    stocked = env.inventory.cpu().numpy()[np.arange(n), active - 1] > 0
    use = torch.from_numpy(still & (stocked if kind == 'place' else True)).to(dev)
    cells = torch.where(use, cells, torch.full_like(cells, -1))
    chosen = cells >= 0
    turns = G.aim_decode(code.gather(1, cells.clamp(min=0).unsqueeze(1)).squeeze(1))[0]
    print(f'{kind}: {int(chosen.sum())} envs at rest with a cell to aim at, '
          f'{int((turns[chosen] > 0).sum())} of them have to turn first (up to {int(turns[chosen].max())} turns)')
    assert int(chosen.sum()) >= 8 and int((turns[chosen] > 0).sum()) >= 4
    acted = torch.zeros(n, dtype=torch.bool, device=dev)
    for _ in range(8):
        a = G.aim_action(env.aim(max_turns=6)[kind], cells, kind=kind)
        a = torch.where(acted, torch.zeros_like(a), a)
        assert bool(((a == 0) | (a == last) | ((a >= 12) & (a <= 15))).all()) and bool((a[~chosen] == 0).all())
        env.step(a)
        acted |= a == last
    assert bool((acted == chosen).all())
    if kind == 'place':      # (a break may take away what the agent stands on)
        assert np.array_equal(env.internals()[:, :3][still], state[:, :3][still])
    diff = (env.grid != before).reshape(n, -1)
    assert bool((diff.sum(1) == chosen.long()).all())
    assert bool((diff.long().argmax(1)[chosen] == cells[chosen]).all())
    after = env.grid.reshape(n, -1).gather(1, cells.clamp(min=0).unsqueeze(1)).squeeze(1)[chosen]
    assert bool((after != 0).all() if kind == 'place' else (after == 0).all())


# ---- 5. batch sizes, out=, sub-batches, one plane ------------------------------------------------------------------------------
def test_odd_batch_sizes_equal_rows_of_the_full_batch_and_write_nothing_else():
    from gridworld_amd import aim as A
    env = _stepped('towers', 12)
    full = {k: _raw(v).clone() for k, v in env.aim(max_turns=9).items()}
    agent, _, occ = env._rows
    # 65 envs: the 32 rows twice and one more
    idx = torch.arange(65, device=env.device) % env.num_envs
    agent65, occ65 = agent[idx].contiguous(), occ[idx].contiguous()
    for n in (1, 3, 65):
        flat = {k: torch.full(((n + 2) * ROW,), 85, dtype=torch.int32, device=env.device) for k in ('place', 'break')}
        A.aim_into(agent65.data_ptr(), occ65.data_ptr(), n, 9, flat['place'][ROW:].data_ptr(),
                   flat['break'][ROW:].data_ptr(), env._stream())
        torch.cuda.synchronize()
        for k in flat:
            rows = flat[k].reshape(n + 2, ROW)
            assert bool((rows[0] == 85).all()) and bool((rows[-1] == 85).all()), (n, k)
            assert torch.equal(rows[1:-1], full[k][idx[:n]]), (n, k)


def test_out_writes_in_place_and_allocates_nothing():
    env = _stepped('appendix_b', 25)
    n = env.num_envs
    keys = ('agent_buf', 'occ_buf', 'grid_buf', 'aux_buf', 'out_buf', 'hist_buf')
    before = {k: getattr(env, k).clone() for k in keys}
    first = env.aim(max_turns=12)
    torch.cuda.synchronize()
    for k in keys:                                   # the query writes nothing but its outputs
        assert torch.equal(getattr(env, k), before[k]), k
    out = {k: torch.as_strided(torch.full((n, ROW), 85, dtype=torch.int32, device=env.device), (n, 9, 11, 11),
                               (ROW, 121, 11, 1)) for k in first}
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated(env.device)
    again = env.aim(max_turns=12, out=out)
    assert torch.cuda.memory_allocated(env.device) == held
    for k in first:
        assert again[k] is out[k] and torch.equal(_raw(again[k]), _raw(first[k])), k
        assert bool((_raw(out[k])[:, CELLS:] == -1).all())
    some = env.aim(max_turns=12, out={'break': out['break']})     # the rest is allocated
    assert some['break'] is out['break'] and some['place'] is not out['place']
    with pytest.raises(ValueError):
        env.aim(out={'place': torch.zeros((n, 9, 11, 11), dtype=torch.int32, device=env.device)})   # not the rows' stride
    with pytest.raises(ValueError):
        env.aim(out={'place': torch.zeros((n, ROW), dtype=torch.int32, device=env.device)})
    with pytest.raises(ValueError):
        env.aim(place=False, out={'place': out['place']})


def test_sub_batches_answer_for_their_own_rows_on_their_own_stream():
    env = _stepped('towers', 12)
    whole = env.aim(max_turns=10)
    torch.cuda.synchronize()
    subs = env.split(2)
    h = env.num_envs // 2
    for k, s in enumerate(subs):
        assert s.stream is not None
        part = s.aim(max_turns=10)
        s.synchronize()
        assert list(part) == ['place', 'break']
        for key in whole:
            assert tuple(part[key].shape) == (h, 9, 11, 11)
            assert torch.equal(_raw(part[key]), _raw(whole[key])[k * h:(k + 1) * h]), key
    assert not torch.equal(_raw(whole['place'])[:h], _raw(whole['place'])[h:])


def test_one_plane_off_leaves_the_other_alone():
    env = _stepped('towers', 12)
    held = env.aim(max_turns=10)
    keep = {k: _raw(v).clone() for k, v in held.items()}
    _raw(held['place']).fill_(85)
    res = env.aim(max_turns=10, brk=False, out={'place': held['place']})
    assert list(res) == ['place'] and res['place'] is held['place']
    assert torch.equal(_raw(held['place']), keep['place']) and torch.equal(_raw(held['break']), keep['break'])
    _raw(held['break']).fill_(85)
    res = env.aim(max_turns=10, place=False, out={'break': held['break']})
    assert list(res) == ['break']
    assert torch.equal(_raw(held['place']), keep['place']) and torch.equal(_raw(held['break']), keep['break'])
    fresh = env.aim(max_turns=10, place=False)
    assert list(fresh) == ['break'] and torch.equal(_raw(fresh['break']), keep['break'])


# ---- 6. errors ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kw', [dict(action_space='flying'), dict(discretize=False)])
def test_aim_raises_outside_discrete_18(kw):
    from gridworld_amd import VecGridWorld, workloads
    env = VecGridWorld(4, size_reward=False, **kw)
    env.set_tasks(workloads.rt20(4, seed=1).numpy())
    env.reset()
    with pytest.raises(ValueError):
        env.aim()


def test_aim_raises_for_a_window_it_does_not_have():
    from gridworld_amd import VecGridWorld, workloads
    env = VecGridWorld(4, size_reward=False)
    env.set_tasks(workloads.rt20(4, seed=1).numpy())
    env.reset()
    for bad in (-1, 73):
        with pytest.raises(ValueError):
            env.aim(max_turns=bad)
    with pytest.raises(ValueError):
        env.aim(place=False, brk=False)
    assert list(env.aim(max_turns=0)) == ['place', 'break']
