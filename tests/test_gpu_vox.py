"""The voxel observation (igw_vox_obs, VecGridWorld.vox_obs, obs['vox_obs']) on the GPU.  One
yardstick, exact: tests/vox_model.py, fed with the CPU oracle's states (tests/vox_cases.py); every comparison is
torch.equal on the raw bits.

1. kernel = model on every case and checkpoint, for five specs chosen to cover;  2. rows at every residue mod 16,
with canaries;  3. the stack and its episode boundaries through reset() and 40 steps;  4. the public surface;
5. an output past 2^32 bytes."""
import numpy as np
import pytest
import torch

import vox_cases as VC
import vox_model as VM

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
ALL4 = (('grid', 'onehot'), ('target', 'occ'), ('want', 'onehot'), ('todo', 'occ'))


def _specs():
    from gridworld_amd import VoxSpec
    return [VoxSpec(planes=ALL4),
            VoxSpec(frame='ego', radius=5, dtype=torch.float16, scale=1 / 3, bias=-0.1),
            VoxSpec(planes=(('grid', 'occ'), ('want', 'onehot')), frame='ego', radius=1, dtype=torch.bfloat16),
            VoxSpec(planes=(('grid', 'occ'), ('todo', 'occ'), ('target', 'occ')), agent=False, frame='ego', radius=10,
                    dtype=torch.float32)]


def _same(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    return torch.equal(VM.bits(got.cpu()), VM.bits(want))


def _model(truth, c, spec, rows=slice(None)):
    src = {k: truth[k][c][rows] for k in ('target', 'want', 'todo')}
    return VM.observe(VM.planes(truth['grid'][c][rows], truth['pose'][c][rows], src, spec), None, None, spec)


def _state_planes(env, spec, goal=None):
    """The model's planes of the env's OWN state (for the tests of the stack, where the state's truth is not the point)."""
    n = env.num_envs
    src = {'target': (env.task_target[env.env_task.long()] + env.task_start[env.env_task.long()])[:, :1089].cpu().numpy()}
    for k in spec.needs():
        src[k] = goal[k].cpu().numpy()
    return VM.planes(env.grid.cpu().numpy().reshape(n, -1), env.internals()[:, :4], src, spec)


def _compare_at_checkpoint(env, truth, c, name):
    from gridworld_amd import VoxSpec, vox as X
    n = env.num_envs
    goal = env.goal(want=True, todo=True)
    for spec in _specs():
        got = env.vox_obs(spec, goal=goal)
        assert tuple(got.shape) == spec.shape(n) and got.dtype is spec.dtype
        assert _same(got, _model(truth, c, spec)), (name, c, spec)
    # a source given as a contiguous [n, 9, 11, 11] tensor at an odd address (stride 1089), through the library's entry
    spec = VoxSpec(planes=(('grid', 'onehot'), ('grid', 'occ')), frame='ego', radius=3)
    flat = torch.zeros(n * 1089 + 1, dtype=torch.int8, device=env.device)[1:]
    flat.view(n, 1089).copy_(env.grid.reshape(n, 1089))
    assert flat.data_ptr() % 2 == 1
    rows = (flat.data_ptr(), None, 1089, 0)
    got = X.launch(env.agent_buf, env.aux_buf, n, spec, [rows, rows], None, None, False, env.device, env._stream())
    assert _same(got, _model(truth, c, spec)), (name, c, 'dense rows')


# ---- 1. against the model on the oracle's states, case by case -----------------------------------------------------------
@pytest.mark.parametrize('name', list(VC.walking_cases()))
def test_kernel_equals_the_model_on_the_walking_cases(name):
    from gridworld_amd import VecGridWorld
    case, truth = VC.walking_cases()[name], VC.walking_truth(name)
    env = VecGridWorld(VC.E, **case['kw'])
    env.set_tasks(case['targets'], case['starts'], init_pose=case['poses'])
    env.reset()
    acts = torch.from_numpy(case['actions']).to(env.device)
    t = 0
    for c, tc in enumerate(VC.CHECKPOINTS):
        while t < tc:
            env.step(acts[t])
            t += 1
        _compare_at_checkpoint(env, truth, c, name)


def test_kernel_equals_the_model_on_the_flying_batch():
    from gridworld_amd import VecGridWorld
    case, truth = VC.flying_case(), VC.flying_truth()
    env = VecGridWorld(VC.FLY_N, autoreset=True, **case['kw'])
    env.set_tasks(case['targets'])
    env.reset()
    t = 0
    for c, tc in enumerate(VC.FLY_CHECKPOINTS):
        while t < tc:
            env.step(case['actions'][t])
            t += 1
        _compare_at_checkpoint(env, truth, c, 'flying')


@pytest.mark.parametrize('flying', [False, True])
def test_kernel_equals_the_model_on_the_directed_reset_poses(flying):
    from gridworld_amd import VecGridWorld
    case, truth = VC.directed_case(flying), VC.directed_truth(flying)
    env = VecGridWorld(len(case['poses']), **case['kw'])
    env.set_tasks(case['targets'], case['starts'], init_pose=case['poses'])
    env.reset()
    assert np.array_equal(env.internals()[:, :4], truth['pose'][0])
    _compare_at_checkpoint(env, truth, 0, 'directed')


# ---- 2. rows at every residue mod 16 ---------------------------------------------------------------------------------------
def _small_env(n, **kw):
    from gridworld_amd import VecGridWorld, workloads
    env = VecGridWorld(n, size_reward=False, **kw)
    env.set_tasks(workloads.rt20(n, seed=2).numpy())
    env.reset()
    acts = env.fill_actions(12, seed=5)
    for t in range(12):
        env.step(acts[t])
    return env


@pytest.mark.parametrize('dtype, offset', [(torch.uint8, 0), (torch.uint8, 1), (torch.float16, 0), (torch.float16, 1),
                                           (torch.float32, 3)])
def test_misaligned_rows_and_canaries(dtype, offset):
    """n = 5, one occupancy plane, ego R = 1, stack 2: a slot is 81 elements and an env's run 162, so every slot starts
    at another residue mod 16; `offset`: elements between a 16-byte boundary and the output."""
    from gridworld_amd import VoxSpec
    n = 5
    env = _small_env(n, max_steps=250)
    spec = VoxSpec(planes=(('grid', 'occ'),), agent=False, frame='ego', radius=1, dtype=dtype, stack=2)
    count = int(np.prod(spec.shape(n)))
    assert count == n * 162
    pad = 64
    buf = torch.full((pad + offset + count + pad,), 7, dtype=dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    out = buf[pad + offset:pad + offset + count].view(spec.shape(n))
    assert out.data_ptr() % 16 == (offset * out.element_size()) % 16
    first = VM.observe(_state_planes(env, spec), None, None, spec)
    assert env.vox_obs(spec, out=out, fill=True) is out
    assert _same(out, first)
    env.step(env.fill_actions(1, seed=6)[0])
    restart = torch.tensor([0, 1, 0, 0, 255], dtype=torch.uint8, device=DEV)
    env.vox_obs(spec, out=out, restart=restart)
    assert _same(out, VM.observe(_state_planes(env, spec), first, restart.cpu().numpy(), spec))
    canary = torch.cat([buf[:pad + offset], buf[pad + offset + count:]]).cpu()
    assert bool((canary == 7).all())


# ---- 3. the stack and its episode boundaries --------------------------------------------------------------------------------
def _busy_env(name='looking_down', **kw):
    """An env of a walking case whose grids keep changing (40 % of the actions place, 15 % break), not yet reset, and
    the case's actions [48, 32] on the device."""
    from gridworld_amd import VecGridWorld
    case = VC.walking_cases()[name]
    env = VecGridWorld(VC.E, **dict(case['kw'], **kw))
    env.set_tasks(case['targets'], case['starts'], init_pose=case['poses'])
    return env, torch.from_numpy(case['actions']).to(DEV)


STACKED = dict(planes=(('grid', 'onehot'), ('target', 'occ')), frame='ego', radius=2, dtype=torch.float16, stack=4,
               scale=0.5, bias=-0.25)


@pytest.mark.parametrize('autoreset', [True, False])
def test_obs_key_follows_reset_and_40_steps(autoreset):
    from gridworld_amd import VoxSpec
    n, spec = VC.E, VoxSpec(**STACKED)
    env, acts = _busy_env(max_steps=16, autoreset=autoreset, vox_obs=dict(STACKED))
    obs = env.reset()
    env.set_step_no(np.arange(n) % 5)   # the episodes end at different steps
    held = obs['vox_obs']
    assert tuple(held.shape) == spec.shape(n) and held.dtype is torch.float16
    want = VM.observe(_state_planes(env, spec), None, None, spec)
    assert _same(held, want)
    rng = np.random.RandomState(1)
    restarts = told_apart = 0

    def follow(want, restart):
        new = _state_planes(env, spec)
        shifted = VM.observe(new, want, None, spec)
        want = VM.observe(new, want, restart, spec)
        return want, int(not torch.equal(VM.bits(shifted), VM.bits(want)))
    for t in range(40):
        obs, _, done, _ = env.step(acts[t])
        assert obs['vox_obs'] is held
        restarts += int(done.sum()) if autoreset else 0
        want, apart = follow(want, done.cpu().numpy() if autoreset else None)
        told_apart += apart
        assert _same(held, want), t
        if not autoreset and t % 6 == 5:
            mask = rng.choice(np.array([0, 0, 1, 255], np.uint8), n)
            obs = env.reset(torch.from_numpy(mask).to(DEV))
            restarts += int((mask != 0).sum())
            assert obs['vox_obs'] is held
            want, apart = follow(want, mask)
            told_apart += apart
            assert _same(held, want), ('reset(mask)', t)
    print(f'autoreset={autoreset}: {restarts} stacks restarted; a restart changed the stack in {told_apart} writes')
    assert restarts >= n and told_apart >= 3     # (a kernel that ignored `restart`, or always filled, would be seen)
    assert not torch.equal(held[:, :spec.channels], held[:, -spec.channels:])   # the slots do hold different steps


def test_next_write_fills_after_an_unfollowed_move():
    from gridworld_amd import VoxSpec
    spec = VoxSpec(**STACKED)
    env, acts = _busy_env(vox_obs=spec)
    env.reset()
    for t in range(20):
        env.step(acts[t])
    held = env.obs()['vox_obs']
    assert not _same(held, VM.observe(_state_planes(env, spec), None, None, spec))   # a stack of different steps
    snap = env.state_dict()
    env.rollout_actions(acts[20:30].contiguous())
    env.step(acts[30])
    assert _same(held, VM.observe(_state_planes(env, spec), None, None, spec))
    for t in range(31, 40):
        env.step(acts[t])
    assert not _same(held, VM.observe(_state_planes(env, spec), None, None, spec))
    env.load_state_dict(snap)
    env.step(acts[20])
    assert _same(held, VM.observe(_state_planes(env, spec), None, None, spec))


def test_restart_is_read_at_stride_64_and_at_stride_1():
    from gridworld_amd import VoxSpec
    n = 9
    env = _small_env(n, max_steps=14, autoreset=True)       # the step after the 12 of _small_env is not the last; the next is
    spec = VoxSpec(planes=(('grid', 'occ'),), frame='ego', radius=2, stack=3)
    out = env.vox_obs(spec)
    a = env.fill_actions(4, seed=8)
    env.set_step_no(np.where(np.arange(n) % 2 == 0, 13, 3))   # every second env ends with the next step
    env.step(a[0])
    done = env.done
    assert done.stride(0) == 64 and done.cpu().tolist() == [1, 0] * 4 + [1]
    prev = out.cpu()
    env.vox_obs(spec, out=out, restart=done)
    want = VM.observe(_state_planes(env, spec), prev, done.cpu().numpy(), spec)
    assert _same(out, want)
    env.step(a[1])
    mask = torch.tensor([0, 0, 1, 0, 0, 255, 0, 0, 0], dtype=torch.uint8, device=DEV)
    env.vox_obs(spec, out=out, restart=mask)
    want = VM.observe(_state_planes(env, spec), want, mask.cpu().numpy(), spec)
    assert _same(out, want)
    env.vox_obs(spec, out=out, restart=[True, False] * 4 + [False])      # (host data is converted)
    assert _same(out, VM.observe(_state_planes(env, spec), want, np.array([1, 0] * 4 + [0]), spec))


# ---- 4. the surface -----------------------------------------------------------------------------------------------------------
def test_out_is_written_without_an_allocation():
    from gridworld_amd import VoxSpec
    env = _small_env(16, max_steps=250)
    spec = VoxSpec(dtype=torch.float16, stack=2)
    out = env.vox_obs(spec)
    restart = torch.zeros(16, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats(DEV)['allocation.all.allocated']
    assert env.vox_obs(spec, out=out, restart=restart) is out
    assert torch.cuda.memory_stats(DEV)['allocation.all.allocated'] == before
    for bad in (out[:8], out.to(torch.float32), out.cpu(), out.transpose(3, 4)):
        with pytest.raises(ValueError):
            env.vox_obs(spec, out=bad)
    with pytest.raises(ValueError):
        env.vox_obs(spec, out=out, restart=torch.zeros(15, dtype=torch.uint8, device=DEV))


def test_sub_batches_write_their_rows_on_their_own_streams():
    from gridworld_amd import VoxSpec
    env = _small_env(16, max_steps=250)
    spec = VoxSpec(planes=ALL4, frame='ego', radius=4, dtype=torch.bfloat16)
    whole = env.vox_obs(spec, goal=env.goal(want=True, todo=True))
    torch.cuda.synchronize()
    parts = env.split(4)
    for k, sub in enumerate(parts):
        got = sub.vox_obs(spec, goal=sub.goal(want=True, todo=True))
        sub.synchronize()
        assert _same(got, whole[4 * k:4 * k + 4].cpu())


def test_goal_planes_and_the_obs_key_with_goal():
    from gridworld_amd import VecGridWorld, VoxSpec, workloads
    n, spec = 10, VoxSpec(planes=ALL4, dtype=torch.float32, scale=2.0, bias=1.0)
    env = VecGridWorld(n, size_reward=False, goal=('want', 'todo'), vox_obs=spec)
    env.set_tasks(workloads.rt20(n, seed=6).numpy())
    obs = env.reset()
    acts = env.fill_actions(15, seed=2)
    for t in range(15):
        obs = env.step(acts[t])[0]
    assert _same(obs['vox_obs'], VM.observe(_state_planes(env, spec, obs), None, None, spec))
    goal = env.goal(want=True, todo=True)
    assert bool((goal['want'] != 0).any()) and torch.equal(goal['want'], obs['want'])
    assert _same(env.vox_obs(spec, goal=goal), VM.observe(_state_planes(env, spec, goal), None, None, spec))
    with pytest.raises(ValueError):
        env.vox_obs(spec)
    halves = env.split(2)                       # children inherit their rows of the tensor and of the goal's planes
    assert halves[1].obs()['vox_obs'].data_ptr() == obs['vox_obs'][5:].data_ptr()
    obs['vox_obs'].fill_(7.0)
    torch.cuda.synchronize()
    halves[1].step_walking_ptr(acts[0, 5:].contiguous())
    halves[1].synchronize()
    want = VM.observe(_state_planes(env, spec, env.obs()), None, None, spec)
    assert _same(obs['vox_obs'][5:], want[5:]) and bool((obs['vox_obs'][:5] == 7.0).all())   # its rows, and no others


@pytest.mark.parametrize('stack', [1, 3])
def test_a_captured_chain_leaves_what_the_eager_loop_leaves(stack):
    from gridworld_amd import VoxSpec
    T = 6
    spec = VoxSpec(planes=(('grid', 'onehot'), ('todo', 'occ')), frame='ego', radius=3, dtype=torch.float16, stack=stack)
    (eager, acts), (graphed, _) = (_busy_env('towers', max_steps=9, autoreset=True, goal=('todo',), vox_obs=spec)
                                   for _ in range(2))
    eager.reset()
    graphed.reset()
    buf = acts[:T].clone()
    graph = graphed.capture_steps(buf)
    c, moved = spec.channels, 0
    for rounds in range(3):     # (from the second replay on the stack is current: no fill; episodes end in the second)
        buf.copy_(acts[rounds * T:(rounds + 1) * T])
        for t in range(T):
            eager.step(buf[t])
        obs = graph.replay()[0]
        assert obs['vox_obs'] is graphed.obs()['vox_obs']
        assert _same(obs['vox_obs'], eager.obs()['vox_obs'].cpu()), rounds
        moved += int(not torch.equal(obs['vox_obs'][:, :c], obs['vox_obs'][:, -c:]))
    assert torch.equal(eager.grid_buf, graphed.grid_buf)
    assert stack == 1 or moved >= 1     # the slots did hold different steps


def test_facade_returns_row_0_as_numpy():
    import gridworld_amd as G
    env = G.make('IGLUGridworldVector-v0', size_reward=False)
    env.set_task(G.dummy_task())
    env.reset()
    for a in (14, 14, 14, 14, 14, 14, 14, 14, 14, 17, 13, 17, 2, 8, 17):
        env.step(a)
    gw = env.unwrapped
    spec = G.VoxSpec(planes=ALL4, frame='ego', radius=5, dtype=torch.float16, stack=2)
    got = gw.vox_obs(spec)
    assert isinstance(got, np.ndarray) and got.dtype == np.float16 and got.shape == spec.shape(1)[1:]
    v = gw._vec
    goal = {k: t.cpu() for k, t in v.goal(want=True, todo=True).items()}
    want = VM.observe(_state_planes(v, spec, goal), None, None, spec)
    assert np.array_equal(got.view(np.int16), want[0].numpy().view(np.int16))
    assert got.any() and gw.vox_obs(dict(dtype='bfloat16')).dtype == np.float32


def test_the_call_leaves_the_state_alone_and_the_key_does_not_change_the_step():
    from gridworld_amd import VecGridWorld, VoxSpec, workloads
    n = 32
    spec = VoxSpec(planes=ALL4, stack=2)
    envs = []
    for kw in (dict(), dict(goal=('want', 'todo'), vox_obs=spec)):
        env = VecGridWorld(n, size_reward=False, max_steps=20, autoreset=True, **kw)
        env.set_tasks(workloads.rt20(n, seed=5).numpy())
        env.reset()
        envs.append(env)
    plain, keyed = envs
    acts = plain.fill_actions(50, seed=1)
    for t in range(50):
        plain.step(acts[t])
        keyed.step(acts[t])
    a, b = plain.state_dict(), keyed.state_dict()
    assert all(torch.equal(a[k], b[k]) for k in VecGridWorld._STATE_KEYS)
    assert torch.equal(plain.stats_tensor(), keyed.stats_tensor())
    goal = plain.goal(want=True, todo=True)
    before, stats = plain.state_dict(), plain.stats_tensor().clone()
    for s in _specs():
        plain.vox_obs(s, goal=goal)
    after = plain.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in VecGridWorld._STATE_KEYS)
    assert torch.equal(stats, plain.stats_tensor())


# ---- 5. 64-bit offsets ----------------------------------------------------------------------------------------------------------
def test_rows_on_both_sides_of_byte_2_to_the_32():
    """ego R = 10, 25 channels, f32, stack 8: 3,175,200 bytes per env, so 1,400 envs end past 2^32 bytes; rows 0, the two
    around byte 2^32 and the last against the model, after a fill and after a shift."""
    from gridworld_amd import VecGridWorld, VoxSpec, workloads
    n = 1400
    spec = VoxSpec(planes=tuple((k, 'onehot') for k in ('grid', 'target', 'want', 'todo')), frame='ego', radius=10,
                   dtype=torch.float32, stack=8, scale=0.75, bias=0.125)
    row = int(np.prod(spec.shape(1))) * 4
    total = n * row
    assert row == 3175200 and total > 1 << 32
    free = torch.cuda.mem_get_info(DEV)[0]
    if free < total + (1 << 30):
        print(f'skipped: {free} bytes free on the device, the output alone takes {total}')
        pytest.skip('the device lacks the memory for an output past 2^32 bytes')
    env = VecGridWorld(n, size_reward=False, max_steps=250)
    env.set_tasks(workloads.rt20(n, seed=12).numpy())
    env.reset()
    # SURVEY Appendix B's opening (tests/mask_cases.py: _script): look down, land -- then, between the two calls, place
    acts = torch.tensor([14] * 9 + [0] * 3 + [17], dtype=torch.int32, device=DEV).repeat(n, 1).t().contiguous()
    for t in range(12):
        env.step(acts[t])
    at = (1 << 32) // row
    rows = [0, at, at + 1, n - 1]
    assert at * row < 1 << 32 < (at + 1) * row and at + 1 < n - 1

    def model(prev):
        goal = {k: t[rows].cpu() for k, t in env.goal(want=True, todo=True).items()}
        src = {'target': (env.task_target[env.env_task.long()] + env.task_start[env.env_task.long()])[rows, :1089].cpu().numpy(),
               'want': goal['want'].numpy(), 'todo': goal['todo'].numpy()}
        new = VM.planes(env.grid[rows].cpu().numpy(), env.internals()[rows, :4], src, spec)
        return VM.observe(new, prev, None, spec)
    out = env.vox_obs(spec, goal=env.goal(want=True, todo=True))
    assert out.numel() * 4 == total
    first = model(None)
    assert _same(out[rows], first)
    env.step(acts[12])
    env.vox_obs(spec, out=out, goal=env.goal(want=True, todo=True))
    second = model(first)
    assert _same(out[rows], second) and not torch.equal(first, second)
