"""The action mask (igw_action_mask, VecGridWorld.action_mask, obs['action_mask']) on the GPU.
Two yardsticks, both exact (0 mismatches): the CPU oracle's answer to "would action a change the world"
(tests/mask_cases.py), and the step kernel itself on whole wavefronts and tails.

Against the oracle: 6 cases x 6 checkpoints x 32 envs x (18 bits + 2 cells).  Against the step: 9 x 2,049 envs, the 8
probe actions and the jump and pitch actions.  No mismatch is allowed in either."""
import ctypes as C

import numpy as np
import pytest
import torch

import mask_cases as MC

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1


def _gpu_env(case, n_blocks=1, **kw):
    from gridworld_amd import VecGridWorld
    tile = lambda a: None if a is None else np.concatenate([a] * n_blocks)  # noqa: E731
    env = VecGridWorld(MC.E * n_blocks, **dict(case['kw'], **kw))
    env.set_tasks(tile(case['targets']), tile(case['starts']), init_pose=tile(case['poses']))
    return env


# ---- 1. against the oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(MC.cases()))
def test_mask_and_look_equal_the_oracle_truth(name):
    case = MC.cases()[name]
    masks, looks = MC.truth(name)
    env = _gpu_env(case)
    env.reset()
    acts = torch.from_numpy(case['actions']).to(env.device)
    t, bad_bits, bad_cells = 0, 0, 0
    for c, tc in enumerate(MC.CHECKPOINTS):
        while t < tc:
            env.step(acts[t])
            t += 1
        mask, look = env.action_mask(look=True)
        assert mask.dtype == torch.uint8 and tuple(mask.shape) == (MC.E, 18)
        assert look.dtype == torch.int16 and tuple(look.shape) == (MC.E, 2)
        bad_bits += int((mask.cpu().numpy() != masks[c]).sum())
        bad_cells += int((look.cpu().numpy() != looks[c]).sum())
    print(f'{name}: {bad_bits} of {masks.size} bits and {bad_cells} of {looks.size} cells differ from the oracle')
    assert bad_bits == 0 and bad_cells == 0


# ---- 2. against the step, whole wavefronts and tails -----------------------------------------------------------------
B = 2049   # 128 whole wavefronts of 16 envs and a tail of one; nine blocks: 18,441 envs


def _nine_blocks(**kw):
    """Nine identical blocks of B rt20 envs, half of them at poses off the 5-degree lattice (the step's general
    sincos), driven by 30 common actions of the looking-down stream."""
    from gridworld_amd import VecGridWorld, workloads
    targets = workloads.rt20(B, seed=8).numpy().astype(np.int8)
    rng = np.random.RandomState(8)
    pose = np.zeros((B, 5))
    odd = np.arange(B) % 2 == 1
    pose[odd] = np.stack([rng.uniform(-4, 4, B), np.zeros(B), rng.uniform(-4, 4, B), rng.uniform(-180, 180, B),
                          rng.uniform(-20, 20, B)], 1)[odd]
    env = VecGridWorld(9 * B, size_reward=False, max_steps=250, **kw)
    env.set_tasks(np.concatenate([targets] * 9), init_pose=np.concatenate([pose] * 9))
    env.reset()
    acts = torch.from_numpy(np.tile(MC.stream(9, n=B)[:30], (1, 9))).to(env.device)
    for t in range(30):
        env.step(acts[t])
    return env


def _guarded(nbytes, dev):
    buf = torch.full((64 + nbytes + 64,), 0xA5, dtype=torch.uint8, device=dev)
    return buf, buf.data_ptr() + 64


def test_mask_predicts_the_step_on_whole_wavefronts_and_tails():
    from gridworld_amd import query as Q
    env = _nine_blocks()
    dev, N = env.device, 9 * B
    mask, look, actions = env.action_mask(look=True, sample=(5, 3))
    for j in range(1, 9):   # identical blocks: identical rows (the sampled action is keyed by the env index)
        assert torch.equal(mask[:B], mask[j * B:(j + 1) * B]) and torch.equal(look[:B], look[j * B:(j + 1) * B])
    # the C entry on the first n rows: the same bytes, nothing outside them
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for n in (1, 15, 17, B):
        bufs = [_guarded(n * w, dev) for w in (18, 4, 4)]
        Q.action_mask_into(env.agent_buf.data_ptr(), env.occ_buf.data_ptr(), n, True, bufs[0][1], bufs[1][1], bufs[2][1],
                           5, 3, env.env_index_base, stream)
        for (buf, _), want in zip(bufs, (mask, look, actions)):
            assert (buf[:64] == 0xA5).all() and (buf[-64:] == 0xA5).all(), n
            assert torch.equal(buf[64:-64], want[:n].contiguous().view(torch.uint8).reshape(-1)), n
        # ... and the mask at an address that is not dword-aligned (a sub-batch at an odd row)
        buf, p = _guarded(n * 18 + 2, dev)
        Q.action_mask_into(env.agent_buf.data_ptr(), env.occ_buf.data_ptr(), n, True, p + 2, None, None, 0, 0, 0, stream)
        assert (buf[:66] == 0xA5).all() and (buf[-64:] == 0xA5).all(), n
        assert torch.equal(buf[66:-64], mask[:n].reshape(-1)), n
    # block j + 1 takes probe action j, block 0 a no-op: a row changes iff its bit was set
    before = env.grid_buf.clone()
    a = torch.zeros(N, dtype=torch.int32, device=dev)
    for j, p in enumerate(MC.PROBES):
        a[(j + 1) * B:(j + 2) * B] = p
    env.step(a)
    changed = (env.grid_buf != before).any(1)
    assert not changed[:B].any()
    m0 = mask[:B].bool()
    wrong = 0
    for j, p in enumerate(MC.PROBES):
        rows = slice((j + 1) * B, (j + 2) * B)
        wrong += int((changed[rows] != m0[:, p]).sum())
        if p >= 16:   # ... and the cell that changed is the one `look` named
            cell = (env.grid_buf[rows] != before[rows]).int().argmax(1)
            want = look[:B, p - 16].long()
            assert torch.equal(torch.where(changed[rows], cell, torch.full_like(cell, -1)), want)
        print(f'action {p}: {int(m0[:, p].sum())} of {B} envs can')
        assert 50 <= int(m0[:, p].sum()) <= B - 50
    assert wrong == 0
    # the jump and pitch bits against the step as well: the pose moves iff the bit was set
    env2 = _nine_blocks()
    m = env2.action_mask()[:B].bool()
    pose0 = torch.from_numpy(env2.internals()[:B])
    a = torch.zeros(N, dtype=torch.int32, device=dev)
    a[B:2 * B], a[2 * B:3 * B], a[3 * B:4 * B] = 5, 14, 15
    env2.step(a)
    st = torch.from_numpy(env2.internals())
    jumped = st[B:2 * B, 5] != st[:B, 5]     # against the no-op's block: a jump that starts leaves another dy
    assert torch.equal(jumped, m[:, 5].cpu()) and torch.equal(pose0[:, 5] == 0.0, m[:, 5].cpu())
    assert 50 <= int(jumped.sum()) <= B - 50
    assert torch.equal(st[2 * B:3 * B, 4] != pose0[:, 4], m[:, 14].cpu())
    assert torch.equal(st[3 * B:4 * B, 4] != pose0[:, 4], m[:, 15].cpu())


# ---- 3. no side effects -----------------------------------------------------------------------------------------------
def test_the_query_writes_nothing_but_its_outputs():
    env = _gpu_env(MC.cases()['towers'])
    env.reset()
    acts = torch.from_numpy(MC.cases()['towers']['actions']).to(env.device)
    for t in range(12):
        env.step(acts[t])
    keys = ('agent_buf', 'occ_buf', 'grid_buf', 'aux_buf', 'out_buf', 'hist_buf')
    before = {k: getattr(env, k).clone() for k in keys}
    first = env.action_mask(look=True, sample=(1, 2))
    again = env.action_mask(look=True, sample=(1, 2))
    torch.cuda.synchronize()
    for k in keys:
        assert torch.equal(getattr(env, k), before[k]), k
    for x, y in zip(first, again):
        assert torch.equal(x, y)
    out = torch.zeros((MC.E, 18), dtype=torch.uint8, device=env.device)
    assert env.action_mask(out=out) is out and torch.equal(out, first[0])
    with pytest.raises(ValueError):
        env.action_mask(out=torch.zeros((MC.E, 17), dtype=torch.uint8, device=env.device))


# ---- 4. plumbing --------------------------------------------------------------------------------------------------------
def _fresh(env):
    m = env.action_mask()
    assert m is not env._mask
    return m


def test_obs_action_mask_follows_reset_step_autoreset_and_replay():
    case = MC.cases()['looking_down']
    env = _gpu_env(case, autoreset=True, action_mask=True, max_steps=11)
    acts = torch.from_numpy(case['actions']).to(env.device)
    obs = env.reset()
    held = obs['action_mask']
    assert held.dtype == torch.uint8 and tuple(held.shape) == (MC.E, 18)
    assert torch.equal(held, _fresh(env))
    for t in range(14):   # the time limit ends every episode at step 11: the mask then shows the new episode's state
        obs, _, done, _ = env.step(acts[t])
        assert obs['action_mask'] is held and torch.equal(held, _fresh(env)), t
        # the tensor moves with the state: at pitch -10 the ground is more than 8 units away along the ray (nothing to
        # place on), at -15 every env sees it inside the build zone, with a full inventory
        if t == 1:
            assert int(held[:, 17].sum()) == 0
        if t == 2:
            assert int(held[:, 17].sum()) == MC.E
        if t == 9:
            assert int(held[:, 17].sum()) >= 8
        if t == 10:
            assert done.all() and int(held[:, 16].sum()) == 0 and int(held[:, 17].sum()) == 0   # looking ahead again
    some = torch.arange(MC.E, device=env.device) % 3 == 0
    obs = env.reset(some)
    assert obs['action_mask'] is held and torch.equal(held, _fresh(env))
    assert int(held[some][:, 17].sum()) == 0
    # a captured loop: the launch follows every step of the chain; after the replay the tensor shows the last state
    for chains in (1, 2):
        g = env.capture_steps(acts[14:20].contiguous(), chains=chains)
        obs, _, _, _ = g.replay()
        assert obs['action_mask'] is held and torch.equal(held, _fresh(env)), chains
        env.step(acts[20])    # (moves the state, so that the second replay starts somewhere else)
        obs, _, _, _ = g.replay()
        assert torch.equal(obs['action_mask'], _fresh(env)), chains
        del g
    # whatever else moves the state takes the mask along
    state = env.state_dict()
    env.step(acts[21])
    env.load_state_dict(state)
    assert torch.equal(held, _fresh(env))
    env.rollout_actions(acts[22:25])
    assert torch.equal(held, _fresh(env))


def test_sub_batches_query_their_own_rows_on_their_own_stream():
    case = MC.cases()['towers']
    env = _gpu_env(case, action_mask=True)
    env.reset()
    acts = torch.from_numpy(case['actions']).to(env.device)
    for t in range(12):
        env.step(acts[t])
    whole, wlook, wact = env.action_mask(look=True, sample=(7, 1))
    subs = env.split(2)
    h = MC.E // 2
    for k, s in enumerate(subs):
        m, lk, a = s.action_mask(look=True, sample=(7, 1))
        s.synchronize()
        rows = slice(k * h, (k + 1) * h)
        assert torch.equal(m, whole[rows]) and torch.equal(lk, wlook[rows])
        assert torch.equal(a, wact[rows])          # keyed by the global env index
        assert s.obs()['action_mask'].data_ptr() == env._mask[rows].data_ptr()
    for k, s in enumerate(subs):                    # stepped on its own: its rows of obs['action_mask'] follow
        s.step_walking_ptr(acts[12, k * h:(k + 1) * h].contiguous())
        s.join()
    assert torch.equal(env._mask, _fresh(env))


def test_the_facade_answers_for_its_one_env():
    import gridworld_amd as G
    case = MC.cases()['appendix_b']
    col = 0                                         # env 0 runs the script from step 0
    from gridworld_amd import VecGridWorld
    vec = VecGridWorld(1, **case['kw'])
    vec.set_tasks(case['targets'][:1])
    vec.reset()
    env = G.make('IGLUGridworldVector-v0', size_reward=False)
    env.set_task(G.Task('', case['targets'][col].astype(np.int32)))
    env.reset()
    for t in range(26):
        m = env.unwrapped.action_mask()
        assert m.dtype == np.bool_ and m.shape == (18,)
        assert np.array_equal(m, vec.action_mask()[0].cpu().numpy().astype(bool)), t
        a = int(case['actions'][t, col])
        _, _, _, info = env.step(a)
        assert info == {}
        vec.step(torch.tensor([a], dtype=torch.int32))
    assert np.array_equal(m, MC.truth('appendix_b')[0][4, col].astype(bool))   # step 25 is a checkpoint


# ---- 5. sampling --------------------------------------------------------------------------------------------------------
def _splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _sample_model(mask, seed, t, env_offset):
    """include/igw_query.h: the k-th set bit of env i's mask, k = (r * popcount) >> 32, r the high word of the hash."""
    out = np.zeros(len(mask), np.int32)
    for i, row in enumerate(mask):
        e = (env_offset + i) & M64
        h = _splitmix64(seed ^ _splitmix64((e * 0x9E3779B1 + t * 0x100000001B3 + 0x6d61736b) & M64))
        bits = np.flatnonzero(row)
        out[i] = bits[((h >> 32) * len(bits)) >> 32]
    return out


def test_sampled_actions_follow_the_documented_hash_and_cover_the_mask():
    from gridworld_amd import VecGridWorld, workloads
    n, base, seed = 4096, 1000, 0xDEADBEEFCAFE
    env = VecGridWorld(n, size_reward=False, env_index_base=base)
    env.set_tasks(workloads.rt20(n, seed=2).numpy())
    env.reset()
    acts = torch.from_numpy(MC.stream(12, n=n)[:14]).to(env.device)
    for t in range(14):
        env.step(acts[t])
    ever, drawn = np.zeros(18, bool), np.zeros(18, bool)
    for t in (0, 1, 2, 3, 250, 1 << 20, 1 << 40, M64):
        mask, a = env.action_mask(sample=(seed, t))
        assert a.dtype == torch.int32 and tuple(a.shape) == (n,)
        mask, a = mask.cpu().numpy(), a.cpu().numpy()
        assert np.array_equal(a, _sample_model(mask, seed, t, base)), t
        assert (mask[np.arange(n), a] == 1).all()
        ever |= mask.any(0)
        drawn[np.unique(a)] = True
    assert ever.all() and np.array_equal(drawn, ever)


# ---- 6. errors -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kw', [dict(action_space='flying'), dict(discretize=False)])
def test_flying_and_dict_envs_raise(kw):
    import gridworld_amd as G
    from gridworld_amd import VecGridWorld
    env = VecGridWorld(4, **kw)
    with pytest.raises(ValueError):
        env.action_mask()
    with pytest.raises(ValueError):
        VecGridWorld(4, action_mask=True, **kw)
    one = G.make('IGLUGridworldVector-v0', **kw)
    with pytest.raises(ValueError):
        one.unwrapped.action_mask()
