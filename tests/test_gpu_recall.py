"""The recall query (igw_recall, G.recall, VecGridWorld.recall, SubBatch.recall) on the GPU.
Yardstick, exact (0 mismatching bits): the numpy model of tests/recall_model.py -- which tests/test_recall_cpu.py pins to
the stepped CPU oracle and to tests/vox_model.py's own stack rule -- on the oracle's grids and float32 poses for the real
logs of the eight shared cases, on hand-written records for what the physics never writes, and the live vox_obs stack
where the float32 log and the float64 state agree on the head cell."""
import numpy as np
import pytest
import torch

from gridworld_amd import recall as _feature  # noqa: F401  (without the query nothing in this file can run)

import recall_cases as RCC
import recall_model as RCM
import relabel_cases as RC
import vox_model as VM

pytestmark = pytest.mark.gpu

E, T = RCC.E, RCC.T
ROW, CAP = 1104, 64          # the logs of this file hold 64 steps per slot
DEV = torch.device('cuda:0')
ALL = ('obs', 'next_obs', 'record', 'valid')


def _spec(**kw):
    from gridworld_amd import VoxSpec
    return VoxSpec(**kw)


def _specs():
    """The five layouts of the exhaustive comparison."""
    both = (('grid', 'onehot'), ('grid', 'occ'), ('target', 'onehot'), ('target', 'occ'))
    return {'world_u8': _spec(planes=both, agent=True, dtype=torch.uint8, stack=1),
            'ego5_f16': _spec(planes=(('grid', 'onehot'), ('target', 'occ')), agent=True, frame='ego', radius=5,
                              dtype=torch.float16, scale=1 / 3, bias=-0.1, stack=4),
            'ego1_bf16': _spec(planes=(('grid', 'onehot'),), agent=True, frame='ego', radius=1, dtype=torch.bfloat16, stack=8),
            'ego10_f32': _spec(planes=(('grid', 'occ'), ('target', 'occ')), agent=False, frame='ego', radius=10,
                               dtype=torch.float32, stack=2),
            'odd_goal': _spec(planes=(('target', 'onehot'), ('grid', 'occ')), agent=True, dtype=torch.uint8, stack=2)}


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


def _rows(a, dev=DEV):
    """int8 numpy [..., 1089] -> device tensor [..., 1104]."""
    out = np.zeros(a.shape[:-1] + (ROW,), np.int8)
    out[..., :1089] = a
    return torch.from_numpy(out).to(dev)


def _same(got, want, where=''):
    """Every bit of every output named in `want` (the model's dict) equals `got` (the dict recall returned)."""
    for k in ('obs', 'next_obs'):
        if k in want and k in got:
            g, w = got[k].cpu(), want[k]
            assert g.dtype == w.dtype and g.shape == w.shape, (where, k, g.dtype, g.shape, w.dtype, w.shape)
            bad = int((VM.bits(g) != VM.bits(w)).sum())
            assert bad == 0, f'{where} {k}: {bad} of {w.numel()} elements differ'
    for k in ('record', 'valid'):
        if k in want and k in got:
            g = got[k].cpu().numpy()
            assert g.dtype == want[k].dtype and g.shape == want[k].shape, (where, k)
            assert np.array_equal(g, want[k]), f'{where} {k}: {int((g != want[k]).sum())} bytes differ'


@pytest.fixture(scope='module')
def logs():
    """name -> (env, records, heads, first, length) of the case's real log, made once."""
    made = {}

    def get(name):
        if name not in made:
            env, rec, heads = _logged(RCC.cases()[name])
            made[name] = (env, rec, heads) + _episodes(heads, CAP)
        return made[name]
    return get


def _oracle_log(name):
    """The records the oracle's run implies (change words and float32 poses, everything else zero) and where each env's
    episode lies in them."""
    b = RCC.base(name)
    return b, RCC.records_of(b['change'], b['pos']), np.arange(E) * T, np.full(E, T)


# ---- 1. exhaustive on real logs ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(RCC.cases()))
def test_every_logged_transition_of_a_real_log_equals_the_model(name, logs):
    """All 32 x 48 (e, t) pairs of the case, five layouts: obs and next_obs against the model on the ORACLE's grids and
    float32 poses (so the log is checked on the way), record against the log's own rows, valid all 1."""
    import gridworld_amd as G
    env, rec, heads, first, length = logs(name)
    assert (length == T).all()
    b, orec, ofirst, olen = _oracle_log(name)
    # the log holds the oracle's change words and poses; the task table the reset pose
    slot = ((first // CAP) % 2).cpu().numpy()
    mine = rec.cpu().numpy()[np.arange(E), slot, :T]                     # [E, T, 64]
    assert np.array_equal(mine[:, :, 40:42], orec.reshape(E, T, 64)[:, :, 40:42])
    assert np.array_equal(mine[:, :, 0:20], orec.reshape(E, T, 64)[:, :, 0:20])
    init = env.task_meta[:E, :40].contiguous().view(torch.float64)
    assert np.array_equal(init.cpu().numpy(), b['init'])
    episode, step = RCC.pairs()
    targets = RCC.cases()[name]['targets'].reshape(E, -1).astype(np.int8)
    goal = torch.from_numpy(targets).to(DEV).view(E, 9, 11, 11)
    odd = torch.zeros(E * 1089 + 1, dtype=torch.int8, device=DEV)[1:].view(E, 1089)
    odd.copy_(goal.view(E, 1089))
    assert odd.data_ptr() % 2 == 1 and odd.stride(0) == 1089
    starts = _rows(b['starts'])
    want_record = mine.reshape(E * T, 64)
    for key, spec in _specs().items():
        want = RCM.recall(orec, ofirst, olen, b['starts'], b['init'], episode, step, spec, goal=targets, L=CAP)
        assert want['valid'].all()
        want['record'] = want_record
        got = G.recall(rec, first, length, starts, init, episode, step, spec, goal=odd if key == 'odd_goal' else goal,
                       outputs=ALL)
        assert list(got)[:4] == list(ALL) and tuple(got['obs'].shape) == spec.shape(E * T)
        _same(got, want, f'{name} {key}')
        # the views of the record are the log's fields
        assert torch.equal(got['action'].cpu(), torch.from_numpy(RCC.cases()[name]['actions'].T.reshape(-1).copy()))
        assert np.array_equal(got['agent_pos'].cpu().numpy(), b['pos'].reshape(-1, 5))
        del got, want


# ---- 2. what the physics never writes, against the model --------------------------------------------------------------------
def _hand_written(seed=3, n_rec=1000, L=300):
    rng = np.random.RandomState(seed)
    cells = np.array([y * 121 + x * 11 + z for y in (0, 1) for x in range(3, 8) for z in range(3, 8)])
    word = np.where(rng.uniform(size=n_rec) < 0.5, rng.choice(cells, n_rec) | rng.randint(0, 7, n_rec) << 11, 0xffff)
    odd = rng.uniform(size=n_rec)
    word = np.where(odd < 0.03, rng.randint(1089, 2048, n_rec) | rng.randint(0, 8, n_rec) << 11, word)   # cells >= 1089
    word = np.where((odd >= 0.03) & (odd < 0.06), rng.choice(cells, n_rec) | 7 << 11, word)              # colour 7
    again = np.flatnonzero((odd >= 0.06) & (odd < 0.46))                   # the same cell on consecutive steps
    again = again[again > 0]
    word[again] = (word[again - 1] & 0x7ff) | rng.randint(0, 7, len(again)) << 11
    word[again] = np.where(word[again - 1] == 0xffff, 0xffff, word[again])
    rec = rng.randint(0, 256, (n_rec, 64)).astype(np.uint8)        # every other field of a record is noise
    rec[:, 40:42] = word.astype(np.uint16).view(np.uint8).reshape(-1, 2)
    # poses: on and around the grid, half-integers, heads outside in x, y and z, yaws at and around the quadrant bounds
    pos = np.stack([rng.choice([-7.5, -5.5, -5.0, -2.5, -0.5, 0.0, 0.5, 1.5, 3.25, 5.0, 5.5, 6.0, 40.0], n_rec),
                    rng.choice([-3.0, -1.0, 0.0, 0.5, 1.0, 2.5, 7.0, 8.0, 9.0], n_rec),
                    rng.choice([-6.0, -5.5, -4.5, -1.0, 0.0, 0.5, 2.5, 4.5, 5.0, 5.5, 7.0], n_rec),
                    rng.uniform(-90, 90, n_rec),
                    rng.choice([-405.0, -135.0, -45.0, -44.99, 0.0, 44.99, 45.0, 90.0, 134.9, 135.0, 180.0, 225.0, 270.0,
                                315.0, 359.0, 720.0], n_rec)], 1).astype(np.float32)
    rec[:, 0:20] = pos.view(np.uint8).reshape(-1, 20)
    #                 whole   1   0   L-1  chunk+1 chunk  64  65  63  clamped  <0  aliases ....  out of the buffer ....
    first = np.array([0,     5,  9,  700, 100,   100,  300, 300, 300, 650,  20,  0,   1,  700, 701, 999, 1000, -1, 1 << 40])
    length = np.array([300,  1,  0,  299, 257,   256,  64,  65,  63,  400,  -3,  300, 300, 300, 300, 1,   1,    5,  5], np.int32)
    e = len(first)
    starts = np.zeros((e, ROW), np.int8)
    goals = np.zeros((e + 2, 1089), np.int8)
    for i in range(e):
        starts[i, rng.choice(cells, 8, replace=False)] = rng.choice([1, 2, 3, 4, 5, 6, 7, -1, 100], 8)   # (7, -1, 100 read as 0)
        starts[i, 1089:] = rng.randint(-128, 128, 15)                                                   # (pad bytes are noise)
    for i in range(e + 2):
        goals[i, rng.choice(cells, 12, replace=False)] = rng.choice([1, 2, 3, 4, 5, 6, 7, -3], 12)
    init = np.stack([rng.choice([-5.5, 0.0, 0.5, 2.5, 6.0], e), rng.choice([0.0, 1.0, 8.0], e),
                     rng.choice([-4.5, 0.0, 1.5, 7.0], e), rng.choice([0.0, 90.0, 180.0, 270.0, -45.0], e),
                     rng.uniform(-90, 90, e)], 1)
    return rec, first, length, starts, init, goals, L


def _hand_samples(first, length, L, n_goals, k):
    """Per episode: the steps at its ends, at the 64- and 256-record boundaries and around the stack's reach, one beyond
    each end; then every padding cause, duplicates included."""
    episode, step, index = [], [], []
    for e in range(len(first)):
        n = int(np.clip(length[e], 0, L))
        for t in sorted({0, 1, 2, k - 1, k, k + 1, 63, 64, 65, 66, 255, 256, 257, 258, n - 1, n, n + 1}):
            episode.append(e), step.append(t), index.append((e * 7 + t) % n_goals)
    for e, t, g in ((-1, 1, 0), (len(first), 1, 0), (1 << 30, 1, 0), (0, -5, 0), (0, 1 << 30, 0), (0, 1, -1), (0, 1, n_goals),
                    (0, 1, 1 << 40), (0, 300, 0), (0, 300, 0), (3, 299, 1), (0, 300, 0)):
        episode.append(e), step.append(t), index.append(g)
    return np.array(episode, np.int32), np.array(step, np.int32), np.array(index, np.int64)


@pytest.mark.parametrize('key', ['world_u8', 'ego5_f16', 'ego1_bf16'])
def test_hand_written_records_equal_the_model(key):
    """Lengths 0, 1, L and beyond, t at the 64- and 256-record boundaries, changes to cells >= 1089, colour 7, the same cell
    on consecutive steps, starting cells outside 0..6, goal values outside 1..6, aliased `first`, heads outside the grid,
    half-integer poses, every padding cause (zeros and `bias` written, valid 0), duplicated samples."""
    import gridworld_amd as G
    rec, first, length, starts, init, goals, L = _hand_written()
    spec = _specs()[key]
    episode, step, index = _hand_samples(first, length, L, len(goals), spec.stack)
    want = RCM.recall(rec, first, length, starts, init, episode, step, spec, goal=goals, goal_index=index, L=L)
    got = G.recall(torch.from_numpy(rec).to(DEV), first, length, torch.from_numpy(starts).to(DEV), init, episode, step, spec,
                   goal=torch.from_numpy(goals).to(DEV), goal_index=index, outputs=ALL, pad=L)
    _same(got, want, key)
    ok = want['valid'] == 1
    assert int(ok.sum()) >= 100 and int((~ok).sum()) >= 40
    pad_value, bad = VM.convert(torch.zeros(1, dtype=torch.uint8), spec), torch.from_numpy(~ok)
    assert bool((VM.bits(got['obs'].cpu()[bad]) == VM.bits(pad_value)).all()) and not got['record'].cpu().numpy()[~ok].any()
    assert bool((VM.bits(got['next_obs'].cpu()[bad]) == VM.bits(pad_value)).all())
    # what the samples reach, counted on the inputs alone
    n = np.clip(length, 0, L)
    pos = np.ascontiguousarray(rec[:, :20]).view(np.float32)
    outside = half = twice = 0
    for e, t in zip(episode[ok], step[ok]):
        p = pos[first[e] + t - 1]
        outside += bool(abs(np.rint(p[0])) > 5 or abs(np.rint(p[2])) > 5 or not 0 <= np.rint(p[1]) + 1 <= 8)
        half += bool(p[0] % 1 == 0.5 or p[2] % 1 == 0.5)
        w = RCM.words_of_records(rec[first[e] + max(0, t - spec.stack):first[e] + t]).astype(np.int64)
        w = w[(w != 0xffff) & ((w & 0x7ff) < 1089)] & 0x7ff
        twice += len(w) != len(set(w.tolist()))
    print(f'{key}: {int(ok.sum())} valid samples, head outside the grid {outside}, half-integer {half}, '
          f'a cell changed twice in the window {twice}')
    assert outside >= 20 and half >= 20 and (twice >= 20 or spec.stack == 1)
    assert {64, 65, 256, 257} <= set(step[ok & (episode == 0)].tolist()) and n[0] == 300
    # B = 1, and a duplicated sample is the same sample
    i = int(np.flatnonzero(ok & (step == 257))[0])
    one = G.recall(torch.from_numpy(rec).to(DEV), first, length, torch.from_numpy(starts).to(DEV), init, episode[i:i + 1],
                   step[i:i + 1], spec, goal=torch.from_numpy(goals).to(DEV), goal_index=index[i:i + 1], outputs=ALL, pad=L)
    for k in ALL:
        assert torch.equal(one[k], got[k][i:i + 1]), k
    assert torch.equal(got['obs'][-1], got['obs'][-3]) and torch.equal(got['next_obs'][-1], got['next_obs'][-4])


def test_no_sample_writes_nothing():
    from gridworld_amd import recall as R
    rec, first, length, starts, init, goals, L = _hand_written()
    spec, s = R.spec_of(_specs()['world_u8'])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    t = dict(rec=dev(rec), first=dev(first.astype(np.int64)), length=dev(length), starts=dev(starts), init=dev(init),
             episode=dev(np.zeros(4, np.int32)), step=dev(np.ones(4, np.int32)), goal=dev(goals))
    outs = [torch.full((4096,), 0x55, dtype=torch.uint8, device=DEV) for _ in range(4)]
    stream = torch.cuda.current_stream(DEV).cuda_stream
    R.recall_into(t['rec'].data_ptr(), len(rec), t['first'].data_ptr(), t['length'].data_ptr(), t['starts'].data_ptr(),
                  t['init'].data_ptr(), len(first), L, t['episode'].data_ptr(), t['step'].data_ptr(), 0, t['goal'].data_ptr(),
                  1089, len(goals), None, s, [o.data_ptr() for o in outs], stream)
    torch.cuda.synchronize()
    assert all(bool((o == 0x55).all()) for o in outs)
    import gridworld_amd as G
    none = G.recall(t['rec'], t['first'], t['length'], t['starts'], t['init'], t['episode'][:0], t['step'][:0], spec,
                    goal=t['goal'], outputs=ALL)
    assert tuple(none['obs'].shape) == spec.shape(0) and tuple(none['record'].shape) == (0, 64) and 'action' in none


# ---- 3. output rows at every residue mod 16 ------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.uint8, torch.float16, torch.bfloat16, torch.float32])
def test_misaligned_rows_and_canaries(dtype, logs):
    """B = 5 (one of them padding), one occupancy plane and the agent, ego R = 1, stack 2: a slot is 162 elements and a
    sample's run 324, so the slots start at many residues mod 16; the output itself starts at every element offset of a
    16-byte piece.  obs, next_obs, record and valid each sit between canaries."""
    import gridworld_amd as G
    env, rec, heads, first, length = logs('towers')
    b, orec, ofirst, olen = _oracle_log('towers')
    spec = _spec(planes=(('grid', 'occ'),), agent=True, frame='ego', radius=1, dtype=dtype, stack=2,
                 **({} if dtype is torch.uint8 else dict(scale=0.5, bias=-0.25)))
    episode, step = np.array([3, 9, 40, 17, 31], np.int32), np.array([1, 2, 5, 30, 48], np.int32)
    want = RCM.recall(orec, ofirst, olen, b['starts'], b['init'], episode, step, spec, L=CAP)
    assert want['valid'].tolist() == [1, 1, 0, 1, 1]
    count = int(np.prod(spec.shape(5)))
    assert count == 5 * 324
    starts, init = _rows(b['starts']), torch.from_numpy(b['init'].copy()).to(DEV)
    slot = ((first // CAP) % 2).cpu().numpy()
    want['record'] = np.where(want['valid'][:, None] == 1,
                              rec.cpu().numpy()[np.clip(episode, 0, E - 1), slot[np.clip(episode, 0, E - 1)], step - 1],
                              0).astype(np.uint8)
    pad, size = 64, torch.empty((), dtype=dtype).element_size()
    for offset in range(16 // size):
        bufs = [torch.full((pad + offset + count + pad,), 7, dtype=dtype, device=DEV) for _ in range(2)]
        small = [torch.full((pad + 4 * offset + n + pad,), 7, dtype=torch.uint8, device=DEV) for n in (5 * 64, 5)]
        out = {'obs': bufs[0][pad + offset:pad + offset + count].view(spec.shape(5)),
               'next_obs': bufs[1][pad + offset:pad + offset + count].view(spec.shape(5)),
               'record': small[0][pad + 4 * offset:pad + 4 * offset + 320].view(5, 64),
               'valid': small[1][pad + 4 * offset:pad + 4 * offset + 5]}
        assert out['obs'].data_ptr() % 16 == (offset * size) % 16
        got = G.recall(rec, first, length, starts, init, episode, step, spec, outputs=ALL, out=out)
        assert all(got[k] is out[k] for k in ALL)
        _same(got, want, f'{dtype} offset {offset}')
        for buf, lo, n in ((bufs[0], pad + offset, count), (bufs[1], pad + offset, count),
                           (small[0], pad + 4 * offset, 320), (small[1], pad + 4 * offset, 5)):
            assert bool((buf[:lo] == 7).all()) and bool((buf[lo + n:] == 7).all()), (dtype, offset)


# ---- 4. against the live stack -------------------------------------------------------------------------------------------------
def test_next_obs_is_what_the_live_vox_obs_stack_showed():
    """An env with vox_obs=spec (K = 3, ego) and the log on: obs['vox_obs'] after every step against recall's next_obs of
    that step.  A sample whose window holds an entry where rint of the float64 state and rint of its float32 rounding pick
    different head cells is left out (the query is defined on the log's values); counted, reported, at most 1 %."""
    import gridworld_amd as G
    from gridworld_amd import VecGridWorld
    spec = _spec(planes=(('grid', 'onehot'), ('target', 'onehot')), agent=True, frame='ego', radius=3, dtype=torch.uint8,
                 stack=3)
    left_out = compared = 0
    episode, step = RCC.pairs()
    for name, case in RCC.cases().items():
        b = RCC.base(name)
        env = VecGridWorld(E, vox_obs=spec, **case['kw'])
        env.set_tasks(case['targets'], case['starts'], init_pose=case['poses'])
        rec, heads = env.enable_trajectory_log(E, CAP)
        env.reset()
        acts = torch.from_numpy(case['actions']).to(env.device)
        live = torch.empty((T,) + spec.shape(E), dtype=spec.dtype, device=DEV)
        for t in range(T):
            obs = env.step(acts[t])[0]
            live[t].copy_(obs['vox_obs'])
        first, length = _episodes(heads, CAP)
        got = G.recall(rec, first, length, env.task_start, env.task_meta[:E, :40].contiguous().view(torch.float64), episode,
                       step, spec, goal=(env.task_target + env.task_start)[:E], outputs=('next_obs', 'valid'))
        assert got['valid'].all()
        differs = RCC.head_differs(b)                                    # [E, T + 1]
        keep = np.ones((E, T), bool)
        for t in range(1, T + 1):
            keep[:, t - 1] = ~differs[:, max(0, t - spec.stack + 1):t + 1].any(1)
        left_out += int((~keep).sum())
        compared += int(keep.sum())
        nxt = got['next_obs'].view((E, T) + spec.shape(1)[1:]).permute(1, 0, 2, 3, 4, 5)      # [T, E, ...]
        same = (nxt == live).flatten(2).all(2).cpu().numpy().T                                # [E, T]
        assert same[keep].all(), (name, int((~same[keep]).sum()))
    print(f'live stack: {compared} samples compared, {left_out} left out (a head cell the float32 log rounds differently)')
    assert left_out <= 0.01 * (compared + left_out)


# ---- 5. with relabel -----------------------------------------------------------------------------------------------------------
def test_env_recall_with_relabelled_goals_eager_and_captured():
    """env.relabel(entries, outputs=('reward', 'done', 'target')) -> env.recall(goals=r, goal=g): the `target` planes show
    the oracle's grid at the goal's entry, reward_relabel / done_relabel are the oracle's stepped under that goal; the same
    call captured in a graph, with out=, gives the same bits, and the stateless launch with out= allocates nothing."""
    import gridworld_amd as G
    name = 'towers'
    case = dict(RCC.cases()[name])
    case['kw'] = dict(case['kw'], max_steps=T)
    env, rec, heads = _logged(case)
    b, orec, ofirst, olen = _oracle_log(name)
    fixed = [RC.AT[k] for k in ('final', 'at24', 'at5', 'at0')]
    cols = [RC.GOALS.index(k) for k in ('final', 'at24', 'at5', 'at0')]
    length = torch.full((E,), T, dtype=torch.int32, device=DEV)
    at = torch.cat([torch.tensor([fixed] * E, dtype=torch.int32, device=DEV), G.relabel_future(length, 2, seed=9)], 1)
    r = env.relabel(at, outputs=('reward', 'done', 'target'))
    assert r['valid'].all() and (r['length'] == T).all()
    n_g = at.shape[1]
    episode, step = RCC.pairs()
    g = (episode + step) % n_g
    spec = _spec(planes=(('grid', 'onehot'), ('target', 'onehot')), agent=True, dtype=torch.float16, stack=2)
    ep_d, st_d, g_d = (torch.from_numpy(x).to(DEV) for x in (episode, step, g.astype(np.int64)))
    m = env.recall(spec, episode=ep_d, step=st_d, goals=r, goal=g_d)
    at_np = at.cpu().numpy()
    goal_rows = np.stack([[b['grids'][at_np[e, k], e] for k in range(n_g)] for e in range(E)]).reshape(E * n_g, 1089)
    want = RCM.recall(orec, ofirst, olen, b['starts'], b['init'], episode, step, spec, goal=goal_rows,
                      goal_index=episode.astype(np.int64) * n_g + g, L=CAP)
    _same(m, {k: want[k] for k in ('obs', 'next_obs', 'valid')}, 'relabelled')
    assert m['valid'].all() and torch.equal(m['episode'], ep_d) and torch.equal(m['step'], st_d)
    truth = RC.truth(name, max_steps=T)
    rw, dn = m['reward_relabel'].contiguous().cpu().numpy(), m['done_relabel'].contiguous().cpu().numpy()
    for k, col in enumerate(cols):
        pick = g == k
        assert np.array_equal(rw[pick].view(np.uint32), truth['reward'][episode[pick], col, step[pick] - 1].view(np.uint32)), k
        assert np.array_equal(dn[pick], truth['done'][episode[pick], col, step[pick] - 1]), k
    all_r = r['reward'].cpu().numpy()
    assert np.array_equal(rw.view(np.uint32), all_r[episode, g, step - 1].view(np.uint32))
    # the logged reward and done are the record's
    own = env.recall(spec, episode=ep_d, step=st_d, goals='own', outputs=('record', 'next_obs'))
    assert np.array_equal(own['reward'].contiguous().cpu().numpy().view(np.uint32),
                          RC.truth(name, max_steps=T)['reward'][episode, RC.GOALS.index('own'), step - 1].view(np.uint32))
    assert int(own['done'].sum()) >= E
    want_own = RCM.recall(orec, ofirst, olen, b['starts'], b['init'], episode, step, spec,
                          goal=case['targets'].reshape(E, -1).astype(np.int8), L=CAP)
    _same(own, {'next_obs': want_own['next_obs']}, 'own')
    # captured, with out=: the same bits
    out = {k: torch.zeros_like(m[k]) for k in ALL}
    env.recall(spec, episode=ep_d, step=st_d, goals=r, goal=g_d, out=out)           # warm
    for t in out.values():
        t.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = env.recall(spec, episode=ep_d, step=st_d, goals=r, goal=g_d, out=out)
    graph.replay()
    torch.cuda.synchronize()
    for k in ALL:
        assert res[k] is out[k] and torch.equal(res[k], m[k]), k
    assert torch.equal(res['reward_relabel'], m['reward_relabel']) and torch.equal(res['done_relabel'], m['done_relabel'])
    # the stateless launch with every output given allocates nothing
    first, ln = _episodes(heads, CAP)
    starts, init = env.task_start, env.task_meta[:E, :40].contiguous().view(torch.float64)
    index = ep_d.long() * n_g + g_d
    for t in out.values():
        t.zero_()
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated(DEV)
    again = G.recall(rec, first, ln, starts, init, ep_d, st_d, spec, goal=r['target'], goal_index=index, outputs=ALL, out=out)
    assert torch.cuda.memory_allocated(DEV) == held
    torch.cuda.synchronize()
    for k in ALL:
        assert again[k] is out[k] and torch.equal(again[k], m[k]), k


# ---- 6. the other surfaces -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('space', ['flying', 'walking_dict'])
def test_a_flying_and_a_walking_dict_log_answer(space):
    """The record is a verbatim copy of the log's row, its views are the actions that were passed, and the planes are the
    model's on the log's own records."""
    from gridworld_amd import VecGridWorld, workloads
    n, steps = 32, 30
    kw = dict(size_reward=False, max_steps=steps, **(dict(action_space='flying') if space == 'flying' else dict(discretize=False)))
    targets = workloads.rt20(n, seed=15).numpy().astype(np.int8)
    env = VecGridWorld(n, **kw)
    env.set_tasks(targets)
    rec, heads = env.enable_trajectory_log(n)
    env.reset()
    rng = np.random.RandomState(15)
    cams, moves, buttons = [], [], []
    for t in range(steps):
        cam = rng.uniform(-5, 5, (n, 2)).astype(np.float32)
        cam[:, 1] = np.where(t < 8, -5.0, cam[:, 1])   # (look down first: something to build on)
        cams.append(cam)
        if space == 'flying':
            mv = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
            moves.append(mv)
            env.step(dict(movement=mv, camera=cam, inventory=rng.randint(0, 7, n).astype(np.int32),
                          placement=rng.choice([0, 1, 1, 2], n).astype(np.int32)))
        else:
            bt = (rng.rand(n, 8) < 0.3).astype(np.uint8)
            bt[:, 7] = rng.randint(0, 7, size=n) * (rng.rand(n) < 0.3)
            buttons.append(bt)
            env.step(dict(buttons=bt, camera=cam))
    spec = _spec(planes=(('grid', 'onehot'), ('target', 'occ')), agent=True, frame='ego', radius=4, dtype=torch.bfloat16,
                 scale=2.0, bias=-1.0, stack=3)
    e, t = np.meshgrid(np.arange(n), np.arange(1, steps + 1), indexing='ij')
    episode, step = e.reshape(-1).astype(np.int32), t.reshape(-1).astype(np.int32)
    got = env.recall(spec, episode=episode, step=step, goals='own')
    assert got['valid'].all()
    first, length = _episodes(heads, steps)             # (the log's capacity is max_steps)
    assert (length == steps).all()
    log = rec.cpu().numpy().reshape(-1, 64)
    f = first.cpu().numpy()
    want = RCM.recall(log, f, np.full(n, steps), np.zeros((n, 1089), np.int8),
                      env.task_meta[:n, :40].contiguous().view(torch.float64).cpu().numpy(), episode, step, spec,
                      goal=targets.reshape(n, -1), L=steps)
    _same(got, want, space)
    changed = int((RCM.words_of_records(log[(f[:, None] + np.arange(steps)).reshape(-1)]) != 0xffff).sum())
    print(f'{space}: {changed} logged steps changed a cell')
    assert changed >= 32
    cam = np.stack(cams, 1).reshape(-1, 2)                                  # [n * steps, 2] in sample order
    assert np.array_equal(got['camera'].cpu().numpy(), cam) and 'action' not in got
    if space == 'flying':
        assert np.array_equal(got['movement'].cpu().numpy(), np.stack(moves, 1).reshape(-1, 3))
    else:
        assert np.array_equal(got['buttons'].cpu().numpy(), np.stack(buttons, 1).reshape(-1, 8))


def test_sub_batches_the_sampler_and_an_untouched_env():
    import gridworld_amd as G
    case = dict(RCC.cases()['looking_down'])
    case['kw'] = dict(case['kw'], max_steps=T)
    env, rec, heads = _logged(case)
    spec = _spec(planes=(('grid', 'onehot'), ('target', 'occ')), agent=True, frame='ego', radius=2, dtype=torch.float16, stack=4)
    before, stats, log = env.state_dict(), env.stats_tensor().clone(), (rec.clone(), heads.clone())
    # the seeded sampler: deterministic, in range, every sample valid once every env has finished an episode
    a = env.recall(spec, batch=512, seed=11, goals='own')
    again = env.recall(spec, batch=512, seed=11, goals='own')
    other = env.recall(spec, batch=512, seed=12, goals='own')
    assert a['valid'].all() and a['valid'].dtype == torch.uint8 and tuple(a['obs'].shape) == spec.shape(512)
    assert a['episode'].dtype == a['step'].dtype == torch.int32
    assert int(a['episode'].min()) >= 0 and int(a['episode'].max()) < E and int(a['step'].min()) >= 1 and int(a['step'].max()) <= T
    assert len(set(a['episode'].tolist())) == E and len(set(a['step'].tolist())) >= 40
    for k in a:
        assert torch.equal(a[k], again[k]), k
    assert not torch.equal(a['episode'], other['episode'])
    whole = env.recall(spec, episode=a['episode'], step=a['step'], goals='own')
    for k in ('obs', 'next_obs', 'record', 'valid'):
        assert torch.equal(whole[k], a[k]), k
    torch.cuda.synchronize()
    # nothing moved
    after = env.state_dict()
    for k, v in before.items():
        assert torch.equal(v, after[k]) if torch.is_tensor(v) else v == after[k], k
    assert torch.equal(stats, env.stats_tensor()) and torch.equal(rec, log[0]) and torch.equal(heads, log[1])
    # sub-batches: the range's own logged envs, numbered from its first
    h = E // 2
    ep, st = a['episode'], a['step']
    for k, s in enumerate(env.split(2)):
        mine = (ep >= k * h) & (ep < (k + 1) * h)
        ep_k, st_k = ep[mine] - k * h, st[mine]
        torch.cuda.synchronize()                      # (the sub-batch launches on a stream of its own)
        part = s.recall(spec, episode=ep_k, step=st_k, goals='own')
        s.synchronize()
        assert part['valid'].all()
        for key in ('obs', 'next_obs', 'record'):
            assert torch.equal(part[key], a[key][mine]), (k, key)
    # an env that has not finished an episode yields padding
    young, _, _ = _logged(case, n=8, steps=10)
    none = young.recall(spec, batch=64, seed=1, goals='own')
    assert not none['valid'].any() and not none['record'].any() and (none['step'] == 1).all()
    assert bool((none['obs'] == 0).all()) and bool((none['next_obs'] == 0).all())
    biased = young.recall(_spec(planes=(('grid', 'occ'),), dtype=torch.float32, scale=2.0, bias=0.75), batch=8)
    assert bool((biased['obs'] == 0.75).all()) and bool((biased['next_obs'] == 0.75).all()) and not biased['valid'].any()
    assert G.vox_channel_names(spec) == ['grid:%d' % k for k in range(1, 7)] + ['target', 'agent']


def test_the_value_errors_are_raised():
    import gridworld_amd as G
    case = dict(RCC.cases()['looking_down'])
    case['kw'] = dict(case['kw'], max_steps=4)
    env, rec, heads = _logged(case, n=8, steps=4)
    grid = _spec(planes=(('grid', 'occ'),))
    ok = env.recall(grid, batch=16)
    assert ok['valid'].all() and tuple(ok['obs'].shape) == (16, 2, 9, 11, 11)
    for outputs in ((), ('gain',), ('obs', 'word'), 'observations'):
        with pytest.raises(ValueError):
            env.recall(grid, batch=4, outputs=outputs)
    for spec in (_spec(planes=(('want', 'occ'),)), _spec(planes=(('grid', 'occ'), ('todo', 'onehot'))), 'world', None):
        with pytest.raises(ValueError):
            env.recall(spec, batch=4)
    with pytest.raises(ValueError, match="'target' plane"):
        env.recall(_spec(), batch=4)
    r = env.relabel('final', outputs=('reward', 'target'))
    for kw in (dict(), dict(batch=-1), dict(episode=[0, 1]), dict(step=[1, 1]), dict(episode=[0, 1], step=[1]),
               dict(episode=[0.5], step=[1]), dict(episode=[[0]], step=[[1]]), dict(batch=4, goals='final'),
               dict(batch=4, goals={'reward': r['reward']}), dict(batch=4, goal=[0] * 4), dict(batch=4, goals='own', goal=[0] * 4),
               dict(batch=4, goals=r, goal=[0] * 3), dict(batch=4, goals=r, goal=[0.0] * 4),
               dict(batch=4, goals=dict(r, target=r['target'][:4])), dict(batch=4, goals=dict(r, reward=r['reward'][:, :, :2].contiguous()[:4])),
               dict(batch=4, out={'obs': torch.zeros((4, 2, 9, 11, 12), dtype=torch.uint8, device=DEV)}),
               dict(batch=4, out={'obs': torch.zeros((4, 2, 9, 11, 11), dtype=torch.float16, device=DEV)}),
               dict(batch=4, outputs=('obs',), out={'valid': torch.zeros(4, dtype=torch.uint8, device=DEV)})):
        with pytest.raises(ValueError):
            env.recall(grid, **kw)
    good = env.recall(_spec(), episode=[0, 7, 8, 3], step=[1, 4, 1, 5], goals=r, goal=[0, 0, 0, 1])
    assert good['valid'].tolist() == [1, 1, 0, 0] and good['reward_relabel'].tolist()[2:] == [0.0, 0.0]
    parts = env.split(2)
    env.disable_trajectory_log()
    with pytest.raises(ValueError, match='episode log'):
        env.recall(grid, batch=4)
    env.enable_trajectory_log(2)
    with pytest.raises(ValueError, match='logged'):
        parts[1].recall(grid, batch=4)            # envs 4..7: the log holds the first two
    assert not parts[0].recall(grid, batch=4)['valid'].any()
    with pytest.raises(ValueError, match='device tensor'):
        G.recall(rec.cpu(), [0], [1], np.zeros((1, 1089), np.int8), np.zeros((1, 5)), [0], [1], grid)
