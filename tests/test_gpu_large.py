"""Batches whose buffers pass the 2^31 and 2^32 byte marks: what a 32-bit byte offset, signed or unsigned, would break.

Every header promises 64-bit offsets; these tests make that a tested property.  The sizes, the windows and the scenario
are tests/large_cases.py (checked on the oracle alone by tests/test_large_cases_cpu.py): 2^22 + 101 walking and 2^22 + 64
flying envs -- the 1,024-byte histogram row passes 2^32 at env 2^22, the 1,104-byte grid row before it -- and render,
observation and codec launches whose outputs pass 4 GiB.

Nothing of whole-batch size is copied to the host.  The rows around each mark, the first and the last (large_cases.
windows) are gathered on the device and compared bit for bit: the step path, the goal query with the CPU oracle; the
renderer, the observation stage and the codec with the same entry run as a small launch over copies of those rows (small
launches are pinned to their models by test_gpu_render*.py and test_gpu_jpeg.py).  Everything else is a reduction on the
device over the whole buffer: the episode clock of every env, no sentinel byte left where a frame belongs, no byte
written where none does.  A wrapped offset lands inside the allocation -- it corrupts rows instead of faulting -- so
one shows as a low row that holds a high env's result, a high row that holds nothing, or both.

Out of scope: the action mask reads only `occ` and `agent`, whose first mark lies at 11 M envs; the trajectory log and
igw_render_episodes need a 4.3 GB record buffer and a design for it.

Peak device memory is about 21 GB (two walking batches, or one and the planes).
"""
import gc
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import large_cases as LC

pytestmark = pytest.mark.gpu

SENTINEL = 7          # no byte of a frame drawn with the default atlas (render.FLAT_COLOURS, CLEAR_RGBA) has this value
GUARD = 0xA5


def _free():
    gc.collect()
    torch.cuda.empty_cache()


def _parts(n, parts=16):
    step = -(-n // parts)
    return [slice(lo, min(lo + step, n)) for lo in range(0, n, step)]


def _any(flat, pred):
    """Whether pred(x) holds anywhere in the 1-D or row-major tensor `flat`, a sixteenth at a time (no whole-size temporaries)."""
    return any(bool(pred(flat[sl]).any()) for sl in _parts(flat.shape[0]))


def _equal(a, b):
    return all(torch.equal(a[sl], b[sl]) for sl in _parts(a.shape[0]))


def _batch(mode, n):
    from gridworld_amd import VecGridWorld
    targets, starts, poses = LC.tasks()
    env = VecGridWorld(n, autoreset=True, num_tasks=LC.NUM_TASKS, action_space=mode, **LC.KW)
    env.set_tasks(targets, starts, init_pose=poses, env_task=LC.env_task(n))
    env.reset()
    assert env.cfg.lanes_per_env in (0, 4)
    return env


def _index(rows, dev):
    return torch.from_numpy(np.asarray(rows, np.int64)).to(dev)


# ---- 1. the step path ----------------------------------------------------------------------------------------------------
def _final_rows_equal_the_oracle(env, widx, w, ob):
    """Window rows at the end of a run: float64 internals, the episode record's integers, the occupancy bitmap against
    grid != 0 and the histogram against a recount."""
    from test_gpu_parity import _check_hist, _check_occ
    targets, starts, _ = LC.tasks()
    rows = LC.Gathered(env, widx)
    assert np.array_equal(rows.internals().view(np.uint64), ob.internals().view(np.uint64))
    ts, want = rows.task_state(), [e.task_state() for e in ob.envs]
    for mine, theirs in (('step_no', 'step_no'), ('prev_size', 'syn_prev_size'), ('max_int', 'syn_max_int'),
                         ('target_size', 'syn_target_size')):
        assert np.array_equal(ts[mine], np.array([s[theirs] for s in want])), mine
    assert np.array_equal(ts['inventory'], ob.inventory.astype(np.int64))
    aux = rows.aux_buf.cpu().numpy().view(np.int32)
    assert np.array_equal(aux[:, 2], w % LC.NUM_TASKS) and (aux[:, 3] == 1 + LC.T // LC.MAX_STEPS).all()
    _check_occ(rows)
    _check_hist(rows, targets[w % LC.NUM_TASKS], starts[w % LC.NUM_TASKS])


def _whole_batch_clock(env, n, done_counts):
    """Device-side reductions over every env: a hole or a clobbered row anywhere shows here, not only in the windows."""
    step_no = env.agent_buf.view(torch.int16)[:, 30]
    assert bool((step_no == LC.T - LC.MAX_STEPS).all())
    assert bool((env.episode == 1 + LC.T // LC.MAX_STEPS).all())
    assert bool((env.env_task == torch.arange(n, dtype=torch.int32, device=env.device) % LC.NUM_TASKS).all())
    assert done_counts == [n if t == LC.MAX_STEPS - 1 else 0 for t in range(LC.T)]
    assert not bool(env.done.any())
    st = env.stats()
    assert st['steps'] == n * LC.T and st['resets'] >= n and st['bad_actions'] == 0 and st['bad_poses'] == 0
    # every block in a grid row is off the inventory: a grid row that another env's result landed on breaks the sum
    for sl in _parts(n):
        blocks = (env.grid_buf[sl, :LC.L.CELLS] != 0).sum(1)
        assert torch.equal(env.inventory[sl].sum(1), (120 - blocks).to(torch.float32))


def _not_periodic(env, w):
    """Envs e and e - 2^22 play the same task with other actions: an aliasing bug that is self-consistent would make the
    agent records periodic in 2^32 / 1024 envs."""
    hi = _index(w[w >= LC.N_MARK], env.device)
    assert hi.numel() >= 64
    differ = (env.agent_buf[hi] != env.agent_buf[hi - LC.N_MARK]).any(1)
    assert differ.float().mean().item() > 0.9


@pytest.fixture(scope='module')
def walked():
    """The walking batch after the scenario's T steps, with the window rows of every step's output (gathered on the
    device as the run went) -- the batch the goal and render tests below read in place."""
    t0 = time.time()
    env = _batch('walking', LC.N_WALK)
    w = LC.step_windows(LC.N_WALK)
    widx = _index(w, env.device)
    acts = env.fill_actions(LC.T, seed=LC.WALK_SEED)
    steps, done_counts = [], []
    for t in range(LC.T):
        env.step(acts[t])
        steps.append(LC.Gathered(env, widx, state=False))
        done_counts.append(env.done.sum(dtype=torch.int64))
    torch.cuda.synchronize()
    print(f'walking: {LC.N_WALK} envs x {LC.T} steps built and stepped in {time.time() - t0:.2f} s')
    run = SimpleNamespace(env=env, w=w, widx=widx, acts=acts, steps=steps, done_counts=[int(c) for c in done_counts])
    yield run
    del run.env, run.acts, run.steps, env, acts, steps
    _free()


def test_flying_windows_equal_the_oracle_and_every_env_keeps_its_clock():
    """2^22 + 64 flying envs, a whole number of blocks (the EXACT variant), the oracle in device-trig mode: everything
    bit for bit, as in test_flying_vs_oracle_device_trig."""
    from fuzz_parity import compare
    from oracle import oracle as O
    n = LC.N_FLY
    env = _batch('flying', n)
    w = LC.step_windows(n)
    widx, every = _index(w, env.device), torch.arange(n, dtype=torch.int64, device=env.device)
    steps, done_counts = [], []
    for t in range(LC.T):
        env.step(LC.fly_actions(every, t))
        steps.append(LC.Gathered(env, widx, state=False))
        done_counts.append(env.done.sum(dtype=torch.int64))
    torch.cuda.synchronize()
    ob = LC.oracle_batch(w, action_space='flying')
    O.use_device_trig(True)
    try:
        for t in range(LC.T):
            a = LC.fly_actions(w, t)
            ob.step_flying(a['movement'], a['camera'], a['inventory'], a['placement'], autoreset=True, nthreads=8)
            compare(steps[t], ob, f'flying step {t}')
        _final_rows_equal_the_oracle(env, widx, w, ob)
    finally:
        O.use_device_trig(False)
    _whole_batch_clock(env, n, [int(c) for c in done_counts])
    _not_periodic(env, w)
    del env, steps
    _free()


def test_walking_windows_equal_the_oracle_at_every_step(walked):
    from fuzz_parity import compare
    a_np = walked.acts[:, walked.widx].cpu().numpy()
    assert np.array_equal(a_np, LC.walk_actions(walked.w))       # the stream the CPU test ran the scenario on
    ob = LC.oracle_batch(walked.w)
    for t in range(LC.T):
        ob.step_walking(a_np[t], autoreset=True, nthreads=8)
        compare(walked.steps[t], ob, f'walking step {t}')
    _final_rows_equal_the_oracle(walked.env, walked.widx, walked.w, ob)


def test_walking_every_env_keeps_its_clock(walked):
    _whole_batch_clock(walked.env, LC.N_WALK, walked.done_counts)
    _not_periodic(walked.env, walked.w)


def test_fused_rollout_equals_stepping_over_the_whole_buffers(walked):
    other = _batch('walking', LC.N_WALK)
    other.rollout_actions(walked.acts)
    torch.cuda.synchronize()
    for name in ('grid_buf', 'agent_buf', 'hist_buf', 'occ_buf'):
        assert _equal(getattr(other, name), getattr(walked.env, name)), name
    assert other.stats()['steps'] == LC.N_WALK * LC.T
    del other
    _free()


# ---- 2. the goal query -----------------------------------------------------------------------------------------------------
def test_goal_query_of_the_stepped_batch(walked):
    """want / todo are 4.6 GB each and the kernel reads every env's histogram row.  Window rows against the oracle model
    (tests/goal_cases.py: the stateless Task evaluation, nine oracle blocks for the rewards); the whole batch through
    what ties the outputs to one another and to the state."""
    import goal_cases as GC
    env, w, n = walked.env, walked.w, LC.N_WALK
    W = len(w)
    res = env.goal(want=True, todo=True, gain=True)
    got = {k: v[walked.widx].cpu().numpy() for k, v in res.items()}
    targets, starts, _ = LC.tasks()
    ob = LC.oracle_batch(w, blocks=9)
    acts = LC.walk_actions(w)
    for t in range(LC.T):
        ob.step_walking(np.tile(acts[t], 9), autoreset=True, nthreads=16)
    want = dict(align=np.zeros((W, 3), np.int8), fit=np.zeros((W, 4), np.int16),
                want=np.zeros((W, 9, 11, 11), np.int8), todo=np.zeros((W, 9, 11, 11), np.int8))
    for k, e in enumerate(w):
        r = e % LC.NUM_TASKS
        want['align'][k], want['fit'][k], want['want'][k], want['todo'][k] = GC.env_truth(
            targets[r], starts[r], ob.grid[k].reshape(9, 11, 11), ob.envs[k].task_state()['syn_max_int'])
    ob.step_walking(np.concatenate([np.zeros(W, np.int32)] + [np.full(W, p, np.int32) for p in GC.PROBES]), nthreads=16)
    want['gain'], want['ends'] = np.repeat(ob.reward[:W, None], 18, 1), np.repeat(ob.done[:W, None], 18, 1)
    for j, p in enumerate(GC.PROBES):
        want['gain'][:, p], want['ends'][:, p] = ob.reward[(j + 1) * W:(j + 2) * W], ob.done[(j + 1) * W:(j + 2) * W]
    bad = {}
    for k in want:
        a, b = np.ascontiguousarray(got[k]), want[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        bad[k] = int((a.view(np.uint32) != b.view(np.uint32)).sum()) if k == 'gain' else int((a != b).sum())
    print(f'goal: {W} window rows, {int((want["gain"] != 0).sum())} rewards not 0, live max_int > 0 in '
          f'{int((want["fit"][:, 0] > 0).sum())}; elements that differ: {bad}')
    assert (want['gain'] != 0).sum() >= W and (want['fit'][:, 0] > 0).sum() >= 8 and want['todo'].any()
    assert not any(bad.values())
    # the whole batch
    raw = {k: torch.as_strided(res[k], (n, LC.GRID_ROW), (LC.GRID_ROW, 1)) for k in ('want', 'todo')}
    for sl in _parts(n):
        t, wn = raw['todo'][sl], raw['want'][sl]
        assert not bool(((t != 0) & (t != wn)).any())             # todo is a subset of want != 0, with want's values
        assert not bool(wn[:, LC.L.CELLS:].any()) and not bool(t[:, LC.L.CELLS:].any())
    assert bool(torch.isfinite(res['gain']).all()) and int(res['ends'].max()) <= 1
    aux16 = env.aux_buf.view(torch.int16)
    assert torch.equal(res['fit'][:, 3], aux16[:, 2]) and torch.equal(res['fit'][:, 1], aux16[:, 3])
    assert torch.equal(res['fit'][:, 2], aux16[:, 1] & 0x7fff)
    assert bool(((res['align'][:, 2] >= 0) & (res['align'][:, 2] <= 3)).all())
    del res, raw
    _free()


# ---- 3. render, planes, views, observations and the codec --------------------------------------------------------------------
def _guarded(n, row, dtype, fill, dev):
    """(flat, rows): `rows` = n rows of `row` elements inside `flat`, which has a guard row before and after them; all
    of it holds `fill`."""
    flat = torch.full(((n + 2) * row,), fill, dtype=dtype, device=dev)
    return flat, flat[row:(n + 1) * row]


def _guards_untouched(flat, row, fill):
    ref = torch.full((row,), fill, dtype=flat.dtype, device=flat.device)
    return torch.equal(flat[:row].view(torch.uint8), ref.view(torch.uint8)) and \
        torch.equal(flat[-row:].view(torch.uint8), ref.view(torch.uint8))


def _state_ptrs(env, lo=0):
    return (env.agent_buf[lo:].data_ptr(), env.grid_buf[lo:].data_ptr(), env.occ_buf[lo:].data_ptr())


def _small_launch(env, idx, outputs=None):
    """The pov entry over gathered copies of the state rows `idx` (a device index tensor)."""
    from gridworld_amd import render as R
    m = int(idx.numel())
    agent, grid, occ = env.agent_buf[idx], env.grid_buf[idx], env.occ_buf[idx]
    res = R.launch('pov', (agent.data_ptr(), grid.data_ptr(), occ.data_ptr(), m), m, LC.SIZE, 3, outputs, None,
                   env._atlas(), env.device, env._stream())
    torch.cuda.synchronize()     # (the gathered copies are read by the launch)
    return res


def test_pov_frames_past_4_gib(walked):
    from gridworld_amd import render as R
    env, n = walked.env, LC.N_POV
    flat, rows = _guarded(n, LC.FRAME_ROW, torch.uint8, SENTINEL, env.device)
    out = rows.view(n, LC.SIZE[1], LC.SIZE[0], 3)
    R.launch('pov', (*_state_ptrs(env), n), n, LC.SIZE, 3, None, out, env._atlas(), env.device, env._stream())
    torch.cuda.synchronize()
    idx = _index(LC.windows(LC.FRAME_ROW, n), env.device)
    small = _small_launch(env, idx)
    assert torch.equal(out[idx], small)
    assert small.flatten(1).ne(small[:1].flatten(1)).any(1).float().mean().item() > 0.9   # the frames are not all alike
    assert _guards_untouched(flat, LC.FRAME_ROW, SENTINEL)
    assert not _any(rows, lambda x: x == SENTINEL)                 # every byte of every frame was written
    del flat, rows, out
    _free()


def test_planes_past_their_marks(walked):
    """depth (16,384 B per frame) passes 2^32 at frame 262,144, surface (8,192 B) passes 2^31; label passes no mark."""
    from gridworld_amd import render as R
    env, n, px = walked.env, LC.N_POV, LC.SIZE[0] * LC.SIZE[1]
    fills = dict(depth=(torch.float32, -1.0), label=(torch.uint8, 99), surface=(torch.int16, -2))   # values no pixel has
    flats, out = {}, {}
    for k, (dt, fill) in fills.items():
        flats[k], rows = _guarded(n, px, dt, fill, env.device)
        out[k] = rows.view(n, LC.SIZE[1], LC.SIZE[0])
    R.launch('pov', (*_state_ptrs(env), n), n, LC.SIZE, 3, tuple(fills), out, env._atlas(), env.device, env._stream())
    torch.cuda.synchronize()
    spans = [np.arange(64), np.arange(n - 64, n)] + [r for s in (LC.DEPTH_ROW, LC.SURFACE_ROW) for _, r in LC.marks_in(s, n)]
    assert len(spans) == 2 + 3
    w = np.unique(np.concatenate(spans))
    idx = _index(w, env.device)
    small = _small_launch(env, idx, tuple(fills))
    for k in fills:
        assert torch.equal(out[k][idx].view(torch.uint8), small[k].view(torch.uint8)), k
        assert _guards_untouched(flats[k], px, fills[k][1]), k
        assert not _any(flats[k][px:(n + 1) * px], lambda x, f=fills[k][1]: x == f), k
    shows_block = ((small['label'] >= 1) & (small['label'] <= 6)).flatten(1).any(1).cpu().numpy()
    for rows_ in spans:
        share = shows_block[np.searchsorted(w, rows_)].mean()
        assert share >= 0.5, (rows_[0], share)                       # the windows look at something
    del flats, out
    _free()


def test_views_read_grid_rows_past_their_marks_in_place(walked):
    import gridworld_amd as G
    env = walked.env
    w = LC.windows(LC.GRID_ROW, LC.N_WALK)
    poses = G.orbit_poses((0, 1, 0), 12, 5, len(w))
    vg = torch.from_numpy(w.astype(np.int32)).to(env.device)
    got = env.render_views(poses, rows=vg, size=LC.SIZE)
    dense = env.grid_buf[vg.long()].contiguous()
    want = G.render_views(dense, poses, size=LC.SIZE, atlas=env._atlas(), device=env.device)
    empty = G.render_views(torch.zeros_like(dense), poses, size=LC.SIZE, atlas=env._atlas(), device=env.device)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert got.flatten(1).ne(empty.flatten(1)).any(1).float().mean().item() >= 0.5    # the views show blocks


def test_observation_stacks_past_4_gib(walked):
    """f32, RGB, K = 8 at 64 x 64: 393,216 B per env, no frame beside it (the sink path on more than 2,048 blocks).  Call
    j draws envs [j n, (j + 1) n) of the batch, so that every call shifts other frames in: fill, two shifts, a restart
    mask at stride 1."""
    import obs_model as OM
    from gridworld_amd import ObsSpec
    from gridworld_amd import render as R
    env, n = walked.env, LC.N_OBS
    spec = ObsSpec(torch.float32, stack=LC.OBS_STACK, scale=1 / 255)
    row = LC.OBS_ROW // 4
    flat, rows = _guarded(n, row, torch.float32, 9.0, env.device)     # (written values lie in [0, 1])
    out = rows.view(spec.shape(n, LC.SIZE))
    w = LC.windows(LC.OBS_ROW, n)
    idx = _index(w, env.device)
    restart = (torch.arange(n, device=env.device) % 3 == 0).to(torch.uint8)
    stack, first = None, None
    for j in range(4):
        mask = restart if j == 3 else None
        got = R.launch_obs((*_state_ptrs(env, j * n), n), n, LC.SIZE, spec, out, None, mask, j == 0, env._atlas(),
                           env.device, env._stream())
        assert got is out
        frames = _small_launch(env, idx + j * n)
        first = frames if first is None else first
        stack = OM.observe(frames, stack, None if mask is None else mask[idx], spec)
        assert torch.equal(OM.bits(out[idx]), OM.bits(stack)), j
        if j == 0:
            assert not _any(rows, lambda x: x > 1.5)                # every element of every stack was written
    assert frames.flatten(1).ne(first.flatten(1)).any(1).float().mean().item() > 0.9   # the shifts moved other frames in
    assert _guards_untouched(flat, row, 9.0)
    del flat, rows, out
    _free()


def test_jpeg_slots_of_1_mib_past_4_gib():
    import gridworld_amd as G
    import jpeg_model as J
    n, stride, dev = LC.N_JPEG, LC.JPEG_STRIDE, torch.device('cuda:0')
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    frames = torch.randint(0, 256, (n, LC.SIZE[1], LC.SIZE[0], 3), dtype=torch.uint8, device=dev, generator=g)
    small, small_sizes = G.encode_jpeg(frames, 90)                  # the default stride (grown to fit noise)
    buf = torch.full((n, stride), GUARD, dtype=torch.uint8, device=dev)
    sizes = torch.full((n,), -7, dtype=torch.int32, device=dev)
    G.encode_jpeg(frames, 90, out=(buf, sizes))
    assert torch.equal(sizes, small_sizes) and int(sizes.min()) >= G.codec.HEADER_BYTES + 2
    S = small.shape[1]
    assert int(sizes.max()) <= S < stride
    used = torch.arange(S, device=dev)[None, :] < sizes[:, None]
    assert torch.equal(buf[:, :S][used], small[used])
    cols = torch.arange(stride, device=dev)[None, :]
    for sl in _parts(n, 32):
        assert not bool(((buf[sl] != GUARD) & (cols >= sizes[sl, None])).any())
    marks = [m // stride for m in LC.MARKS]
    assert marks == [2048, 4096]
    for i in (0, marks[0] - 1, marks[0], marks[1] - 1, marks[1], n - 1):   # the slots that end and begin at each mark
        s = int(sizes[i])
        assert buf[i, :s].cpu().numpy().tobytes() == J.encode(frames[i].cpu().numpy(), 90), i
    del buf, small, frames
    _free()
