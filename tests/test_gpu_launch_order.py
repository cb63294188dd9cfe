"""The launch sequence of the batched env's host layer (gridworld_amd/vec_env.py): which library entries reset / step /
step_walking_ptr / rollout / rollout_actions / capture_steps call, in which order, with whose context, stream and
pointers.  The four loaded libraries are wrapped in a recorder that notes the entry's name and calls through, so the
outputs are the real ones; the outputs themselves are pinned elsewhere (tests/test_gpu_api.py, test_gpu_render_obs.py,
test_gpu_action_mask.py).  What this file pins is what those cannot see: a draw issued twice, a mask in front of the
draw, a step that converts a tensor it could have passed on.

The batch: 6 envs (3 per chain with chains=2), 8 x 8 frames, T = 3 captured steps, max_steps=2 with auto-reset, so an
episode ends inside the three steps."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, T, SIZE, CHAINS = 6, 3, (8, 8), 2
STEP = {'walking': 'igw_step_walking', 'flying': 'igw_step_flying', 'dict': 'igw_step_walking_dict'}
LAUNCHES = {'igw_reset', *STEP.values(), 'igw_rollout_walking', 'igw_rollout_walking_actions',
            'igw_rollout_flying_actions', 'igw_render_pov', 'igw_render_pov_aux', 'igw_render_pov_obs',
            'igw_action_mask'}
MASK = 'igw_action_mask'
# what follows the state: name -> (constructor arguments, the entry that draws or None, action mask, frames stacked)
FOLLOWERS = {
    'none': ({}, None, False, 1),
    'pov': (dict(renderer='hip'), 'igw_render_pov', False, 1),
    'planes': (dict(renderer='hip', pov_outputs=('rgb', 'depth')), 'igw_render_pov_aux', False, 1),
    'obs1': (dict(renderer='hip', pov_obs=dict(stack=1)), 'igw_render_pov_obs', False, 1),
    'obs2': (dict(renderer='hip', pov_obs=dict(stack=2)), 'igw_render_pov_obs', False, 2),
    'mask': (dict(action_mask=True), None, True, 1),
    'pov+mask': (dict(renderer='hip', action_mask=True), 'igw_render_pov', True, 1),
    'obs2+mask': (dict(renderer='hip', pov_obs=dict(stack=2), action_mask=True), 'igw_render_pov_obs', True, 2),
}


class Recorder:
    """Stands in front of a loaded library: every entry notes (name, arguments) in `calls`, then calls through."""

    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def entry(*args):
            self._calls.append((name, args))
            return fn(*args)
        return entry


class Calls:
    def __init__(self, monkeypatch):
        from gridworld_amd import query as Q, render as R
        self.monkeypatch, self.calls = monkeypatch, []
        for binding in (R.BINDING, R.OBS_BINDING, Q.BINDING):
            monkeypatch.setattr(binding, 'lib', Recorder(binding.load(), self.calls))

    def watch(self, env):
        self.monkeypatch.setattr(env, 'lib', Recorder(env.lib, self.calls))
        return env

    def take(self):
        """The launches since the last take(), [(name, arguments)]; what is not a launch (contexts made and bound,
        sampler settings, error texts) is left out."""
        got = [c for c in self.calls if c[0] in LAUNCHES]
        del self.calls[:]
        return got

    def names(self):
        return [name for name, _ in self.take()]


@pytest.fixture
def rec(monkeypatch):
    return Calls(monkeypatch)


def _raw(x):
    """An argument as the integer the library receives: pointers and streams go as ints or as c_void_p."""
    return getattr(x, 'value', x)


def _env(rec, space='walking', **kw):
    from gridworld_amd import VecGridWorld, workloads
    how = dict(action_space='flying') if space == 'flying' else dict(discretize=False) if space == 'dict' else {}
    env = VecGridWorld(N, autoreset=True, max_steps=2, size_reward=False, render_size=SIZE, **how, **kw)
    env.set_tasks(workloads.rt20(N, seed=5).to(env.device))
    return rec.watch(env)


def _actions(space, dev, steps=T):
    """Device tensors of the kernel's dtypes, [steps, N, ...]: a tensor for walking, a dict for the other two."""
    rng = np.random.RandomState(3)
    put = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)  # noqa: E731
    cam = put(rng.uniform(-5, 5, (steps, N, 2)), torch.float32)
    if space == 'walking':
        return put(rng.randint(0, 16, (steps, N)), torch.int32)        # (no break / place: the grid stays as reset)
    if space == 'flying':
        return dict(movement=put(rng.uniform(-1, 1, (steps, N, 3)), torch.float32), camera=cam,
                    inventory=put(rng.randint(0, 7, (steps, N)), torch.int32),
                    placement=put(rng.randint(0, 3, (steps, N)), torch.int32))
    return dict(buttons=put(rng.rand(steps, N, 8) < 0.3, torch.uint8), camera=cam)


def _after(step, draw, mask):
    return [step] + ([draw] if draw else []) + ([MASK] if mask else [])


# ---- reset / step ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(FOLLOWERS))
def test_reset_and_step_launch_the_state_move_then_the_draw_then_the_mask(rec, name):
    kw, draw, mask, _ = FOLLOWERS[name]
    env = _env(rec, **kw)
    acts = _actions('walking', env.device)
    rec.take()
    env.reset()
    assert rec.names() == _after('igw_reset', draw, mask)
    for t in range(T):
        _, _, done, _ = env.step(acts[t])
        (step, args), *rest = rec.take()
        assert [step] + [n for n, _ in rest] == _after(STEP['walking'], draw, mask)
        assert _raw(args[0]) == env.ctx.value and _raw(args[1]) == acts[t].data_ptr()    # the caller's tensor, as is
        assert bool(done.all()) == (t == 1)  # the second step ends every episode: an auto-reset, the same sequence
    env.step(acts[0].cpu().tolist())         # a converted input launches the same sequence
    assert rec.names() == _after(STEP['walking'], draw, mask)
    env.reset(torch.tensor([1, 0, 1, 0, 0, 1], dtype=torch.uint8))
    assert rec.names() == _after('igw_reset', draw, mask)
    torch.cuda.synchronize()


@pytest.mark.parametrize('space', ['flying', 'dict'])
@pytest.mark.parametrize('name', ['none', 'obs2'])
def test_dict_actions_of_the_kernel_dtypes_reach_the_step_entry_as_they_are(rec, space, name):
    kw, draw, _, _ = FOLLOWERS[name]
    env = _env(rec, space, **kw)
    acts = _actions(space, env.device)
    env.reset()
    rec.take()
    for t in range(T):
        a = {k: v[t] for k, v in acts.items()}
        env.step(a)
        (step, args), *rest = rec.take()
        assert [step] + [n for n, _ in rest] == _after(STEP[space], draw, False)
        assert _raw(args[0]) == env.ctx.value
        assert [_raw(p) for p in args[1:-1]] == [v.data_ptr() for v in a.values()]
    if space == 'dict':                      # the reference's eight keys, one array each: converted, same sequence
        b = acts['buttons'][0].cpu().numpy()
        keys = ('forward', 'back', 'left', 'right', 'jump', 'attack', 'use', 'hotbar')
        env.step(dict({k: b[:, i] for i, k in enumerate(keys)}, camera=acts['camera'][0].cpu().numpy()))
        assert rec.names() == _after(STEP[space], draw, False)
    torch.cuda.synchronize()


# ---- step_walking_ptr: the whole batch does not draw, a sub-batch does ---------------------------------------------------
@pytest.mark.parametrize('name', list(FOLLOWERS))
def test_step_walking_ptr_draws_for_a_sub_batch_only(rec, name):
    kw, draw, mask, _ = FOLLOWERS[name]
    env = _env(rec, **kw)
    acts = _actions('walking', env.device)
    env.reset()
    rec.take()
    env.step_walking_ptr(acts[0])
    assert rec.names() == _after(STEP['walking'], None, mask)
    subs = env.split(CHAINS)
    rec.take()
    for k, sub in enumerate(subs):
        a = acts[1, k * 3:(k + 1) * 3].contiguous()
        sub.step_walking_ptr(a)
        (step, args), *rest = rec.take()
        assert [step] + [n for n, _ in rest] == _after(STEP['walking'], draw, mask)
        assert _raw(args[0]) == sub.ctx.value and _raw(args[1]) == a.data_ptr()
        assert _raw(args[2]) == sub.stream.cuda_stream
        assert all(_raw(more[-1]) == sub.stream.cuda_stream for _, more in rest)
        sub.reset()
        assert rec.names() == _after('igw_reset', draw, mask)
    for sub in subs:
        sub.join()
    torch.cuda.synchronize()


# ---- fused rollouts: no draw; the next draw restarts every stack ---------------------------------------------------------
def test_rollouts_launch_the_mask_but_no_draw_and_the_next_step_restarts_every_stack(rec):
    """The restart is seen through the tensor: the frame in front of each rollout is drawn with one atlas, the step
    after it with another, and that step ends no episode (the envs run in lockstep: a rollout of 2 or 3 steps leaves
    them at the start of an episode) -- so a stack slot that still held the old frame would differ from the new one."""
    from gridworld_amd import render as R
    env = _env(rec, **FOLLOWERS['obs2+mask'][0])
    acts = _actions('walking', env.device, 4)
    other = R.default_atlas()
    other[..., :3] = 255 - other[..., :3]

    def step_fills(atlas, t):
        before = env.pov.clone()
        env.set_render_atlas(atlas)
        rec.take()
        obs, _, done, _ = env.step(acts[t])
        assert rec.names() == _after(STEP['walking'], 'igw_render_pov_obs', True)
        frame = obs['pov'].permute(0, 3, 1, 2)
        assert not bool(done.any()) and not torch.equal(obs['pov'], before)
        assert torch.equal(obs['pov_obs'][:, :3], frame) and torch.equal(obs['pov_obs'][:, 3:], frame)

    env.reset()
    rec.take()
    env.rollout(2, seed=1)
    assert rec.names() == ['igw_rollout_walking', MASK]
    step_fills(other, 0)                     # step_no 1
    env.rollout_actions(acts[1:4].contiguous())
    assert rec.names() == ['igw_rollout_walking_actions', MASK]
    step_fills(None, 0)
    # without a rollout in between the same step shifts: the slots differ again (the check above can fail)
    env.reset()
    env.set_render_atlas(other)
    obs = env.step(acts[0])[0]
    assert not torch.equal(obs['pov_obs'][:, :3], obs['pov_obs'][:, 3:])
    fly = _env(rec, 'flying')
    fly.reset()
    rec.take()
    fly.rollout_actions(_actions('flying', fly.device))
    assert rec.names() == ['igw_rollout_flying_actions']
    torch.cuda.synchronize()


# ---- capture_steps --------------------------------------------------------------------------------------------------------
def _chain_sequence(draw, mask, stacked):
    per_step = _after(STEP['walking'], draw if stacked else None, mask)
    return per_step * T + ([draw] if draw and not stacked else [])


@pytest.mark.parametrize('chains', [1, CHAINS])
@pytest.mark.parametrize('name', list(FOLLOWERS))
def test_a_capture_records_each_chain_in_order_on_its_own_context_and_stream(rec, name, chains):
    kw, draw, mask, stack = FOLLOWERS[name]
    env = _env(rec, **kw)
    acts = _actions('walking', env.device)
    env.reset()
    rec.take()
    g = env.capture_steps(acts, chains=chains)
    got = rec.take()
    want = _chain_sequence(draw, mask, stack > 1)
    assert [n for n, _ in got] == want * chains
    n = N // chains
    for k in range(chains):
        ctx = env.ctx if chains == 1 else g.subs[k].ctx
        steps = [a for name, a in got[k * len(want):(k + 1) * len(want)] if name == STEP['walking']]
        for t, args in enumerate(steps):
            assert _raw(args[0]) == ctx.value and _raw(args[1]) == acts[t, k * n:].data_ptr()
        for _, args in got[k * len(want):(k + 1) * len(want)]:
            assert _raw(args[-1]) == g.streams[k].cuda_stream
    g.replay()
    assert rec.take() == []                  # a replay launches the graph: no entry is called
    torch.cuda.synchronize()


@pytest.mark.parametrize('space', list(STEP))
def test_the_chains_of_a_capture_read_their_rows_of_every_action_buffer(rec, space):
    env = _env(rec, space)
    acts = _actions(space, env.device)
    env.reset()
    rec.take()
    g = env.capture_steps(acts, chains=CHAINS)
    got = rec.take()
    assert [n for n, _ in got] == [STEP[space]] * (T * CHAINS)
    buffers = list(acts.values()) if isinstance(acts, dict) else [acts]
    assert [b.data_ptr() for b in g.buffers] == [b.data_ptr() for b in buffers]
    for t in range(T):
        first, second = got[t][1], got[T + t][1]
        assert _raw(first[0]) == g.subs[0].ctx.value and _raw(second[0]) == g.subs[1].ctx.value
        for i, b in enumerate(buffers):
            row_bytes = b.element_size() * int(np.prod(b.shape[2:], dtype=np.int64))
            assert _raw(first[1 + i]) == b[t].data_ptr()
            assert _raw(second[1 + i]) - _raw(first[1 + i]) == (N // CHAINS) * row_bytes
    g.replay()
    torch.cuda.synchronize()


@pytest.mark.parametrize('chains', [1, CHAINS])
def test_a_replay_leaves_what_the_eager_loop_leaves(rec, chains):
    kw = FOLLOWERS['obs2+mask'][0]
    eager, graphed = _env(rec, **kw), _env(rec, **kw)
    acts = _actions('walking', eager.device)
    eager.reset()
    graphed.reset()
    g = graphed.capture_steps(acts, chains=chains)
    for rep in range(2):
        for t in range(T):
            want = eager.step(acts[t])[0]
        got = g.replay()[0]
        torch.cuda.synchronize()
        for key in ('pov_obs', 'action_mask', 'pov'):
            assert got[key].dtype == want[key].dtype and torch.equal(got[key], want[key]), (rep, key)
