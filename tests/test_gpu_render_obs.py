"""The training-layout observation (igw_render_pov_obs, obs['pov_obs']; DESIGN.md section 8, "Training-layout
observations") on the GPU.  The yardstick is the existing path: the uint8 frames render_pov() draws of the same state
(itself pinned to the f64 model by tests/test_gpu_render.py), pushed through tests/obs_model.py.  Equality is exact for
every dtype -- torch.equal on the raw bits: both sides round one f32 value per element the same way."""
import numpy as np
import pytest
import torch

import large_cases as LC
import obs_cases as OC
import obs_model as OM

pytestmark = pytest.mark.gpu
R_CHUNK, R_SINK_SLOTS = LC.CHUNK, LC.SINK_SLOTS     # pixels per block, slots of the no-frame sink (from the sources)


def _env(n=OC.N, autoreset=True, size=(64, 64), **kw):
    from gridworld_amd import VecGridWorld
    targets, poses, actions = OC.inputs(n)
    env = VecGridWorld(n, autoreset=autoreset, max_steps=OC.MAX_STEPS, render_size=size, renderer='hip', **kw)
    env.set_tasks(targets, init_pose=poses)
    return env, torch.from_numpy(actions).to(env.device)


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert torch.equal(OM.bits(got), OM.bits(want)), what


def _follow(env, actions, spec, steps, on_step=None):
    """reset() and `steps` steps of env, its obs['pov_obs'] compared with the model after each; returns the model's
    stack and the restarts per step (bool [steps, n])."""
    obs = env.reset()
    stack = OM.observe(env.render_pov(), None, None, spec)
    _same(obs['pov_obs'], stack, 'reset')
    restarts = []
    for t in range(steps):
        obs, _, done, _ = env.step(actions[t])
        assert obs['pov_obs'] is env.pov_obs
        mask = done.clone() if env.autoreset else None
        stack = OM.observe(env.render_pov(), stack, mask, spec)
        _same(obs['pov_obs'], stack, f'step {t}')
        restarts.append(done.ne(0).cpu().numpy())
        if on_step is not None:
            stack = on_step(t, stack)
    return stack, np.stack(restarts)


def test_episode_boundaries_under_autoreset():
    from gridworld_amd import ObsSpec
    spec = ObsSpec(gray=True, stack=4)
    env, actions = _env(pov_obs=spec)
    first = env.reset()['pov_obs']
    assert first.shape == (OC.N, 4, 64, 64) and first.dtype == torch.uint8 and first is env.pov_obs
    _, restarts = _follow(env, actions, spec, OC.STEPS)
    assert env.pov_obs is first                                        # the same tensor every call
    assert restarts[:, :OC.EMPTY].all()                                # the empty-target rows: done on every step
    n = int(restarts[:, OC.EMPTY:].sum())
    print(f'{n} (env, step) pairs restarted outside the {OC.EMPTY} empty-target rows (the time limit alone gives 64)')
    assert 32 <= n <= 96
    # a row that always restarts holds K copies of the current frame; the others hold distinct frames
    cur = OM.luminance(env.render_pov())
    for k in range(4):
        assert torch.equal(first[:OC.EMPTY, k], cur[:OC.EMPTY])
    assert not torch.equal(first[OC.EMPTY:, 0], first[OC.EMPTY:, 3])


def test_without_autoreset_terminal_frames_shift_in_and_a_masked_reset_fills():
    """autoreset=False: no step restarts anything (the terminal frame joins its own episode's stack); reset(mask) is
    a draw like any other whose masked rows fill -- a byte of 255 counts as set -- while the others shift."""
    from gridworld_amd import ObsSpec
    spec = ObsSpec(gray=True, stack=4)
    env, actions = _env(autoreset=False, pov_obs=spec)
    masks = {5: torch.zeros(OC.N, dtype=torch.uint8), 9: torch.zeros(OC.N, dtype=torch.uint8)}
    masks[5][0::3] = 255
    masks[9][1::3] = 1
    seen = {}

    def on_step(t, stack):
        if t + 1 not in masks:
            return stack
        m = masks[t + 1].to(env.device)
        before = env.render_pov().clone()
        obs = env.reset(m)
        frames = env.render_pov()
        unmasked = (m == 0)
        assert torch.equal(frames[unmasked], before[unmasked])       # the mask leaves the other rows' state alone
        stack = OM.observe(frames, stack, m, spec)
        _same(obs['pov_obs'], stack, f'reset(mask) after step {t + 1}')
        lum = OM.luminance(frames)
        for k in range(4):                                            # masked rows: K copies of the new episode's frame
            assert torch.equal(obs['pov_obs'][~unmasked][:, k], lum[~unmasked])
        seen[t + 1] = int((~unmasked).sum())
        return stack
    _, done = _follow(env, actions, spec, 12, on_step)
    assert seen == {5: 16, 9: 16}
    assert done[6, OC.EMPTY:].any()                                    # the time limit fell inside the run


@pytest.mark.parametrize('kw', [dict(dtype=torch.float16, scale=1 / 255),
                                dict(dtype=torch.bfloat16, stack=3, scale=2 / 255, bias=-1),
                                dict(dtype=torch.float32, gray=True, stack=2, scale=1, bias=-128),
                                dict(dtype=torch.uint8, stack=4)], ids=['rgb-f16-k1', 'rgb-bf16-k3', 'grey-f32-k2',
                                                                       'rgb-u8-k4'])
def test_dtypes_and_planes(kw):
    from gridworld_amd import ObsSpec
    spec = ObsSpec(**kw)
    env, actions = _env(8, pov_obs=spec)
    stack, restarts = _follow(env, actions, spec, 6)
    assert stack.shape == spec.shape(8, (64, 64)) and stack.dtype == spec.dtype
    assert restarts.any() and not restarts.all()


def _slices_and_sentinels(size, kw, with_frame=True):
    """N = 3, so env bases are odd multiples of the frame; `out` starts 5 elements into a sentinel-filled tensor, so no
    row of it is aligned for four pixels: heads, bodies and tails, and nothing outside the slice.  with_frame=False
    passes frame=None, so that the entry gets out = NULL and the frame's flush goes to the sink."""
    from gridworld_amd import ObsSpec
    spec = ObsSpec(**kw)
    env, actions = _env(3, size=size)
    env.reset()
    shape = spec.shape(3, size)
    numel, pad = int(np.prod(shape)), 5
    sentinel = 77
    big = torch.full((numel + 2 * pad,), sentinel, dtype=spec.dtype, device=env.device)
    aligned = torch.full((numel,), sentinel, dtype=spec.dtype, device=env.device)
    for flat, lo in ((big, pad), (aligned, 0)):
        out = flat[lo:lo + numel].view(shape)
        env.reset()
        frame = torch.empty((3, size[1], size[0], 3), dtype=torch.uint8, device=env.device) if with_frame else None
        got = env.render_pov_obs(spec, out=out, fill=True, frame=frame)
        assert got is out
        want = OM.observe(env.render_pov(), None, None, spec)
        _same(out, want, 'fill')
        if with_frame:
            assert torch.equal(frame, env.render_pov())
        env.step(actions[0])
        env.render_pov_obs(spec, out=out)
        want = OM.observe(env.render_pov(), want, None, spec)
        _same(out, want, 'shift')
        env.step(actions[1])
        mask = torch.tensor([0, 255, 0], dtype=torch.uint8, device=env.device)
        env.render_pov_obs(spec, out=out, restart=mask)
        want = OM.observe(env.render_pov(), want, mask, spec)
        _same(out, want, 'restart')
        if lo:
            edge = torch.full((pad,), sentinel, dtype=spec.dtype, device=env.device)
            assert torch.equal(OM.bits(flat[:pad]), OM.bits(edge)) and torch.equal(OM.bits(flat[-pad:]), OM.bits(edge))
    new = env.render_pov_obs(spec)                                     # no out: a new, filled tensor
    _same(new, OM.observe(env.render_pov(), None, None, spec), 'new')


TAIL_SPECS = dict(argvalues=[dict(gray=True, stack=2), dict(dtype=torch.float16, stack=2, scale=1 / 255)],
                  ids=['grey-u8-k2', 'rgb-f16-k2'])


@pytest.mark.parametrize('size', [(13, 7), (1, 1), (96, 80), (64, 64)], ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('kw', **TAIL_SPECS)
def test_shapes_that_reach_the_tail_paths(size, kw):
    _slices_and_sentinels(size, kw)


@pytest.mark.parametrize('size,with_frame', [((96, 80), False), ((65, 65), False), ((65, 65), True)],
                         ids=['96x80-no-frame', '65x65-no-frame', '65x65-frame'])
@pytest.mark.parametrize('kw', **TAIL_SPECS)
def test_several_chunks_without_a_frame_and_off_four_pixels(size, with_frame, kw):
    """Two chunks per frame.  Without a frame the second chunk's flush is aimed at sink + slot * 12288 - c0 * 3 with
    c0 = 4,096; at 65 x 65 = 4,225 pixels the planes of the stack are not aligned alike, so every pixel goes alone."""
    assert size[0] * size[1] > R_CHUNK and (size == (96, 80) or size[0] * size[1] % 4)
    _slices_and_sentinels(size, kw, with_frame)


def test_without_a_frame_blocks_share_sink_slots():
    """pov_frame=False on 2,500 envs at 64 x 64: one block per env, more blocks than the sink has slots, so blocks in
    flight flush their frames over one another's slot.  The observation does not come from there: it equals that of an
    env that draws the frame too, and the model's."""
    from gridworld_amd import ObsSpec, VecGridWorld
    n, spec = 2500, ObsSpec(gray=True, stack=4)
    assert n > R_SINK_SLOTS
    targets, poses, actions = OC.inputs()
    rows = np.arange(n) % OC.N
    poses = poses[rows].copy()
    poses[:, 3] += 5.0 * (np.arange(n) // OC.N)                     # no two envs draw the same frame
    envs = []
    for kw in (dict(), dict(pov_frame=False)):
        env = VecGridWorld(n, autoreset=True, max_steps=OC.MAX_STEPS, render_size=(64, 64), renderer='hip', pov_obs=spec,
                           **kw)
        env.set_tasks(targets[rows], init_pose=poses)
        envs.append(env)
    both, alone = envs
    acts = torch.from_numpy(np.ascontiguousarray(actions[:, rows])).to(both.device)
    a, b = both.reset(), alone.reset()
    assert 'pov' not in b and alone.pov is None
    stack = OM.observe(a['pov'], None, None, spec)
    for t in range(4):
        _same(b['pov_obs'], a['pov_obs'], f'step {t}: without a frame')
        _same(a['pov_obs'], stack, f'step {t}: the model')
        if t < 3:
            a, b = both.step(acts[t])[0], alone.step(acts[t])[0]
            stack = OM.observe(a['pov'], stack, both.done.clone(), spec)
    frames = a['pov'].flatten(1)
    assert frames[OC.N:].ne(frames[:-OC.N]).any(1).float().mean().item() > 0.9   # (the tiled rows do differ)


@pytest.mark.parametrize('K', [5, 6, 7, 8])
@pytest.mark.parametrize('kw', [dict(gray=True), dict(dtype=torch.float16, scale=1 / 255)], ids=['grey-u8', 'rgb-f16'])
def test_stack_depths_five_to_eight(K, kw):
    """The shift holds slots 1..7 in seven hand-named registers; the other tests stop at K = 4.  A fill and K + 1
    shifts without a restart (autoreset=False), so that every slot has held every position."""
    from gridworld_amd import ObsSpec
    spec = ObsSpec(stack=K, **kw)
    env, actions = _env(8, autoreset=False, pov_obs=spec)
    stack, restarts = _follow(env, actions, spec, K + 1)
    P = spec.planes
    assert stack.shape == (8, K * P, 64, 64)
    slots = stack.reshape(8, K, -1)
    for k in range(K - 1):                                             # K different frames in most rows
        assert slots[:, k].ne(slots[:, k + 1]).any(1).float().mean().item() >= 0.5, k


def test_the_frame_beside_the_observation():
    from gridworld_amd import ObsSpec
    spec = ObsSpec(torch.float16, stack=2, scale=1 / 255)
    both, actions = _env(8, pov_obs=spec)
    alone, _ = _env(8, pov_obs=dict(dtype=torch.float16, stack=2, scale=1 / 255), pov_frame=False)
    plain, _ = _env(8)
    a, b, c = both.reset(), alone.reset(), plain.reset()
    assert set(a) - set(c) == {'pov_obs'} and set(c) - set(b) == {'pov'} and 'pov_obs' not in c
    assert alone.pov is None and both.pov is a['pov']
    for t in range(4):
        a, b, c = both.step(actions[t])[0], alone.step(actions[t])[0], plain.step(actions[t])[0]
        assert 'pov' not in b
        assert torch.equal(a['pov'], both.render_pov()) and torch.equal(a['pov'], c['pov'])
        _same(a['pov_obs'], b['pov_obs'], f'step {t}')


def test_split_halves_equal_the_whole_batch():
    from gridworld_amd import ObsSpec
    spec = ObsSpec(gray=True, stack=4)
    whole, actions = _env(pov_obs=spec)
    parts, _ = _env(pov_obs=spec)
    whole.reset()
    parts.reset()
    halves = parts.split(2)
    for t in range(9):
        whole.step(actions[t])
        for k, h in enumerate(halves):
            h.step_walking_ptr(actions[t, k * 24:(k + 1) * 24].contiguous())
    for h in halves:
        h.join()
    _same(parts.pov_obs, whole.pov_obs, 'split')
    assert torch.equal(parts.pov, whole.pov)
    assert halves[1].pov_obs.data_ptr() == parts.pov_obs[24:].data_ptr()


@pytest.mark.parametrize('chains', [1, 2])
def test_captured_steps_draw_after_every_step_of_their_chain(chains):
    from gridworld_amd import ObsSpec
    spec = ObsSpec(gray=True, stack=4)
    eager, actions = _env(pov_obs=spec)
    graphed, _ = _env(pov_obs=spec)
    eager.reset()
    graphed.reset()
    g = graphed.capture_steps(actions[:5].contiguous(), chains=chains)
    for rep in range(2):
        for t in range(5):
            want = eager.step(actions[t])[0]
        got = g.replay()[0]
        _same(got['pov_obs'], want['pov_obs'], f'replay {rep}')
        assert got['pov_obs'] is graphed.pov_obs and torch.equal(got['pov'], want['pov'])
    # the state moves without a draw: the next draw, eager or replayed, restarts every stack
    eager.rollout_actions(actions[5:8].contiguous())
    graphed.rollout_actions(actions[5:8].contiguous())
    for t in range(5):
        want = eager.step(actions[t])[0]
        if t == 0:
            lum = OM.luminance(eager.render_pov())
            for k in range(4):
                assert torch.equal(want['pov_obs'][:, k], lum)
    _same(g.replay()[0]['pov_obs'], want['pov_obs'], 'replay after rollout_actions')
    for t in range(5):
        want = eager.step(actions[t])[0]
    _same(g.replay()[0]['pov_obs'], want['pov_obs'], 'replay after the fill')
