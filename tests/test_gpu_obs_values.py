"""Every byte value through the observation stage (igw_render_pov_obs; DESIGN.md section 8, "Training-layout
observations"): frames that hold every value of R, G, B and of the luminance (tests/value_cases.py: the atlas, the poses
and the (scale, bias) table, pinned by tests/test_value_cases_cpu.py), at a size that takes the four-pixel lanes and at
one that sends every pixel alone.  The yardstick never touches the device: value_cases.expected() is numpy, IEEE-754
with gradual underflow and overflow to +-inf -- what torch gives on the CPU -- so a flush or a rounding mode of the
device cannot show up on both sides.  Equality is on the raw bits."""
import numpy as np
import pytest
import torch

import value_cases as V
from render_checks import Tally

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', params=V.SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def drawn(request):
    """(env, its uint8 frames on the host) of the scene of value_cases at one frame size: one construction a size."""
    from gridworld_amd import VecGridWorld
    grid, poses = V.scene()
    n = len(poses)
    env = VecGridWorld(n, render_size=request.param)
    env.set_render_atlas(V.atlas().copy())
    grids = np.repeat(grid[None], n, 0)
    env.set_tasks(grids, grids, init_pose=poses)
    env.reset()
    frames = env.render_pov().cpu().numpy()
    assert frames.shape == (n, request.param[1], request.param[0], 3)
    return env, frames


def _bits(t):
    """The raw bits of a device tensor as an unsigned numpy array."""
    t = t.cpu()
    if t.dtype is torch.uint8:
        return t.numpy()
    signed, unsigned = {2: (torch.int16, np.uint16), 4: (torch.int32, np.uint32)}[t.element_size()]
    return t.view(signed).numpy().view(unsigned)


def _spec(dtype, gray, row, stack=1):
    from gridworld_amd import ObsSpec
    scale, bias, _ = V.ROWS[row]
    return ObsSpec(dtype, gray=gray, stack=stack, scale=scale, bias=bias)


def _differences(got, want, frames, gray):
    """The byte values whose stored bits differ, as 'v: got / want' strings (the first few)."""
    bad = np.argwhere(got != want)
    src = np.tile(V.planes(frames, gray), (1, got.shape[1] // (1 if gray else 3), 1, 1))
    seen = {}
    for i in bad[:4096]:
        seen.setdefault(int(src[tuple(i)]), f'{int(got[tuple(i)]):#x} / {int(want[tuple(i)]):#x}')
    return [f'{v}: {s}' for v, s in sorted(seen.items())][:8]


def test_the_frames_drawn_cover_every_value(drawn):
    env, frames = drawn
    c = V.coverage(frames)
    print(f'{frames.shape}: {c["triples"]} distinct triples')
    assert c['missing'] == [[], [], []] and c['missing_luminance'] == [] and c['triples'] >= V.MIN_TRIPLES
    # and they are the frames the f64 model predicts, by the limits of tests/test_gpu_render.py
    tally = Tally(f'value_cases at {frames.shape[2]} x {frames.shape[1]}')
    for k, res in enumerate(V.models((frames.shape[2], frames.shape[1]))):
        tally.add(frames[k], res, 3)
    tally.check()


def test_uint8_planes(drawn):
    from gridworld_amd import ObsSpec
    env, frames = drawn
    for gray in (False, True):
        spec = ObsSpec(torch.uint8, gray=gray, stack=2)
        got = _bits(env.render_pov_obs(spec, fill=True))
        want = V.expected(frames, spec)
        assert got.shape == want.shape and got.dtype == want.dtype
        assert np.array_equal(got, want), ('grey' if gray else 'rgb', _differences(got, want, frames, gray))


@pytest.mark.parametrize('dtype', V.DTYPES)
def test_every_row_of_the_table_in_rgb_and_grey(drawn, dtype):
    env, frames = drawn
    failures = []
    for row, (scale, bias, what) in enumerate(V.ROWS):
        for gray in (False, True):
            spec = _spec(getattr(torch, dtype), gray, row)
            got = _bits(env.render_pov_obs(spec, fill=True))
            want = V.expected(frames, spec)
            assert got.shape == want.shape and got.dtype == want.dtype
            if not np.array_equal(got, want):
                failures.append((f'{scale!r} * v + {bias!r} ({what})', 'grey' if gray else 'rgb',
                                 int((got != want).sum()), _differences(got, want, frames, gray)))
    for f in failures:
        print(dtype, *f)
    assert not failures, failures[:4]


NEG_ZERO, NEG_INF, POS_INF = 17, 16, 15            # rows of V.ROWS: -1 * v - 0.0, -3.3e38 * v + 3.4e38, 3.3e38 * v


@pytest.mark.parametrize('dtype', V.DTYPES)
def test_the_shift_of_a_stack_moves_signed_zeros_and_infinities_unchanged(drawn, dtype):
    """stack = 2: a fill with the -0.0 row, then a shift with the -inf row and one with the +inf row.  What a shift
    moves from slot 1 to slot 0 keeps its bits; rgb, so that all three planes of a slot move."""
    env, frames = drawn
    assert V.ROWS[NEG_ZERO][:2] == (-1.0, -0.0) and V.ROWS[NEG_INF][0] == -3.3e38 and V.ROWS[POS_INF][0] == 3.3e38
    dt = getattr(torch, dtype)
    alone = [V.expected(frames, _spec(dt, False, row)) for row in (NEG_ZERO, NEG_INF, POS_INF)]
    zero = {'float32': 0x80000000}.get(dtype, 0x8000)
    assert (alone[0] == zero).any() and (alone[1] == V.table(dtype, *V.ROWS[NEG_INF][:2])[255]).any()
    out = env.render_pov_obs(_spec(dt, False, NEG_ZERO, stack=2), fill=True)
    assert np.array_equal(_bits(out), np.concatenate([alone[0], alone[0]], 1))
    for k, row in ((1, NEG_INF), (2, POS_INF)):
        assert env.render_pov_obs(_spec(dt, False, row, stack=2), out=out) is out
        assert np.array_equal(_bits(out), np.concatenate([alone[k - 1], alone[k]], 1)), (dtype, k)
