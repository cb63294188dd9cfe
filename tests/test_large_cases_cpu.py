"""tests/large_cases.py on the CPU: the sizes follow from the ABI's constants, every window straddles its mark, and the
committed scenario does on the oracle what tests/test_gpu_large.py needs it to do -- so that the GPU tests cannot pass
on a batch in which nothing happens."""
import numpy as np
import pytest

import large_cases as LC
from gridworld_amd import _lib as L


def test_sizes_follow_from_the_abi():
    assert (LC.GRID_ROW, LC.HIST_ROW, LC.OCC_ROW, LC.OUT_ROW, LC.AGENT_ROW, LC.AUX_ROW) == (1104, 1024, 192, 64, 64, 16)
    assert LC.header_int('include/igw.h', 'IGW_GRID_STRIDE') == L.GRID_STRIDE
    assert LC.header_int('include/igw.h', 'IGW_HIST_ROW') == L.HIST_ROW
    assert LC.N_MARK == 1 << 22 and LC.N_WALK == (1 << 22) + 101 and LC.N_FLY == (1 << 22) + 64
    # the histogram row passes 2^32 at env 2^22, the grid row earlier (inside env 3,890,368); both inside either batch
    assert LC.N_MARK * LC.HIST_ROW == LC.MARKS[1] and LC.MARKS[1] // LC.GRID_ROW == 3890368 < LC.N_MARK
    assert LC.N_WALK % 64 and LC.N_WALK % LC.FLY_ENVS_PER_BLOCK        # a ragged last wavefront and block
    assert LC.FLY_ENVS_PER_BLOCK == 64 and LC.N_FLY % LC.FLY_ENVS_PER_BLOCK == 0   # whole blocks: the EXACT variant
    assert L.auto_lanes(LC.N_WALK) == 4
    # the buffers whose first mark lies past these batches (the action mask's inputs: out of scope)
    assert LC.N_WALK * LC.OCC_ROW < LC.MARKS[0] and LC.N_WALK * LC.AGENT_ROW < LC.MARKS[0]
    assert (LC.N_POV, LC.N_OBS, LC.N_JPEG) == (349526 + 64, 10923 + 64, 4096 + 8)
    assert LC.FRAME_ROW == 12288 and LC.OBS_ROW == 393216 and LC.CHUNK == LC.SIZE[0] * LC.SIZE[1]
    assert (LC.N_POV - 64) * LC.FRAME_ROW >= LC.MARKS[1] > (LC.N_POV - 65) * LC.FRAME_ROW
    assert LC.MARKS[1] // LC.DEPTH_ROW == 262144 < LC.N_POV and LC.MARKS[0] // LC.SURFACE_ROW < LC.N_POV
    assert LC.N_POV * LC.LABEL_ROW < LC.MARKS[0]
    assert (LC.N_OBS - 64) * LC.OBS_ROW >= LC.MARKS[1] and LC.N_OBS > LC.SINK_SLOTS and 4 * LC.N_OBS <= LC.N_WALK
    assert LC.N_JPEG * LC.JPEG_STRIDE > LC.MARKS[1] and LC.N_POV <= LC.N_WALK


@pytest.mark.parametrize('stride,n', [(LC.GRID_ROW, LC.N_WALK), (LC.HIST_ROW, LC.N_WALK), (LC.OUT_ROW, LC.N_WALK),
                                      (LC.HIST_ROW, LC.N_FLY), (LC.FRAME_ROW, LC.N_POV), (LC.DEPTH_ROW, LC.N_POV),
                                      (LC.SURFACE_ROW, LC.N_POV), (LC.OBS_ROW, LC.N_OBS), (LC.JPEG_STRIDE, LC.N_JPEG)])
def test_every_window_straddles_its_mark(stride, n):
    w = LC.windows(stride, n)
    assert w[0] == 0 and w[-1] == n - 1 and len(np.unique(w)) == len(w) and (np.diff(w) > 0).all()
    assert set(range(min(64, n))) <= set(w) and set(range(n - 64, n)) <= set(w)
    assert set(range(n // 64 * 64, n)) <= set(w)                        # the ragged tail
    reached = LC.marks_in(stride, n)
    assert [m for m, _ in reached] == [m for m in LC.MARKS if n * stride > m]
    for mark, rows in reached:
        assert len(rows) == 64 or rows[-1] == n - 1
        assert set(rows) <= set(w)
        assert rows.min() * stride < mark <= (rows.max() + 1) * stride


def test_the_step_windows_are_the_union_over_three_strides():
    w = LC.step_windows(LC.N_WALK)
    assert 350 <= len(w) <= 600   # (the histogram's high window and the tail overlap)
    for s in LC.STEP_STRIDES:
        assert set(LC.windows(s, LC.N_WALK)) <= set(w)
    # the high hist window's envs all have a partner 2^22 envs below with the same task and other actions
    hi = w[w >= LC.N_MARK]
    assert len(hi) >= 64 and (LC.env_task(LC.N_WALK)[hi] == LC.env_task(LC.N_WALK)[hi - LC.N_MARK]).all()
    assert (LC.walk_actions(hi) != LC.walk_actions(hi - LC.N_MARK)).mean() > 0.9


def test_the_task_table():
    targets, starts, poses = LC.tasks()
    assert targets.shape == starts.shape == (64, 9, 11, 11) and poses.shape == (64, 5)
    has_start = starts.reshape(64, -1).any(1)
    assert 20 <= has_start.sum() <= 23                                   # about a third of the rows
    syn = targets.astype(np.int32) - starts
    assert ((syn != 0).reshape(64, -1).sum(1) >= LC.MIN_TARGET).all()    # no episode can end before the time limit
    assert (syn < 0).any() and len(np.unique(poses, axis=0)) == 64
    assert (poses[:, 3:] % 5 == 0).all() and (poses[:, 4] <= -35).all()
    assert LC.T <= 16 and LC.MAX_STEPS < LC.T < 2 * LC.MAX_STEPS


def test_the_flying_action_hash_is_the_same_in_numpy_and_torch():
    import torch
    envs = np.concatenate([np.arange(70), LC.N_MARK + np.arange(-3, 64)])
    for t in (0, 7, LC.T - 1):
        a, b = LC.fly_actions(envs, t), LC.fly_actions(torch.from_numpy(envs), t)
        for k in a:
            assert a[k].dtype == b[k].numpy().dtype and np.array_equal(a[k].view(np.uint32), b[k].numpy().view(np.uint32)), k
        assert (np.abs(a['movement']) <= 1).all() and (np.abs(a['camera']) <= 5).all()
        assert set(np.unique(a['inventory'])) == set(range(7)) and set(np.unique(a['placement'])) == {0, 1, 2}
    assert (LC.fly_actions(envs, 1)['movement'] != LC.fly_actions(envs, 2)['movement']).all(1).mean() > 0.99


@pytest.mark.parametrize('mode,n', [('walking', LC.N_WALK), ('flying', LC.N_FLY)])
def test_in_every_window_every_env_resets_and_eight_change_their_grid(mode, n):
    """The cap that keeps the GPU comparison from being vacuous, on the oracle alone: under the committed tasks, poses,
    seed, T and max_steps every window env auto-resets, by the time limit and by nothing else, and in every window of
    64 at least 8 envs change their grid at least once outside that reset."""
    w = LC.step_windows(n)
    ob, done, changed = LC.replay(mode, w)
    assert done.any(0).all()
    expect = np.zeros(LC.T, np.uint8)
    expect[LC.MAX_STEPS - 1] = 1
    assert (done == expect[:, None]).all()                               # the whole batch's episode clock (tasks())
    acted = np.delete(changed, LC.MAX_STEPS - 1, axis=0).any(0)
    spans = [np.arange(64), np.arange(n - 64, n)] + [rows for s in LC.STEP_STRIDES for _, rows in LC.marks_in(s, n)]
    assert len(spans) == 2 + 4                                           # grid: two marks, hist: two, out: none
    for rows in spans:
        k = int(acted[np.searchsorted(w, rows)].sum())
        assert k >= 8, (mode, rows[0], k)
    built = (ob.grid != 0).any(1)
    print(f'{mode}: {int(acted.sum())} of {len(w)} window envs changed their grid; {int(built.sum())} hold a block at the end')
    assert built.mean() >= 0.5
