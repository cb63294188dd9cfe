"""The aim query past the 2^31 and 2^32 byte marks: a plane is 4,416 bytes per env, so the smallest batch whose `place`
plane passes 2^32 bytes is 972,593 envs.  The entry reads nothing but agent records and occupancy rows, so the batch is
those rows alone: the 64 envs of tests/large_cases.py stepped a few times, env i holding the state of env i % 64.
max_turns = 1 (five rays per env) keeps the launch cheap; the window rows (the first, around each mark, the last) are
compared with the same entry run over copies of those rows, and every pad word of the whole plane is checked on the
device."""
import numpy as np
import pytest
import torch

import aim_cases as AC
import large_cases as LC

pytestmark = pytest.mark.gpu

ROW = 1104
PLANE_ROW = 4 * ROW                                  # 4,416 bytes
N = -(-LC.MARKS[1] // PLANE_ROW) + LC.SPAN           # 972,593 + 64 envs


def test_place_plane_past_4_gib():
    from gridworld_amd import VecGridWorld, aim as A
    assert N * PLANE_ROW > LC.MARKS[1] and (N - LC.SPAN - 1) * PLANE_ROW < LC.MARKS[1]
    targets, starts, poses = LC.tasks()
    small = VecGridWorld(LC.NUM_TASKS, **LC.KW)
    small.set_tasks(targets, starts, init_pose=poses)
    small.reset()
    acts = torch.from_numpy(LC.walk_actions(np.arange(LC.NUM_TASKS), steps=6)).to(small.device)
    for t in range(6):
        small.step(acts[t])
    dev = small.device
    env_of = torch.arange(N, device=dev) % LC.NUM_TASKS
    agent, occ = small.agent_buf[env_of].contiguous(), small.occ_buf[env_of].contiguous()
    place = A.launch(agent, occ, N, 1, True, False, None, dev, small._stream())['place']
    assert tuple(place.shape) == (N, 9, 11, 11) and place.stride(0) == ROW
    raw = torch.as_strided(place, (N, ROW), (ROW, 1))
    w = LC.windows(PLANE_ROW, N)
    assert [len(rows) for _, rows in LC.marks_in(PLANE_ROW, N)] == [LC.SPAN, LC.SPAN] and w[0] == 0 and w[-1] == N - 1
    widx = torch.from_numpy(w).to(dev)
    got = raw[widx]
    want = A.launch(agent[widx].contiguous(), occ[widx].contiguous(), len(w), 1, True, False, None, dev,
                    small._stream())['place']
    want = torch.as_strided(want, (len(w), ROW), (ROW, 1))
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    # the small batch's own answer, tiled: what every row of the large plane has to hold
    ref = torch.as_strided(small.aim(max_turns=1, brk=False)['place'], (LC.NUM_TASKS, ROW), (ROW, 1))
    assert torch.equal(got, ref[widx % LC.NUM_TASKS])
    # ... and that answer is the model's (tests/aim_cases.py; the scenario's poses are on the 5-degree lattice).  The floor
    # is on the model's count: the scenario starts every env looking at the ground ahead of it and six random steps
    # turn few of them away, so at least half of the 64 states have a cell to place at within one turn.
    grids, inter = small.grid.cpu().numpy(), small.internals()
    model = np.stack([AC.model(grids[i], inter[i, :5], 1)['place'] for i in range(LC.NUM_TASKS)])
    assert np.array_equal(ref[:, :1089].cpu().numpy(), model)
    reached = int((model >= 0).sum())
    print(f'{N} envs, {len(w)} window rows; the 64 states reach {reached} place cells within one turn')
    assert reached >= 32
    step = -(-N // 16)
    for lo in range(0, N, step):       # a sixteenth at a time: no whole-size temporaries
        part = raw[lo:lo + step]
        assert bool((part[:, 1089:] == -1).all())
        assert torch.equal(part, ref[env_of[lo:lo + step]])
