"""The peek query past the 2^32 byte mark: `reward` is K * H * 4 bytes per env, so with K = 4,096 candidates of H = 32
steps the smallest batch whose reward output passes 2^32 bytes is 8,193 envs (4,295,491,584 bytes).  The entry reads
nothing but state rows and the task table, so the batch is those rows alone: the 32 envs of the `towers` case stepped
14 times, env i holding the state of env i % 32, with one shared set of random candidates and outputs ('reward',
'ends').  The rows of the first, a middle and the last env are compared with the same entry run over copies of those
three rows; beyond that every env's rows are compared with those of the env whose state it holds, and the canary rows
behind both outputs are checked."""
import pytest
import torch

import peek_cases as PC

pytestmark = pytest.mark.gpu

N, K, H = 8193, 4096, 32


def test_reward_past_4_gib():
    from gridworld_amd import VecGridWorld, peek as P
    assert N * K * H * 4 > 1 << 32 and (N - 1) * K * H * 4 <= 1 << 32
    case = PC.cases()['towers']
    small = VecGridWorld(PC.E, **case['kw'])
    small.set_tasks(case['targets'], case['starts'], init_pose=case['poses'])
    small.reset()
    acts = torch.from_numpy(case['actions']).to(small.device)
    for t in range(14):
        small.step(acts[t])
    dev = small.device
    free, _ = torch.cuda.mem_get_info(dev)
    assert free > 6 << 30, f'{free >> 20} MiB free: the 4.3 GB output and its comparisons need 6 GiB'
    env_of = torch.arange(N, device=dev) % PC.E
    rows = [b[env_of].contiguous() for b in (small.grid_buf, small.occ_buf, small.hist_buf, small.aux_buf, small.agent_buf)]
    table = [small.task_target, small.task_start, small.task_meta, small.task_index]
    cfg = small.cfg
    reward_of = (cfg.right_placement_scale, cfg.wrong_placement_scale, cfg.max_steps, cfg.select_and_place)
    cand = torch.from_numpy(PC.random_candidates(9, n=1, k=K, h=H)[0]).to(dev)
    names = ('reward', 'ends')
    bufs = dict(reward=torch.full((N + 1, K, H), -7.0, dtype=torch.float32, device=dev),
                ends=torch.full((N + 1, K), -7, dtype=torch.int16, device=dev))
    got = P.launch(rows + table, N, cand, reward_of, 1.0, names, {k: v[:N] for k, v in bufs.items()}, dev, small._stream())
    assert got['reward'].data_ptr() == bufs['reward'].data_ptr() and got['reward'].numel() * 4 > 1 << 32
    pick = torch.tensor([0, N // 2, N - 1], device=dev)
    want = P.launch([r[pick].contiguous() for r in rows] + table, 3, cand, reward_of, 1.0, names, None, dev, small._stream())
    torch.cuda.synchronize()
    for k in names:
        assert torch.equal(got[k][pick].view(torch.int16 if k == 'ends' else torch.int32),
                           want[k].view(torch.int16 if k == 'ends' else torch.int32)), k
        assert bool((bufs[k][N] == -7).all()), k                       # the canary row
    # ... and what the small batch's own peek says of those states
    own = small.peek(cand, outputs=names)
    assert torch.equal(own['reward'][pick % PC.E].view(torch.int32), want['reward'].view(torch.int32))
    assert torch.equal(own['ends'][pick % PC.E], want['ends'])
    changed = int((own['reward'] != 0).sum())
    print(f'{N} envs x {K} candidates x {H} steps: {got["reward"].numel() * 4} bytes of reward; the 32 states pay '
          f'{changed} non-zero rewards, {int((own["ends"] > 0).sum())} candidates end')
    assert changed >= 10000
    # every env's rows equal those of the env whose state it holds, a block of 32 envs at a time
    for lo in range(0, N, PC.E):
        m = min(PC.E, N - lo)
        assert torch.equal(got['reward'][lo:lo + m].view(torch.int32), own['reward'][:m].view(torch.int32)), lo
        assert torch.equal(got['ends'][lo:lo + m], own['ends'][:m]), lo
