"""The relabel query past 2^32 bytes of output: 90,000 episodes whose `first` alias the 32 real
logs of one case, 48 goals each, L = 256, `reward` alone -- 4.4 GB, addressed with 64-bit offsets.  Every row equals the
row of the log it aliases, the 32 source rows equal a launch of their own, and the canaries around the buffer stay."""
import numpy as np
import pytest
import torch

from gridworld_amd import relabel as _feature  # noqa: F401  (without the query nothing in this file can run)

import relabel_cases as RC
import relabel_model as RM

pytestmark = pytest.mark.gpu

E, G, L, SRC = 90000, 48, 256, 32
CANARY = 4096    # float32 words in front of and behind the output (16 KiB: the view stays 16-byte aligned)


def test_ninety_thousand_aliased_episodes_fill_4_4_gb_row_for_row():
    import gridworld_amd as GW
    from gridworld_amd import VecGridWorld
    case = RC.cases()['towers']
    env = VecGridWorld(SRC, **case['kw'])
    env.set_tasks(case['targets'], case['starts'])
    rec, heads = env.enable_trajectory_log(SRC, L)
    env.reset()
    acts = torch.from_numpy(case['actions']).to(env.device)
    for t in range(RC.T):
        env.step(acts[t])
    dev = env.device
    h = heads.cpu().numpy()
    slot = h[:, :, 1].argmax(1)
    assert (h[np.arange(SRC), slot, 1] == RC.T).all()
    src_first = torch.from_numpy(((np.arange(SRC) * 2 + slot) * L).astype(np.int64)).to(dev)
    idx = torch.arange(E, device=dev) % SRC
    first, length = src_first[idx].contiguous(), torch.full((E,), RC.T, dtype=torch.int32, device=dev)
    starts = env.task_start[idx].contiguous()
    at = (torch.arange(G, dtype=torch.int32, device=dev) % (RC.T + 1))[None].expand(E, G).contiguous()
    assert E * G * L * 4 > 1 << 32
    base = torch.full((E * G * L + 2 * CANARY,), 7.0, dtype=torch.float32, device=dev)
    out = base[CANARY:CANARY + E * G * L].view(E, G, L)
    res = GW.relabel(rec, first, length, starts, at=at, outputs=('reward',), out={'reward': out})
    assert res['reward'] is out
    small = GW.relabel(rec, src_first, length[:SRC], starts[:SRC], at=at[:SRC], outputs=('reward',))['reward']
    torch.cuda.synchronize()
    assert bool((base[:CANARY] == 7.0).all()) and bool((base[-CANARY:] == 7.0).all())
    bits = out.view(torch.int32)
    want = small.view(torch.int32)
    assert torch.equal(bits[:SRC], want) and torch.equal(bits[E - E % SRC - SRC:E - E % SRC], want)
    step = 100 * SRC
    for lo in range(0, E, step):
        m = min(step, E - lo)
        whole = m - m % SRC
        assert bool((bits[lo:lo + whole].view(-1, SRC, G, L) == want).all()), lo
        if m != whole:
            assert torch.equal(bits[lo + whole:lo + m], want[:m - whole]), lo
    # ... and the source rows are the model's (entries 0..47 of env 5's own episode)
    b = RC.base('towers')
    for g in (0, 1, 24, 47):
        m = RM.episode(b['starts'][5], b['change'][5], b['grids'][g, 5], RC.RIGHT, RC.WRONG, 250, 1.0, L=L)
        assert np.array_equal(small[5, g].cpu().numpy().view(np.uint32), m['reward'].view(np.uint32)), g
