"""The recall query past 2^32 bytes of output: 2,700 samples that alias the 32 real logs of one
case, float32, K = 8, 13 channels, ego R = 10 -- 1.65 MB per sample, 4.46 GB of `next_obs`, addressed with 64-bit offsets.
The first and the last sample and a strided subset equal the model, samples of the same (e, t) equal each other across
the 2^32-byte mark, and the canaries around the buffer stay."""
import numpy as np
import pytest
import torch

from gridworld_amd import recall as _feature  # noqa: F401  (without the query nothing in this file can run)

import recall_cases as RCC
import recall_model as RCM
import vox_model as VM

pytestmark = pytest.mark.gpu

B, SRC, CAP = 2700, 32, 64
CANARY = 4096    # float32 words in front of and behind the output (16 KiB: the view stays 16-byte aligned)


def test_two_thousand_seven_hundred_samples_fill_4_4_gb_sample_for_sample():
    import gridworld_amd as G
    from gridworld_amd import VecGridWorld, VoxSpec
    name = 'towers'
    case, b = RCC.cases()[name], RCC.base(name)
    env = VecGridWorld(SRC, **case['kw'])
    env.set_tasks(case['targets'], case['starts'])
    rec, heads = env.enable_trajectory_log(SRC, CAP)
    env.reset()
    acts = torch.from_numpy(case['actions']).to(env.device)
    for t in range(RCC.T):
        env.step(acts[t])
    dev = env.device
    h = heads.cpu().numpy()
    slot = h[:, :, 1].argmax(1)
    assert (h[np.arange(SRC), slot, 1] == RCC.T).all()
    first = torch.from_numpy(((np.arange(SRC) * 2 + slot) * CAP).astype(np.int64)).to(dev)
    length = torch.full((SRC,), RCC.T, dtype=torch.int32, device=dev)
    spec = VoxSpec(planes=(('grid', 'onehot'), ('target', 'onehot')), agent=True, frame='ego', radius=10,
                   dtype=torch.float32, scale=0.5, bias=0.25, stack=8)
    per = int(np.prod(spec.shape(1)))
    assert spec.channels == 13 and per == 8 * 13 * 9 * 21 * 21 and B * per * 4 > 1 << 32
    i = np.arange(B)
    episode, step = (i % SRC).astype(np.int32), (1 + (i * 7) % RCC.T).astype(np.int32)
    base = torch.full((B * per + 2 * CANARY,), 7.0, dtype=torch.float32, device=dev)
    out = base[CANARY:CANARY + B * per].view(spec.shape(B))
    targets = case['targets'].reshape(SRC, -1).astype(np.int8)
    res = G.recall(rec, first, length, env.task_start, env.task_meta[:SRC, :40].contiguous().view(torch.float64), episode,
                   step, spec, goal=torch.from_numpy(targets).to(dev), outputs=('next_obs', 'valid'), out={'next_obs': out})
    assert res['next_obs'] is out
    torch.cuda.synchronize()
    assert bool((base[:CANARY] == 7.0).all()) and bool((base[-CANARY:] == 7.0).all()) and bool(res['valid'].all())
    # (e, t) repeats every lcm(32, 48) = 96 samples: sample j and sample j + 1536 are the same transition, and for the
    # last 1,164 of them the second lies behind the 2^32-byte mark
    bits = out.view(torch.int32)
    assert B * per * 4 > 1 << 32 > 1536 * per * 4 and 1536 % 96 == 0
    assert torch.equal(bits[:B - 1536], bits[1536:])
    pick = np.unique(np.concatenate([[0, 1, B - 2, B - 1], np.arange(0, B, 97)]))
    orec = RCC.records_of(b['change'], b['pos'])
    want = RCM.recall(orec, np.arange(SRC) * RCC.T, np.full(SRC, RCC.T), b['starts'], b['init'], episode[pick], step[pick], spec,
                      goal=targets, L=CAP)
    got = out[torch.from_numpy(pick).to(dev)].cpu()
    assert torch.equal(VM.bits(got), VM.bits(want['next_obs']))
    assert bool((got == 0.75).any()) and bool((got == 0.25).any())
