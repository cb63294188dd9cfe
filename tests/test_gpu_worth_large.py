"""The worth query past the 2^32 byte mark: `word` is 15,456 bytes per env, so the smallest batch whose last row starts
past 2^32 bytes is 277,887 envs; 277,897 are run.  The entry reads state rows and the task table, so the batch is those
rows alone: the 32 envs of the `towers` case (tests/worth_cases.py) at step 25, env i holding the state of env i % 32.
The first rows, the last rows and 64 seeded rows are compared against the model of tests/worth_model.py, and every row's
`best` against the small batch's."""
import numpy as np
import pytest
import torch

import worth_cases as WC
import worth_model as WM

pytestmark = pytest.mark.gpu

ROW = 1104
ENV_BYTES = 7 * ROW * 2        # 15,456
N = 277897


def test_word_output_past_4_gib():
    from gridworld_amd import VecGridWorld, worth as W
    assert (N - 1) * ENV_BYTES > 2 ** 32
    case, c = WC.cases()['towers'], WC.CHECKPOINTS.index(25)
    E = WC.E
    small = VecGridWorld(E, **case['kw'])
    small.set_tasks(case['targets'], case['starts'])
    small.reset()
    acts = torch.from_numpy(case['actions']).to(small.device)
    for t in range(25):
        small.step(acts[t])
    dev = small.device
    env_of = torch.arange(N, device=dev) % E
    state = [small.grid_buf[env_of].contiguous(), small.hist_buf[env_of].contiguous(), small.aux_buf[env_of].contiguous(),
             small.agent_buf[env_of].contiguous(), small.task_target, small.task_start, small.task_meta, small.task_index]
    cfg = small.cfg
    res = W.launch(state, N, (cfg.right_placement_scale, cfg.wrong_placement_scale, cfg.max_steps), None, False,
                   W.OUTPUTS, None, dev, small._stream())
    word, best = res['word'], res['best']
    assert tuple(word.shape) == (N, 7, 9, 11, 11) and word.stride(0) == 7 * ROW
    assert word.numel() == 0 or (word.data_ptr() % 16 == 0 and word.untyped_storage().nbytes() >= N * ENV_BYTES > 2 ** 32)
    raw = torch.as_strided(word, (N, 7, ROW), (7 * ROW, ROW, 1))
    model = WC.words('towers')[c]
    rng = np.random.RandomState(32)
    rows = np.unique(np.concatenate([np.arange(8), np.arange(N - 8, N), rng.randint(0, N, 64)]))
    got = raw[torch.from_numpy(rows).to(dev)].cpu().numpy()
    assert (rows[-1] * ENV_BYTES) > 2 ** 32
    bad = int((got != model[rows % E]).sum())
    ref = torch.from_numpy(np.stack([WM.best_of(model[i], WC.RIGHT, WC.WRONG) for i in range(E)])).to(dev)
    bad_best = int((best != ref[env_of]).sum())
    print(f'{N} envs, {len(rows)} rows compared: {bad} words differ; {bad_best} elements of best differ over all rows')
    assert bad == 0 and bad_best == 0
