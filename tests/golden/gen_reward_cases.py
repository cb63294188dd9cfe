#!/usr/bin/env python3
"""The directed reward cases (tests/reward_cases.py) as the Python reference plays them -> tests/golden/s15_reward_cases.npz.

Run in the build container only (needs the reference tree, see ref_harness.py):

    python tests/golden/gen_reward_cases.py            records the fixture
    python tests/golden/gen_reward_cases.py --check    records again and compares with the committed fixture, bit for bit

One reference env per case and group (reward_cases.GROUPS: 'main', 'size' with SizeReward, 'short' with a time limit of
six steps), its scripted actions padded as reward_cases.batch() pads them, the user task built with the case's full grid
and invariance, an episode that ended reset before the next step (ref_harness.run_batch), the reference's own libm.  The
fixture holds what the reference returned and nothing else: per group and per (case, step) the float32 observations,
the inventory, reward, done, the float64 internals, the synthetic task's cached max_int, the flag "reset before this
step", per case GridWorld.max_int after the first reset, and the grids as a change list (reward_cases.pack_grids); the
cases themselves stay in reward_cases.py.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_harness as H  # noqa: E402
import reward_cases as R  # noqa: E402

PATH = os.path.join(HERE, 's15_reward_cases.npz')
KEYS = ('agentPos', 'inventory', 'compass', 'reward', 'done', 'internal', 'reset_before', 'syn_max_int', 'env_max_int')


def record(group):
    b = R.batch(group)
    rows = []
    for i in range(len(b['names'])):     # one call per case: the full grid and the invariance are per task
        tk = dict(invariant=bool(b['invariant'][i]))
        if b['has_full'][i]:
            tk['full_grid'] = b['fulls'][i].astype(np.int32)
        rows.append(H.run_batch(dict(b['kw']), b['targets'][i:i + 1], [H.dense_to_sparse(b['starts'][i])],
                                np.ascontiguousarray(b['actions'][:, i:i + 1].T), task_kwargs=tk, init_pose=b['poses'][i:i + 1]))
    ref = {k: np.concatenate([r[k] for r in rows]) for k in KEYS + ('grid',)}
    out = {k: ref[k] for k in KEYS}
    out['inventory'] = out['inventory'].astype(np.int16)
    assert np.array_equal(out['inventory'], ref['inventory'])
    grids = ref['grid'].reshape(len(rows), b['T'], 1089)
    out['grid_changes'] = R.pack_grids(b, grids)
    assert np.array_equal(R.unpack_grids(b, out), grids)
    return out


def main():
    data = {}
    for group in R.GROUPS:
        for k, v in record(group).items():
            data[f'{group}_{k}'] = v
    if '--check' in sys.argv:
        z = np.load(PATH)
        bad = [k for k in data if k not in z.files or z[k].dtype != data[k].dtype or z[k].tobytes() != data[k].tobytes()]
        print('reference vs committed fixture:', 'identical' if not bad else f'DIFFERENT in {bad}')
        return 1 if bad or sorted(z.files) != sorted(data) else 0
    np.savez_compressed(PATH, **data)
    print(PATH, os.path.getsize(PATH), 'bytes;', {k: v.shape for k, v in data.items() if k.endswith('done')})
    return 0


if __name__ == '__main__':
    sys.exit(main())
