#!/usr/bin/env python3
"""The directed step cases (tests/step_cases.py) as the Python reference plays them -> tests/golden/s14_step_cases.npz.

Run in the build container only (needs the reference tree, see ref_harness.py):

    python tests/golden/gen_step_cases.py            records the fixture
    python tests/golden/gen_step_cases.py --check    records again and compares with the committed fixture, bit for bit

One reference env per case, its scripted actions padded with no-ops to the batch's length, max_steps as
step_cases.batch() sets it, an episode that ended reset before the next step (ref_harness.run_batch).  The walking cases
run on the reference's own libm; the flying cases with correctly rounded sin / cos / atan2 (ref_harness.cr_libm), the
convention of s4_fly_crlibm.  The fixture holds what the reference returned and nothing else: per action space and per
(case, step) the float32 observations, the inventory, the grid, reward, done, the float64 internals and the flag
"reset before this step"; the cases themselves stay in step_cases.py.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_harness as H  # noqa: E402
import step_cases as K  # noqa: E402

PATH = os.path.join(HERE, 's14_step_cases.npz')
KEYS = ('agentPos', 'inventory', 'compass', 'reward', 'done', 'grid', 'internal', 'reset_before')


def record(space):
    b = K.batch(space)
    kw = dict(b['kw'])
    starts = [H.dense_to_sparse(s) for s in b['starts']]
    if space == 'walking':
        ref = H.run_batch(kw, b['targets'], starts, np.ascontiguousarray(b['actions'].T), init_pose=b['poses'])
    else:
        acts = {k: np.ascontiguousarray(np.swapaxes(v, 0, 1)) for k, v in b['actions'].items()}
        with H.cr_libm():
            ref = H.run_batch(kw, b['targets'], starts, acts, init_pose=b['poses'])
    out = {k: ref[k] for k in KEYS}
    out['inventory'] = out['inventory'].astype(np.int16)
    assert np.array_equal(out['inventory'], ref['inventory'])
    out['grid'] = out['grid'].reshape(len(starts), -1, 1089)
    return out


def main():
    data = {}
    for space in ('walking', 'flying'):
        for k, v in record(space).items():
            data[f'{space}_{k}'] = v
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
