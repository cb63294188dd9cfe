#!/usr/bin/env python3
"""Records the Python reference's side of the 200 scenarios tests/test_ref_fuzz.py replays (seeds 77000-77199,
at most 150 steps each; scenario generator: tests/scenario_fuzz.py) into tests/golden/s13_ref_fuzz.npz.
Build container only (needs the reference, through ref_harness):   python tests/golden/gen_ref_fuzz.py
While recording, every step is also compared with the live CPU oracle; the archive is written only with 0 mismatches."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE), os.path.dirname(HERE + '/..')]
import fuzz_ref_vs_oracle as F  # noqa: E402
import ref_fuzz_replay as R  # noqa: E402
import scenario_fuzz as S  # noqa: E402

SEEDS = range(77000, 77200)
MAX_T = 150
OUT = os.path.join(HERE, 's13_ref_fuzz.npz')


def main():
    rb = R.RecordingBackend(F.backend())
    records, results = [], []
    for seed in SEEDS:
        rec = rb.begin()
        results.append(S.run_scenario_safe(seed, rb, MAX_T))
        records.append((seed, rec))
    s = S.summarize(results, 0.0)
    print({k: s[k] for k in ('scenarios', 'reference_env_steps', 'resets', 'mismatches')})
    if s['mismatches']:
        print(s['first_mismatches'][:2])
        return 1
    np.savez_compressed(OUT, **R.pack(records))
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')
    return 0


if __name__ == '__main__':
    sys.exit(main())
