"""Reference <-> oracle randomised slice, from the reference's recorded side (no reference needed at test time).

200 scenarios of tests/scenario_fuzz.py (seeds 77000-77199, at most 150 steps) -- random create_env kwargs, task
sources (Task, Subtasks, CustomTasks, RandomTasks), starting grids, initialize_world poses, all three action spaces,
glibc and correctly rounded trig -- whose reference side tests/golden/gen_ref_fuzz.py recorded into
tests/golden/s13_ref_fuzz.npz: every observation, reward, done, float64 internal and task counter the imported Python
reference returned, and the task it held at every reset.  The CPU oracle is stepped live through the same scenarios
and must agree on every step (tests/ref_fuzz_replay.py serves the records in the order run_scenario reads them).
The live version is tests/golden/fuzz_ref_vs_oracle.py; its long run (>= 5 M reference steps) is logged in
profiles/r05_fuzz_ref_vs_oracle.json."""
import os

import numpy as np

import ref_fuzz_replay as R
import scenario_fuzz as S

HERE = os.path.dirname(os.path.abspath(__file__))


def test_reference_vs_oracle_200_scenarios():
    goals = list(np.load(os.path.join(HERE, 'golden', 'cdm_goals.npz'))['dense'])   # sorted C1..C157, as the reference's
    B = R.ReplayBackend(os.path.join(HERE, 'golden', 's13_ref_fuzz.npz'), goals)
    assert B.seeds() == list(range(77000, 77200))
    results = []
    for seed in B.seeds():
        B.select(seed)
        results.append(S.run_scenario_safe(seed, B, max_T=150))
        assert results[-1]['mismatch'] is not None or B.replayed_all(), seed
    s = S.summarize(results, 0.0)
    assert s['scenarios'] == 200 and s['reference_env_steps'] > 15000
    assert s['mismatches'] == 0, s['first_mismatches'][:2]
    # every scenario family was drawn
    for key in ('space:walking', 'space:walking_dict', 'space:flying', 'source:task', 'source:subtasks',
                'source:custom', 'source:random', 'trig:glibc', 'trig:cr_libm'):
        assert s['by'][key]['steps'] > 0, key
