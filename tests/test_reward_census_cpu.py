"""Which situations of the reference's reward path the parity scenarios reach (CPU only, the oracle alone).

The instrumented build of oracle/igw_oracle.c (tests/step_census.py) also counts reward situations -- what the synthetic
task looks like, which votes a changed cell casts, whether the cached max_int went stale and how a recount caught up,
where the best alignment lies, how the episode ended -- and reads the branch outcomes of the oracle's five task
functions.  It is stepped through

  1. the scenarios test_step_census_cpu.py replays (every step fixture, the scenarios of tests/test_gpu_parity.py, the
     first 100 fuzz cases) and the directed step cases of tests/step_cases.py -- what they leave unreached is written to
     profiles/r25_reward_census.json;
  2. the directed cases of tests/reward_cases.py, after which every reward bin is reached by those cases alone and every
     branch outcome of the task functions by the union, except what reward_cases.UNREACHABLE names with its reason.

The oracle must equal tests/golden/s15_reward_cases.npz (the same cases as the Python reference played them, recorded
by tests/golden/gen_reward_cases.py) bit for bit, and where the reference tree is present the fixture is recorded again
and must not have moved."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import reward_cases as R
import step_cases as K
import step_census as SC
from test_step_census_cpu import FUZZ_CASES, FUZZ_ENVS, fuzz_scenarios, parity_scenarios

HERE = os.path.dirname(os.path.abspath(__file__))
PROFILE = os.path.join(HERE, '..', 'profiles', 'r25_reward_census.json')


@pytest.fixture(scope='module')
def census(tmp_path_factory):
    return SC.Census(tmp_path_factory.mktemp('reward_census'))


@pytest.fixture(scope='module')
def before(census):
    """What the older scenarios leave unreached (the instrumented oracle keeps counting: later tests see the union)."""
    steps = dict(fixtures=SC.replay_fixtures(census), parity_scenarios=parity_scenarios(census.O))
    steps['fuzz'], skipped = fuzz_scenarios(census.O)
    steps['step_cases'] = 0
    for space in ('walking', 'flying'):
        b = K.batch(space)
        for _ in K.run_oracle(census.O, b):
            steps['step_cases'] += len(b['names'])
    branches = census.branches(SC.TASK_FUNCTIONS)
    return dict(steps=steps, fuzz_cases_skipped=skipped, bins=len(census.reward_names), branches=len(branches),
                unreached_bins=census.unreached_reward_bins(), unreached_branches=sorted(k for k, v in branches.items() if v == 0))


def test_reward_census_of_the_older_scenarios(before):
    """The measurement: written to profiles/r25_reward_census.json (deterministic, so a rerun rewrites the same file)."""
    doc = dict(what='situations of the reward path that every step fixture, the scenarios of tests/test_gpu_parity.py, '
                    f'{FUZZ_CASES} cases of tests/fuzz_parity.py (seed 0, first {FUZZ_ENVS} envs of a case) and the directed '
                    'cases of tests/step_cases.py never reach; reward bins and branch outcomes of the task functions as '
                    'tests/step_census.py names them',
               oracle_env_steps=before['steps'], fuzz_cases_skipped_device_side_tasks=before['fuzz_cases_skipped'],
               bins_total=before['bins'], bins_unreached=before['unreached_bins'],
               branch_outcomes_total=before['branches'], branch_outcomes_unreached=before['unreached_branches'],
               unreachable=R.UNREACHABLE)
    with open(PROFILE, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    assert before['bins'] >= 95 and before['branches'] > 40
    # the older scenarios do leave reachable reward situations out: that is why the directed cases exist
    assert set(before['unreached_bins']) - set(R.UNREACHABLE)


def test_directed_reward_cases_reach_every_situation(census, before, tmp_path):
    alone = SC.Census(tmp_path, coverage=False)         # bins: by the directed reward cases alone
    for O in (alone.O, census.O):                       # branch outcomes: with the older scenarios
        for group in R.GROUPS:
            for _ in R.run_oracle(O, R.batch(group)):
                pass
            R.user_task_truth(O, R.batch(group))        # (igo_task_eval: the argmax the task kernels are compared with)
    unreached = set(alone.unreached_reward_bins()) | {k for k, v in census.branches(SC.TASK_FUNCTIONS).items() if v == 0}
    assert unreached == set(R.UNREACHABLE), (sorted(unreached - set(R.UNREACHABLE)), sorted(set(R.UNREACHABLE) - unreached))
    assert all(len(reason) > 10 for reason in R.UNREACHABLE.values()) and len(R.UNREACHABLE) <= 12


def test_each_case_lands_in_its_situation(tmp_path):
    """One situation per case: the bins a case is there for, counted on that case alone in the group it runs in."""
    alone = SC.Census(tmp_path, coverage=False)
    want = {'complete_rot0': 'done.complete.rot0', 'complete_rot1': 'done.complete.rot1', 'complete_rot2': 'done.complete.rot2',
            'complete_rot3': 'done.complete.rot3', 'complete_extreme': 'best.shift.extreme', 'complete_extreme_rotated': 'best.shift.extreme',
            'complete_at_max_steps': 'done.complete_at_max_steps', 'empty_task': 'done.empty_task', 'tower_climb': 'syn.top_level.8',
            'restore_start': 'change.syn.restore_start', 'stale_then_catch_up': 'right.ge+2', 'stale_then_catch_down': 'right.le-2',
            'stale_votes_both': 'votes.both', 'alias_difference': 'cache.stale_kept', 'tie_iteration_order': 'best.tie',
            'drop_unique': 'best.drop_unique', 'drop_shared': 'best.drop_shared', 'wrong_colour': 'votes.none', 'full_level': 'votes.121',
            'spans_x': 'adm.x_only', 'spans_z': 'adm.z_only', 'full_grid_narrows': 'user.full_grid_narrows',
            'not_invariant': 'user.not_invariant', 'size_reward_pays': 'size_reward.pays', 'size_reward_zero': 'size_reward.zero'}
    for group in ('main', 'size'):
        b = R.batch(group)
        for i, name in enumerate(b['names']):
            if name not in want:
                continue
            alone.lib.igo_census_reset()
            for _ in R.run_oracle(alone.O, b, [i]):
                pass
            assert alone.reward_bins()[want.pop(name)] > 0, name
    assert not want
    b = R.batch('main')
    i = b['names'].index('complete_unshifted')
    alone.lib.igo_census_reset()
    for _ in R.run_oracle(alone.O, b, [i]):
        pass
    bins = alone.reward_bins()
    assert bins['done.complete.rot0'] > 0 and bins['done.complete.shifted'] == 0
    for lv in range(9):
        alone.lib.igo_census_reset()
        for _ in R.run_oracle(alone.O, b, [b['names'].index(f'level{lv}')]):
            pass
        bins = alone.reward_bins()
        assert bins[f'change.place.level{lv}'] and bins[f'change.break.level{lv}'] and bins[f'syn.top_level.{lv}'], lv


def test_oracle_equals_the_reference_on_the_reward_cases():
    from oracle import oracle as O
    z = np.load(os.path.join(HERE, R.FIXTURE))
    n = sum(R.against_fixture(O, group, z) for group in R.GROUPS)
    assert n == sum(z[g + '_done'].size for g in R.GROUPS) > 4000
    assert all(k.split('_', 1)[1] in ('agentPos', 'inventory', 'compass', 'reward', 'done', 'grid_changes', 'internal', 'reset_before',
                                      'syn_max_int', 'env_max_int') for k in z.files)
    assert os.path.getsize(os.path.join(HERE, R.FIXTURE)) < 300_000
    sys.path.insert(0, os.path.join(HERE, 'golden'))
    try:
        import ref_harness as H
    finally:
        sys.path.pop(0)
    if os.path.isdir(H.REFERENCE_ROOT):
        # the live reference, in a process of its own (importing it shadows `gym` with a shim): it must still return
        # what the fixture holds
        r = subprocess.run([sys.executable, os.path.join(HERE, 'golden', 'gen_reward_cases.py'), '--check'],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
