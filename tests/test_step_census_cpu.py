"""Which situations of the reference's physics the step path's parity scenarios reach (CPU only, the oracle alone).

One instrumented build of oracle/igw_oracle.c (tests/step_census.py) is stepped through

  1. the scenarios the parity chain already had: every step fixture of tests/golden, the scenarios of
     tests/test_gpu_parity.py and the first 100 cases of tests/fuzz_parity.py's scenario draw (seed 0) -- what they
     leave unreached is written to profiles/r15_step_census.json;
  2. the directed cases of tests/step_cases.py, after which every situation bin is reached by the directed cases alone
     and every branch outcome of the step path by the union, except what step_cases.UNREACHABLE names with its reason.

The directed cases are also where the oracle itself had never been compared with the reference: the oracle must equal
tests/golden/s14_step_cases.npz (recorded from the reference by tests/golden/gen_step_cases.py) bit for bit, and where the
reference tree is present the fixture is recorded again and must not have moved."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import step_cases as K
import step_census as SC

HERE = os.path.dirname(os.path.abspath(__file__))
PROFILE = os.path.join(HERE, '..', 'profiles', 'r15_step_census.json')
FUZZ_CASES, FUZZ_ENVS = 100, 3   # of every drawn case the first 3 envs: situations are per env, and a reset (two
# Task constructions) costs the oracle milliseconds, so the batch sizes here are a fraction of the GPU tests'


def _rollout(O, n, T, seed, targets, starts=None, invariant=True, **kw):
    n //= 4
    ob = O.OracleBatch(n, **kw)
    ob.set_tasks(targets[:n] if len(targets) >= n else np.repeat(targets, n, axis=0), starts, invariant=invariant)
    ob.reset()
    return ob.rollout_walking(T, seed, autoreset=True)[0]


def _scripted(O, targets, starts, acts, autoreset=False, **kw):
    n = len(targets) // 4
    ob = O.OracleBatch(n, **kw)
    ob.set_tasks(targets[:n], None if starts is None else starts[:n])
    ob.reset()
    for a in acts:
        ob.step_walking(a[:n], autoreset=autoreset)
    return n * len(acts)


def parity_scenarios(O):
    """The scenarios of tests/test_gpu_parity.py (targets, starting grids, action streams: the counter RNG of
    fill_actions is the oracle's rollout RNG), the first sixteenth (config 2: eightieth) of the envs of each."""
    import golden_replay as GR
    from test_gpu_parity import _rt20_targets
    steps = 0
    tg = np.zeros((1, 9, 11, 11), np.int8)
    tg[0, 8, 10, 10] = 1
    steps += _rollout(O, 205, 120, 1234, tg, invariant=False, size_reward=False, max_steps=50)      # config 2
    steps += _rollout(O, 100, 300, 99, _rt20_targets(1000, 5)[:100], size_reward=False)                # rt20 auto-reset
    steps += _rollout(O, 125, 300, 4242, _rt20_targets(500, 11)[:125], size_reward=False)                    # fused rollout
    fx = GR.load_fixture('s2_walk_cdm')
    tg, st = np.tile(fx['targets'], (6, 1, 1, 1)), np.tile(fx['starts'], (6, 1, 1, 1))
    acts = np.random.RandomState(77).choice([1, 2, 3, 4, 5, 7, 9, 12, 13, 14, 15, 16, 16, 16, 17, 17], size=(400, len(tg))).astype(np.int32)
    acts[:6] = 14
    steps += _scripted(O, tg, st, acts, size_reward=False, max_steps=1000)                             # start grids
    tg, st = np.tile(fx['targets'], (41, 1, 1, 1))[:111], np.tile(fx['starts'], (41, 1, 1, 1))[:111]
    acts = np.random.RandomState(4).choice([1, 3, 5, 7, 9, 12, 14, 14, 15, 16, 16, 16, 17, 17, 17], size=(70, 333)).astype(np.int32)[:, :111]
    acts[40:44] = np.array([14, 14, 17, 16], np.int32)[:, None]
    steps += _scripted(O, tg, st, acts, autoreset=True, size_reward=False, max_steps=9)                # desynchronised
    n = 384
    tg, st, rng = np.zeros((n, 9, 11, 11), np.int8), np.zeros((n, 9, 11, 11), np.int8), np.random.RandomState(12)
    for e in range(n):
        c = 1 + e % 3
        tg[e, 0] = c
        if e % 4 == 1:
            tg[e, 1, 2:9, 2:9] = c
        if e % 4 == 2:
            tg[e, 0, rng.randint(11), :] = 0
        if e % 5 == 3:
            st[e, 0, 4:7, 4:7] = c
    acts = rng.choice([1, 2, 3, 4, 6, 6, 7, 7, 8, 8, 12, 13, 14, 15, 16, 16, 17], size=(260, n)).astype(np.int32)
    acts[:8] = 14
    steps += _scripted(O, tg[:96], st[:96], acts[:, :96], size_reward=False, max_steps=1000)           # one-colour floors
    script = [14] * 8
    for rep in range(12):
        script += [17, 6 + rep % 6, 17, 1 + rep % 4, 17, 16, 12, 17, 16, 16, 5, 17, 3, 17, 13, 16]
    steps += _scripted(O, _rt20_targets(200, 21)[:50], None, np.repeat(np.asarray(script, np.int32)[:, None], 50, 1),
                       size_reward=False, max_steps=1000)                                             # a whole wave changes
    acts = np.random.RandomState(5).choice([1, 2, 3, 4, 5, 6, 7, 8, 12, 13, 14, 14, 15, 16, 16, 17, 17, 17, 0], size=(330, 600)).astype(np.int32)[:, :150]
    steps += _scripted(O, _rt20_targets(600, 31)[:150], None, acts, autoreset=True, size_reward=False, max_steps=120)   # recorded actions
    return steps


def fuzz_scenarios(O, cases=FUZZ_CASES, seed=0):
    """fuzz_parity's scenario draw, case by case in its RNG order, the oracle side alone.  Cases whose tasks the
    device chooses (task sampling, RandomTasks) cannot be played without it: their draws are consumed and skipped."""
    import fuzz_parity as F
    rng = np.random.RandomState(seed)
    steps = skipped = 0
    for c in range(cases):
        case = F.draw_case(c, rng)
        playable = case['extra'] in ('none', 'log')
        m = min(case['n'], FUZZ_ENVS)
        if playable:
            ob = O.OracleBatch(m, **case['space'], **case['kw'])
            ob.set_tasks(case['tg'][:m], case['st'][:m], full_grids=None if case['fg'] is None else case['fg'][:m])
            if case['poses'] is not None:
                ob.set_initial_pose(case['poses'][:m])
            ob.reset()
            O.use_device_trig(case['mode'] != 'walking' or case['poses'] is not None)
        try:
            for kind, da, oa in F.draw_steps(case, rng):
                if not playable:
                    continue
                for a in (da if kind == 'chunk' else [oa]):
                    if kind == 'chunk':
                        ob.step_walking(a[:m], autoreset=case['autoreset'])
                    else:
                        F.oracle_step(ob, case['mode'], tuple(v[:m] for v in a), case['autoreset'] and not case['manual'])
                    if case['manual'] and (case['autoreset'] or case['host_resets']) and ob.done.any():
                        ob.reset(ob.done.astype(bool))     # the logged variant resets the oracle by hand
                    steps += m
        finally:
            O.use_device_trig(False)
        skipped += not playable
    return steps, skipped


@pytest.fixture(scope='module')
def census(tmp_path_factory):
    return SC.Census(tmp_path_factory.mktemp('census'))


@pytest.fixture(scope='module')
def before(census):
    """What the older scenarios leave unreached (the instrumented oracle keeps counting: later tests see the union)."""
    steps = dict(fixtures=SC.replay_fixtures(census), parity_scenarios=parity_scenarios(census.O))
    steps['fuzz'], skipped = fuzz_scenarios(census.O)
    branches = census.branches()
    return dict(steps=steps, fuzz_cases_skipped=skipped, bins=len(census.names), branches=len(branches),
                unreached_bins=census.unreached_bins(), unreached_branches=sorted(k for k, v in branches.items() if v == 0))


def test_census_of_the_older_scenarios(before):
    """The measurement: written to profiles/r15_step_census.json (deterministic, so a rerun rewrites the same file)."""
    doc = dict(what='situations of the step path that every step fixture, the scenarios of tests/test_gpu_parity.py and '
                    f'{FUZZ_CASES} cases of tests/fuzz_parity.py (seed 0, first {FUZZ_ENVS} envs of a case) never reach; '
                    'bins and branch outcomes as tests/step_census.py names them',
               oracle_env_steps=before['steps'], fuzz_cases_skipped_device_side_tasks=before['fuzz_cases_skipped'],
               bins_total=before['bins'], bins_unreached=before['unreached_bins'],
               branch_outcomes_total=before['branches'], branch_outcomes_unreached=before['unreached_branches'],
               unreachable=K.UNREACHABLE)
    with open(PROFILE, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    assert before['steps']['fuzz'] > 5000 and before['fuzz_cases_skipped'] < FUZZ_CASES // 2
    # the random scenarios do leave reachable situations out: that is why the directed cases exist
    assert set(before['unreached_bins']) - set(K.UNREACHABLE)


def test_directed_cases_reach_every_situation(census, before, tmp_path):
    alone = SC.Census(tmp_path, coverage=False)         # bins: by the directed cases alone
    for O in (alone.O, census.O):                       # branch outcomes: with the older scenarios
        for space in ('walking', 'flying'):
            for _ in K.run_oracle(O, K.batch(space)):
                pass
    unreached = set(alone.unreached_bins()) | set(census.unreached_branches())
    assert unreached == set(K.UNREACHABLE), (sorted(unreached - set(K.UNREACHABLE)), sorted(set(K.UNREACHABLE) - unreached))
    assert all(len(reason) > 10 for reason in K.UNREACHABLE.values()) and len(K.UNREACHABLE) <= 12


def test_oracle_equals_the_reference_on_the_directed_cases():
    from oracle import oracle as O
    z = np.load(os.path.join(HERE, K.FIXTURE))
    n = sum(K.against_fixture(O, space, z) for space in ('walking', 'flying'))
    assert n == sum(z[s + '_done'].size for s in ('walking', 'flying')) > 5000
    assert all(k.split('_', 1)[1] in ('agentPos', 'inventory', 'compass', 'reward', 'done', 'grid', 'internal', 'reset_before')
               for k in z.files)
    sys.path.insert(0, os.path.join(HERE, 'golden'))
    try:
        import ref_harness as H
    finally:
        sys.path.pop(0)
    if os.path.isdir(H.REFERENCE_ROOT):
        # the live reference, in a process of its own (importing it shadows `gym` with a shim): it must still return
        # what the fixture holds
        r = subprocess.run([sys.executable, os.path.join(HERE, 'golden', 'gen_step_cases.py'), '--check'],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr


def test_normal_build_is_the_product_oracle(census):
    """The census flags are off in the normal build: no census symbol in oracle/libigw_oracle.so, and the instrumented
    library is another object than the one the parity tests step."""
    from oracle import oracle as O
    syms = subprocess.run(['nm', '-D', '--defined-only', O.build()], capture_output=True, text=True, check=True).stdout
    assert 'igo_step_walking' in syms and 'census' not in syms
    assert census.lib is not O.lib() and hasattr(census.lib, 'igo_census_read') and not hasattr(O.lib(), 'igo_census_read')
