"""The reward path on the directed cases of tests/reward_cases.py: the situations random policies do not reach
(completion at every rotation and at extreme alignments, on the step the time limit ends as well, an empty synthetic
task, votes on every level and for every synthetic id -6..6, the stale cached max_int and the recount that catches up by
two, ties, drops of a unique and of a shared maximum, a full one-colour level ...) through the step kernel's persistent
vote histogram, the two task kernels and the reward queries.

One batch per group, every case in 5 adjacent envs, so that several envs of one wavefront complete, or go stale, on the
same step (at 16 lanes per env all four envs of a wavefront, at one lane per env 5 of 64).  After EVERY step all outputs,
the float64 internals and the task state (cached max_int, dirty, prev_size, step_no, size) are compared as raw bits with
the CPU oracle stepped alongside, and with tests/golden/s15_reward_cases.npz -- the same cases as the Python reference
played them.  0 mismatches allowed anywhere.  The oracle stepped alongside is the build with the situation counters
(tests/step_census.py), so the file also asserts, on this machine, that the cases still reach every reward bin."""
import functools
import os
import tempfile

import numpy as np
import pytest
import torch

import goal_cases as GC
import mask_cases as MC
import reward_cases as R
import step_census as SC
from parity_checks import check_hist, check_occ

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
COPIES = 5
LANES = [0, 64, 16, 4, 1]
OUT_KEYS = ('done', 'reward', 'grid', 'inventory', 'agentPos', 'compass', 'internal')
STATE = (('max_int', 'syn_max_int'), ('dirty', 'dirty'), ('prev_size', 'syn_prev_size'), ('step_no', 'step_no'), ('size', 'size'))
# the query test: checkpoints on both sides of the stale step (2), the completions and the catch-up (7), the second stale
# step (9) and the recount that pays -2 (10)
CHECKPOINTS = (1, 2, 6, 7, 9, 10)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize]) if a.dtype.kind == 'f' else a


@functools.lru_cache(None)
def layout(group):
    """env -> case: every case in COPIES adjacent envs."""
    idx = np.repeat(np.arange(len(R.batch(group)['names'])), COPIES)
    assert group == 'size' or (len(idx) > 64 and len(idx) % 64 != 0)
    return idx


@functools.lru_cache(None)
def truth(group):
    """(every step's outputs and task state of the cases from the counting oracle [T, cases, ...], the reward bins reached)"""
    census = SC.Census(tempfile.mkdtemp(prefix='igw_census_'), coverage=False)
    rec = R.record(census.O, R.batch(group))
    for v in rec.values():
        v.setflags(write=False)
    return rec, census.reward_bins()


@functools.lru_cache(None)
def fixture(group):
    z = np.load(os.path.join(HERE, R.FIXTURE))
    fx = {k[len(group) + 1:]: z[k] for k in z.files if k.startswith(group + '_')}
    fx['grid'] = R.unpack_grids(R.batch(group), fx)
    return fx


def _env(group, lanes, reset=True):
    from gridworld_amd import VecGridWorld
    b, idx = R.batch(group), layout(group)
    env = VecGridWorld(len(idx), autoreset=True, lanes_per_env=lanes, **b['kw'])
    env.set_tasks(b['targets'][idx], b['starts'][idx], full_grids=b['fulls'][idx], invariant=b['invariant'][idx].astype(np.uint8),
                  init_pose=b['poses'][idx])
    if reset:
        env.reset()
    return env


def _actions(group, t=None, device=None):
    a, idx = R.batch(group)['actions'], layout(group)
    return torch.as_tensor(np.ascontiguousarray(a[:, idx] if t is None else a[t][idx]), device=device)


def _outputs(env):
    torch.cuda.synchronize()
    ts = env.task_state()
    return dict(done=env.done.cpu().numpy(), reward=env.reward.cpu().numpy(),
                grid=env.grid.cpu().numpy().reshape(env.num_envs, -1).astype(np.int8), inventory=env.inventory.cpu().numpy(),
                agentPos=env.agent_pos.cpu().numpy(), compass=env.compass.cpu().numpy(), internal=env.internals(),
                **{mine: ts[mine] for mine, _ in STATE})


def _compare_step(group, t, got, names):
    """got == the oracle's step t (every field and the task state, raw bits); == the reference's record where the step did
    not end the episode (the in-kernel auto-reset then shows the next episode's first observation), reward and done
    everywhere."""
    rec, idx, fx = truth(group)[0], layout(group), fixture(group)
    for k, theirs in tuple((k, k) for k in OUT_KEYS) + STATE:
        want = rec[theirs][t][idx]
        bad = (_bits(got[k]).reshape(len(idx), -1) != _bits(want).reshape(len(idx), -1)).any(1)
        assert not bad.any(), f'{group} step {t}: {k} differs from the oracle in envs {np.nonzero(bad)[0][:5]} ({names[idx[bad][0]]}): ' \
                              f'{got[k][bad][0]} vs {want[bad][0]}'
    live = ~got['done'].astype(bool)
    ref = {k: fx[k][idx, t] for k in ('done', 'reward', 'grid', 'inventory', 'agentPos', 'compass', 'internal', 'syn_max_int')}
    assert np.array_equal(got['done'].astype(bool), ref['done'].astype(bool)), f'step {t}: done vs the reference'
    assert np.array_equal(_bits(got['reward']), _bits(ref['reward'].astype(np.float32))), f'step {t}: reward vs the reference'
    for k, theirs in (('grid', 'grid'), ('inventory', 'inventory'), ('agentPos', 'agentPos'), ('compass', 'compass'),
                      ('internal', 'internal'), ('max_int', 'syn_max_int')):
        a, r = _bits(got[k]).reshape(len(idx), -1), _bits(ref[theirs].astype(got[k].dtype)).reshape(len(idx), -1)
        bad = (a != r).any(1) & live
        assert not bad.any(), f'{group} step {t}: {k} differs from the reference in envs {np.nonzero(bad)[0][:5]} ({names[idx[bad][0]]})'


def _final_checks(env, group):
    from test_gpu_parity import _check_index
    b, idx = R.batch(group), layout(group)
    st = env.stats()
    assert st['resets'] >= len(idx) and st['bad_poses'] == st['bad_actions'] == st['bad_tasks'] == 0
    check_occ(env)
    check_hist(env, b['targets'][idx], b['starts'][idx])
    _check_index(env)


@pytest.mark.parametrize('lanes', LANES)
@pytest.mark.parametrize('group', R.GROUPS)
def test_reward_cases_vs_oracle_and_reference(group, lanes):
    """Every group at every lane grouping, compared after every step.  'short' is the auto-reset leg: under a time limit of
    six steps the six-step scripts complete on the very step the time limit ends, the in-step staged reset follows every
    completion, and the episodes after it are compared as well."""
    b = R.batch(group)
    env = _env(group, lanes)
    for t in range(b['T']):
        env.step(_actions(group, t))
        _compare_step(group, t, _outputs(env), b['names'])
    _final_checks(env, group)


@pytest.mark.parametrize('lanes', [0, 4])
@pytest.mark.parametrize('group', ['main', 'short'])
def test_fused_replay_of_the_scripts_equals_stepping(group, lanes):
    """rollout_actions over the same scripts: every step's reward and done and the buffers it leaves are those of stepping."""
    b = R.batch(group)
    rec, idx = truth(group)[0], layout(group)
    a, s = _env(group, lanes), _env(group, lanes)
    rw, dn = a.rollout_actions(_actions(group, device=a.device), return_rewards=True)
    for t in range(b['T']):
        s.step(_actions(group, t))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(rw.cpu().numpy()), _bits(rec['reward'][:, idx])) and np.array_equal(dn.cpu().numpy(), rec['done'][:, idx])
    for name in ('grid_buf', 'occ_buf', 'hist_buf', 'agent_buf', 'aux_buf', 'agent_pos', 'inventory', 'compass', 'reward', 'done'):
        assert torch.equal(getattr(a, name), getattr(s, name)), name
    sa, ss = a.stats(), s.stats()
    assert sa['changed'] == ss['changed'] and sa['resets'] == ss['resets'] and sa['rescans'] == ss['rescans']
    _compare_step(group, b['T'] - 1, _outputs(a), b['names'])
    _final_checks(a, group)


@pytest.mark.parametrize('group', ['main', 'short'])
def test_episode_log_variant_logs_the_reference_episodes(group):
    """The EXTRA kernel variant (episode log on for the first envs): the same outputs at every step, and every episode
    it logs is the episode the reference played -- all of its steps, the last one's own observation included."""
    from gridworld_amd.wrappers import EpisodeLogger
    b, idx, fx = R.batch(group), layout(group), fixture(group)
    n_logged = 60
    env = _env(group, 0, reset=False)
    log = EpisodeLogger(env, n_envs=n_logged, capacity=b['kw']['max_steps'])
    env.reset()
    eps = []
    for t in range(b['T']):
        env.step(_actions(group, t))
        if t % 4 == 3 or t == b['T'] - 1:
            _compare_step(group, t, _outputs(env), b['names'])
            eps += log.collect(dump=False)
    env.disable_trajectory_log()
    assert len(eps) >= n_logged and {e['env'] for e in eps} == set(range(n_logged))
    for ep in eps:
        i = idx[ep['env']]
        starts = np.concatenate([[0], np.nonzero(fx['reset_before'][i])[0], [b['T']]])
        lo, hi = starts[ep['episode'] - 1], starts[ep['episode']]
        assert fx['done'][i, hi - 1] and len(ep['reward']) == hi - lo, (b['names'][i], ep['episode'])
        where = f"{b['names'][i]} episode {ep['episode']}"
        assert np.array_equal(_bits(ep['reward'].astype(np.float32)), _bits(fx['reward'][i, lo:hi].astype(np.float32))), where
        assert np.array_equal(ep['done'], fx['done'][i, lo:hi].astype(bool)), where
        assert np.array_equal(_bits(ep['agentPos'][1:]), _bits(fx['agentPos'][i, lo:hi])) and not ep['agentPos'][0].any(), where
        assert np.array_equal(_bits(ep['compass'][1:, 0]), _bits(fx['compass'][i, lo:hi])), where
        assert np.array_equal(ep['inventory'][1:], fx['inventory'][i, lo:hi]), where
        assert np.array_equal(ep['grid'].reshape(hi - lo + 1, -1)[1:], fx['grid'][i, lo:hi]), where
        assert np.array_equal(ep['grid'].reshape(hi - lo + 1, -1)[0], b['starts'][i].reshape(-1)), where


def test_task_eval_on_every_changed_step():
    """task_eval_kernel on (synthetic target, synthetic grid) of every step that changed a grid, against the oracle's
    Task evaluation: maximal intersection, argmax (the reference's iteration order breaks the ties) and target size."""
    from gridworld_amd import task_eval
    from oracle import oracle as O
    b, grids = R.batch('main'), fixture('main')['grid']     # (the reference's record: a step that ends the episode shows its own grid)
    n = len(b['names'])
    start = b['starts'].reshape(n, -1)
    prev = np.concatenate([start[:, None], grids[:, :-1]], axis=1)
    cc, tt = np.nonzero((grids != prev).any(2))            # (a reset back to the start grid counts as well)
    syn_t = (b['targets'].reshape(n, -1) - start)[cc]
    syn_g = grids[cc, tt] - start[cc]
    assert len(tt) > 100 and (syn_t < 0).any() and (syn_g < 0).any()
    mi, am, ts = task_eval(syn_t, syn_g)
    want = [O.task_eval(syn_t[k], syn_g[k]) for k in range(len(tt))]
    for k, w in enumerate(want):
        where = f"{b['names'][cc[k]]} step {tt[k]}"
        assert mi[k] == w['max_int'] and ts[k] == w['target_size'], where
        assert np.array_equal(am[k], w['argmax']), where + f" argmax {am[k]} vs {w['argmax']}"
    assert len({tuple(w['argmax']) for w in want}) > 8 and {int(w['argmax'][2]) for w in want if w['max_int']} == {0, 1, 2, 3}


@pytest.mark.parametrize('group', ['main', 'size'])
def test_user_tasks_env_max_int_and_task_eval(group):
    """prepare_tasks_kernel's GridWorld.max_int and task_eval_kernel on the user tasks (target, start; the full-grid and the
    non-invariant case included) against the oracle's Task evaluation and the reference's record."""
    from gridworld_amd import task_eval
    from oracle import oracle as O
    b, idx = R.batch(group), layout(group)
    want = R.user_task_truth(O, b)
    env = _env(group, 0, reset=False)
    torch.cuda.synchronize()
    got = env.task_meta.cpu().numpy()[:, 42:44].copy().view(np.int16)[:, 0]
    assert np.array_equal(got, want['max_int'][idx]) and np.array_equal(got, fixture(group)['env_max_int'][idx])
    for flag in (False, True):
        m = b['invariant'] == flag
        if m.any():
            mi, am, ts = task_eval(b['targets'][m], b['starts'][m], full_grids=b['fulls'][m], invariant=flag)
            assert np.array_equal(mi, want['max_int'][m]) and np.array_equal(am, want['argmax'][m]) and np.array_equal(ts, want['target_size'][m])
    if group == 'main':
        narrowed = b['names'].index('full_grid_narrows')
        own = O.task_eval(b['targets'][narrowed], b['starts'][narrowed])
        full = O.task_eval(b['targets'][narrowed], b['starts'][narrowed], full_grid=b['fulls'][narrowed])
        assert full['adm_count'].sum() < own['adm_count'].sum()
    else:
        assert (want['max_int'] > 0).any() and (want['max_int'] == 0).any()


def _query_case(keep=None):
    """The main group in the case format of tests/mask_cases.py (one env per case, or those of `keep`)."""
    b = R.batch('main')
    keep = np.ones(len(b['names']), bool) if keep is None else keep
    return dict(kw=b['kw'], targets=b['targets'][keep], starts=b['starts'][keep], poses=b['poses'][keep],
                actions=np.ascontiguousarray(b['actions'][:, keep]))


def _query_env(case, log=None):
    """The case's envs without auto-reset (the truth functions step without it), reset."""
    from gridworld_amd import VecGridWorld
    env = VecGridWorld(len(case['targets']), **case['kw'])
    env.set_tasks(case['targets'], case['starts'], init_pose=case['poses'])
    out = env.enable_trajectory_log(len(case['targets']), log) if log else None
    env.reset()
    return (env,) + tuple(out) if log else env


def _at_checkpoints(case, ask):
    """{output: [per checkpoint]} of ask(env) on the case's envs after 1, 2, 6, 7, 9 and 10 of their actions."""
    env, t, got = _query_env(case), 0, {}
    acts = torch.from_numpy(case['actions']).to(env.device)
    for tc in CHECKPOINTS:
        while t < tc:
            env.step(acts[t])
            t += 1
        for k, v in ask(env).items():
            got.setdefault(k, []).append(v.cpu().numpy())
    return {k: np.stack(v) for k, v in got.items()}


def _differing(got, want, names):
    """{output: [(checkpoint, cases)]} where the bits differ; shapes and types must agree."""
    bad = {}
    for k in got:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (k, got[k].shape, want[k].shape, got[k].dtype, want[k].dtype)
        C, n = got[k].shape[:2]
        d = (_bits(got[k]).reshape(C, n, -1) != _bits(want[k]).reshape(C, n, -1)).any(2)
        for c in np.nonzero(d.any(1))[0]:
            bad.setdefault(k, []).append((CHECKPOINTS[c], [names[i] for i in np.nonzero(d[c])[0]][:6]))
    return bad


def test_action_mask_at_the_reward_checkpoints():
    """action_mask(look=True) on every case of the main group (none is left out of the query leg) at checkpoints on both
    sides of the stale steps, the completions and the catch-up recounts: the oracle truth of tests/mask_cases.py."""
    case, names = _query_case(), R.batch('main')['names']
    masks, looks = MC.truth_of(case, CHECKPOINTS)

    def ask(env):
        mask, look = env.action_mask(look=True)
        return dict(mask=mask, look=look)
    bad = _differing(_at_checkpoints(case, ask), dict(mask=masks, look=looks), names)
    assert not bad, bad
    assert (looks == -1).any() and (looks >= 0).any() and (masks[:, :, 16] == 0).any() and (masks[:, :, 17] == 0).any()


def test_goal_query_at_the_reward_checkpoints():
    """goal(want, todo, gain) there: the oracle truth of tests/goal_cases.py.  The checkpoints do see a cached maximum
    below and above the live one, probes that pay +2 and -2 and probes that end the episode."""
    case, names = _query_case(), R.batch('main')['names']
    goal = GC.truth_of(case, CHECKPOINTS)
    got = _at_checkpoints(case, lambda env: env.goal(want=True, todo=True, gain=True))
    bad = _differing(got, {k: goal[k] for k in got}, names)
    assert not bad, bad
    fit = goal['fit']     # live maximum, target size, blocks, cached maximum
    assert (fit[..., 0] > fit[..., 3]).any() and (fit[..., 0] < fit[..., 3]).any()
    assert (goal['gain'] >= 2).any() and (goal['gain'] <= -2).any() and goal['ends'].any()


def test_worth_query_at_the_reward_checkpoints():
    """worth() there: every word and `best` against the numpy model of tests/worth_model.py on the oracle's states."""
    import worth_cases as WC
    import worth_model as WM
    case, names = _query_case(), R.batch('main')['names']
    n = len(names)
    model = WC.model_of(case, WC.states_of(case, CHECKPOINTS))
    words = np.stack([np.stack([m['word'] for m in row]) for row in model])
    best = np.stack([np.stack([WM.best_of(words[c, i], WC.RIGHT, WC.WRONG) for i in range(n)]) for c in range(len(CHECKPOINTS))])

    def ask(env):
        res = env.worth()
        return dict(word=torch.as_strided(res['word'], (n, 7, 1104), (7 * 1104, 1104, 1)), best=res['best'])
    bad = _differing(_at_checkpoints(case, ask), dict(word=words, best=best.astype(np.int32)), names)
    assert not bad, bad


PEEK_AT, PEEK_H = (1, 6, 9), 8


def test_peek_query_through_the_interesting_steps():
    """peek() of 18 candidates per env -- each action, then the next seven of the case's own script -- from just after the
    break of the start block (the candidates walk through the stale step and the catch-up), from just before the
    completions and from the second stale step (through the recount that pays -2): the stepped oracle of
    tests/peek_cases.py, all five outputs."""
    import peek_cases as PC
    case, names = _query_case(), R.batch('main')['names']
    n = len(names)
    env, t, bad = _query_env(case), 0, {}
    acts = torch.from_numpy(case['actions']).to(env.device)
    for tc in PEEK_AT:
        while t < tc:
            env.step(acts[t])
            t += 1
        cand = np.zeros((n, 18, PEEK_H), np.int32)
        cand[:, :, 0] = np.arange(18)
        cand[:, :, 1:] = case['actions'][tc + 1:tc + PEEK_H].T[:, None]
        want = PC.truth_of(case, tc, cand)
        for gamma in PC.GAMMAS:
            res = {k: v.cpu().numpy() for k, v in env.peek(torch.from_numpy(cand).to(env.device), gamma=gamma).items()}
            for k, v in res.items():
                w = want['ret'][gamma] if k == 'ret' else want[k]
                assert v.shape == w.shape and v.dtype == w.dtype, k
                d = (_bits(v).reshape(n, -1) != _bits(w).reshape(n, -1)).any(1)
                if d.any():
                    bad.setdefault(k, []).append((tc, gamma, [names[i] for i in np.nonzero(d)[0]][:6]))
        if tc == 1:
            assert (want['reward'] >= 2).any() and (want['ends'] > 0).any()
        if tc == 9:
            assert (want['reward'] <= -2).any()
    assert not bad, bad


def test_relabel_query_under_own_final_and_at0():
    """The logged episodes of the cases relabelled under their own target, their final grid and their starting grid (an
    empty synthetic target): reward, done, progress, end and target size of the oracle stepped under each goal
    (tests/relabel_cases.py).  The format holds 48 steps: the cases whose script is longer are left out of this query,
    at most a quarter of them."""
    import gridworld_amd as G
    import relabel_cases as RC
    from test_gpu_relabel import CAP, _episodes, _rows, _same
    b = R.batch('main')
    keep = np.array([len(c['actions']) <= RC.T and c['name'] != 'complete_at_max_steps' for c in R.cases() if c['group'] == 'main'])
    assert len(keep) == len(b['names']) and (~keep).sum() <= len(keep) // 4
    case = _query_case(keep)
    n, T = int(keep.sum()), RC.T
    base = RC.run(case, case['targets'])
    starts = case['starts'].reshape(n, -1)
    goals = np.stack([case['targets'].reshape(n, -1), base['grids'][T], starts], 1)      # own, final, at0
    runs = [RC.run(case, goals[:, g].reshape(n, 9, 11, 11)) for g in range(3)]
    pad = lambda k: np.concatenate([np.stack([r[k] for r in runs], 1), np.zeros((n, 3, CAP - T), runs[0][k].dtype)], 2)  # noqa: E731
    want = dict(reward=pad('reward'), done=pad('done'), progress=pad('progress'),
                end=RC.end_of(np.stack([r['done'] for r in runs], 1)),
                target_size=np.count_nonzero(goals - starts[:, None], axis=2).astype(np.int16))
    assert (want['end'][:, 0] > 0).sum() >= 10 and (want['end'][:, 2] == 1).all() and (want['reward'] >= 2).any() and (want['reward'] <= -2).any()
    env, rec, heads = _query_env(case, log=CAP)
    acts = torch.from_numpy(case['actions']).to(env.device)
    for t in range(T):
        env.step(acts[t])
    first, length = _episodes(heads, CAP)
    assert (length == T).all()
    kw = dict(right_scale=RC.RIGHT, wrong_scale=RC.WRONG, max_steps=case['kw']['max_steps'], outputs=tuple(want))
    _same(G.relabel(rec, first, length, _rows(starts, env.device), targets=_rows(goals, env.device), **kw), want, 'targets')
    at = torch.tensor([[T, 0]] * n, dtype=torch.int32, device=env.device)       # final and at0 as entries of the episode itself
    _same(G.relabel(rec, first, length, _rows(starts, env.device), at=at, **kw), {k: v[:, 1:] for k, v in want.items()}, 'at')


def test_the_cases_still_reach_every_reward_situation():
    """The census floor, on this machine: the oracle stepped alongside the kernel counted its reward situations; every bin
    is reached by the groups except those reward_cases.UNREACHABLE names.  An edit to a script that stops reaching its bin
    fails here."""
    total = {}
    for group in R.GROUPS:
        for k, v in truth(group)[1].items():
            total[k] = total.get(k, 0) + v
    unreached = {k for k, v in total.items() if v == 0}
    assert unreached == {k for k in R.UNREACHABLE if ' | ' not in k}, sorted(unreached)
    assert len(total) >= 120
