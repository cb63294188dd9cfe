"""The step kernel on the directed cases of tests/step_cases.py: the situations random walks do not reach (every side of
a block on every level, the zone's walls, floor and ceiling, agents outside the zone and far below it where every
occupancy key is clamped, terminal velocity, head bumps, rounding ties, flying with a vertical strafe ...).

One batch per action space, the cases repeated and permuted (every case at several lanes of a wavefront, a ragged last
wave), stepped with the in-kernel auto-reset at every lane grouping.  After EVERY step all outputs and the float64
internals are compared as raw bits with the CPU oracle stepped alongside, and with tests/golden/s14_step_cases.npz -- the
same cases as the Python reference played them.  0 mismatches allowed anywhere.  The oracle stepped alongside is the
build with the situation counters (tests/step_census.py), so the file also asserts, on this machine, that the cases
still reach every situation bin."""
import functools
import os
import tempfile

import numpy as np
import pytest
import torch

import goal_cases as GC
import mask_cases as MC
import step_cases as K
import step_census as SC
from parity_checks import check_hist, check_occ

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPEATS = {'walking': 3, 'flying': 23}
LANES = [0, 64, 16, 4, 1]
CHECKPOINTS = (0, 3, 14)   # of the query test
# ... and its cases: agents outside the zone, under the ground, at the walls and the ceiling, on rounding ties
QUERY_CASES = ('wall_', 'under_ground', 'outside_', 'ring_', 'corner_', 'tower_', 'above_', 'tie_', 'diagonal', 'empty_slot',
               'jump_under', 'head_in', 'legs_in', 'face_top_level7', 'face_xlo_level7', 'face_bottom_level0', 'face_zhi_level-1')
OUT_KEYS = ('done', 'reward', 'grid', 'inventory', 'agentPos', 'compass', 'internal')


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize]) if a.dtype.kind == 'f' else a


@functools.lru_cache(None)
def layout(space):
    """env -> case: REPEATS permutations of the cases, one after the other (> 64 envs, no multiple of 64)."""
    n = len(K.batch(space)['names'])
    rng = np.random.RandomState(14)
    idx = np.concatenate([rng.permutation(n) for _ in range(REPEATS[space])])
    assert len(idx) > 64 and len(idx) % 64 != 0
    return idx


@functools.lru_cache(None)
def truth(space):
    """(every step's outputs of the cases from the counting oracle [T, cases, ...], the situation bins reached)"""
    census = SC.Census(tempfile.mkdtemp(prefix='igw_census_'), coverage=False)
    rec = K.record(census.O, K.batch(space))
    for v in rec.values():
        v.setflags(write=False)
    return rec, census.bins()


def _env(space, lanes, reset=True):
    from gridworld_amd import VecGridWorld
    b, idx = K.batch(space), layout(space)
    env = VecGridWorld(len(idx), autoreset=True, lanes_per_env=lanes, **b['kw'])
    env.set_tasks(b['targets'][idx], b['starts'][idx], init_pose=b['poses'][idx])
    if reset:
        env.reset()
    return env


def _actions(space, t=None, device=None):
    b, idx = K.batch(space), layout(space)
    a = b['actions']
    pick = (lambda v: v[:, idx]) if t is None else (lambda v: v[t][idx])
    if isinstance(a, dict):
        return {k: torch.as_tensor(np.ascontiguousarray(pick(v)), device=device) for k, v in a.items()}
    return torch.as_tensor(np.ascontiguousarray(pick(a)), device=device)


def _outputs(env):
    torch.cuda.synchronize()
    return dict(done=env.done.cpu().numpy(), reward=env.reward.cpu().numpy(),
                grid=env.grid.cpu().numpy().reshape(env.num_envs, -1).astype(np.int8), inventory=env.inventory.cpu().numpy(),
                agentPos=env.agent_pos.cpu().numpy(), compass=env.compass.cpu().numpy(), internal=env.internals())


def _fixture(space):
    z = np.load(os.path.join(HERE, K.FIXTURE))
    return {k[len(space) + 1:]: z[k] for k in z.files if k.startswith(space + '_')}


def _compare_step(space, t, got, names):
    """got == the oracle's step t (every field, raw bits); == the reference's record where the step did not end the
    episode (the in-kernel auto-reset then shows the next episode's first observation), reward and done everywhere."""
    rec, idx, fx = truth(space)[0], layout(space), _fixture(space)
    for k in OUT_KEYS:
        want = rec[k][t][idx]
        bad = (_bits(got[k]).reshape(len(idx), -1) != _bits(want).reshape(len(idx), -1)).any(1)
        assert not bad.any(), f'step {t}: {k} differs from the oracle in envs {np.nonzero(bad)[0][:5]} ({names[idx[bad][0]]})'
    live = ~got['done'].astype(bool)
    ref = {k: fx[k][idx, t] for k in ('done', 'reward', 'grid', 'inventory', 'agentPos', 'compass', 'internal')}
    assert np.array_equal(got['done'].astype(bool), ref['done'].astype(bool)), f'step {t}: done vs the reference'
    assert np.array_equal(_bits(got['reward']), _bits(ref['reward'].astype(np.float32))), f'step {t}: reward vs the reference'
    for k in ('grid', 'inventory', 'agentPos', 'compass', 'internal'):
        a, r = _bits(got[k]).reshape(len(idx), -1), _bits(ref[k].astype(got[k].dtype)).reshape(len(idx), -1)
        bad = (a != r).any(1) & live
        assert not bad.any(), f'step {t}: {k} differs from the reference in envs {np.nonzero(bad)[0][:5]} ({names[idx[bad][0]]})'


@pytest.mark.parametrize('lanes', LANES)
@pytest.mark.parametrize('space', ['walking', 'flying'])
def test_directed_cases_vs_oracle_and_reference(space, lanes):
    b, idx = K.batch(space), layout(space)
    env = _env(space, lanes)
    for t in range(b['T']):
        env.step(_actions(space, t))
        _compare_step(space, t, _outputs(env), b['names'])
    st = env.stats()
    assert st['resets'] >= len(idx) and st['bad_poses'] == st['bad_actions'] == st['bad_tasks'] == 0
    check_occ(env)
    check_hist(env, b['targets'][idx], b['starts'][idx])


@pytest.mark.parametrize('lanes', [0, 4])
@pytest.mark.parametrize('space', ['walking', 'flying'])
def test_fused_replay_of_the_scripts_equals_stepping(space, lanes):
    """rollout_actions (igw_rollout_walking_actions / igw_rollout_flying_actions) over the same scripts: every step's
    reward and done and the buffers it leaves are those of stepping."""
    b = K.batch(space)
    rec, idx = truth(space)[0], layout(space)
    a, s = _env(space, lanes), _env(space, lanes)
    rw, dn = a.rollout_actions(_actions(space, device=a.device), return_rewards=True)
    for t in range(b['T']):
        s.step(_actions(space, t))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(rw.cpu().numpy()), _bits(rec['reward'][:, idx])) and np.array_equal(dn.cpu().numpy(), rec['done'][:, idx])
    for name in ('grid_buf', 'occ_buf', 'hist_buf', 'agent_buf', 'agent_pos', 'inventory', 'compass', 'reward', 'done'):
        assert torch.equal(getattr(a, name), getattr(s, name)), name
    sa, ss = a.stats(), s.stats()
    assert sa['changed'] == ss['changed'] and sa['resets'] == ss['resets'] and sa['rescans'] == ss['rescans']
    _compare_step(space, b['T'] - 1, _outputs(a), b['names'])


@pytest.mark.parametrize('space', ['walking', 'flying'])
def test_episode_log_variant_logs_the_reference_episodes(space):
    """The EXTRA kernel variant (episode log on for the first envs): the same outputs at every step, and every episode
    it logs is the episode the reference played -- all of its steps, the last one's own observation included."""
    from gridworld_amd.wrappers import EpisodeLogger
    b, idx, fx = K.batch(space), layout(space), _fixture(space)
    n_logged = 40
    env = _env(space, 0, reset=False)
    log = EpisodeLogger(env, n_envs=n_logged, capacity=b['kw']['max_steps'])
    env.reset()
    eps = []
    for t in range(b['T']):
        env.step(_actions(space, t))
        if t % 8 == 7 or t == b['T'] - 1:
            _compare_step(space, t, _outputs(env), b['names'])
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


def test_mask_and_goal_queries_on_the_walking_cases():
    """action_mask() and goal(gain=True) march the step's ray over the same clamped keys: at steps where agents are
    outside the zone, under the ground and at the ceiling they must equal the oracle truth of tests/mask_cases.py and
    tests/goal_cases.py (nine oracle blocks per checkpoint: the base and eight probes).  Envs whose episode has ended
    before a checkpoint are left out there (the truth steps without auto-reset)."""
    b, idx = K.batch('walking'), layout('walking')
    rec = truth('walking')[0]
    sel = np.array([i for i, name in enumerate(b['names']) if name.startswith(QUERY_CASES)])
    assert len(sel) >= 25
    sub = dict(kw=b['kw'], targets=b['targets'][sel], starts=b['starts'][sel], poses=b['poses'][sel], actions=b['actions'][:, sel])
    masks, looks = MC.truth_of(sub, CHECKPOINTS)
    goal = GC.truth_of(sub, CHECKPOINTS)
    row = np.full(len(b['names']), -1)
    row[sel] = np.arange(len(sel))
    asked, rows = row[idx] >= 0, row[idx].clip(0)       # per env: is its case one of the query cases, and which
    env = _env('walking', 0)
    t, bad, compared = 0, {}, 0
    for c, tc in enumerate(CHECKPOINTS):
        while t < tc:
            env.step(_actions('walking', t))
            t += 1
        alive = ~rec['done'][:tc].astype(bool).any(0)[idx] & asked
        assert alive.sum() >= 0.8 * asked.sum() > 60
        mask, look = env.action_mask(look=True)
        res = {k: v.cpu().numpy() for k, v in env.goal(want=True, todo=True, gain=True).items()}
        got = dict(res, mask=mask.cpu().numpy(), look=look.cpu().numpy())
        want = dict({k: goal[k][c][rows] for k in res}, mask=masks[c][rows], look=looks[c][rows])
        for k in got:
            assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
            d = (_bits(got[k]).reshape(len(idx), -1) != _bits(want[k]).reshape(len(idx), -1)).any(1) & alive
            if d.any():
                bad.setdefault(k, []).append((tc, [b['names'][i] for i in sorted(set(idx[d]))][:6]))
        compared += int(alive.sum())
    print(f'{compared} (env, checkpoint) pairs compared; differing: {bad}')
    assert not bad
    # the checkpoints do see the situations they are there for
    inv = rec['internal'][[tc - 1 for tc in CHECKPOINTS[1:]]][:, sel]
    assert (np.abs(inv[..., 0]) > 6.5).any() and (inv[..., 1] < -4.5).any() and (inv[..., 1] > 7.5).any()
    assert (looks == -1).any() and (looks >= 0).any() and (masks[:, :, 17] == 0).any()


def test_the_cases_still_reach_every_situation():
    """The census floor, on this machine: the oracle stepped alongside the kernel counted its situations; every bin is
    reached by the two batches except those step_cases.UNREACHABLE names."""
    total = {}
    for space in ('walking', 'flying'):
        for k, v in truth(space)[1].items():
            total[k] = total.get(k, 0) + v
    unreached = {k for k, v in total.items() if v == 0}
    assert unreached == {k for k in K.UNREACHABLE if ' | ' not in k}, sorted(unreached)
    assert len(total) > 120
