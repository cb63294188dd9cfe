"""Recorded reference side of tests/scenario_fuzz.py scenarios (test infrastructure).

RecordingBackend wraps a live backend (the imported Python reference, tests/golden/fuzz_ref_vs_oracle.py) and writes
down, per scenario, everything run_scenario reads from the env: every reset's and every step's observation, reward,
done, float64 internals, synthetic-task counters, GridWorld.max_int / step_no, and the task (target, starting grid,
full_grid, invariant) it hands to the oracle at every reset.  ReplayBackend serves those records back in the same
order, so run_scenario steps the live CPU oracle against the reference's recorded outputs -- every field on every
step, bit for bit, as in the live run -- without the reference being present.

Storage (one .npz, tests/golden/gen_ref_fuzz.py): per record kind a row per event; grids as indices into one table
of distinct int8 grids; float bit patterns XOR-ed with the previous row of the same stream (they change little from
step to step, so the archive compresses well)."""
import numpy as np

OBS_F32 = 6          # agentPos (5), compass (1)
INT_COLS = 11        # inventory (6), syn max_int, syn prev_size, env max_int, step_no, done
TASK_COLS = 5        # target grid id, full grid id (-1 = none), invariant (-1 = None), len(admissible), start rows


class _Grids:
    def __init__(self):
        self.ids, self.rows = {}, []

    def add(self, g):
        g = np.ascontiguousarray(np.asarray(g).reshape(9, 11, 11), dtype=np.int8)
        key = g.tobytes()
        if key not in self.ids:
            self.ids[key] = len(self.rows)
            self.rows.append(g)
        return self.ids[key]


def _sparse(start):
    return np.asarray([[int(v) for v in b] for b in (start if start is not None else [])], np.int32).reshape(-1, 4)


def _xor_delta(bits):
    out = bits.copy()
    out[1:] ^= bits[:-1]
    return out


def _xor_undo(bits):
    return np.bitwise_xor.accumulate(bits, axis=0)


# ------------------------------------------------------------------------------------------------ recording
class _RecordingEnv:
    def __init__(self, env, rec, backend):
        self.env, self.rec, self.backend = env, rec, backend

    def __getattr__(self, name):
        return getattr(self.env, name)

    def initialize_world(self, starting_grid, pose):
        # run_scenario has just read the task's target and starting grid for this call: keep them
        u = self.env.unwrapped
        self.rec['pre_task'] = (None if u._task is None else np.asarray(u._task.target_grid), _sparse(u.starting_grid))
        return self.env.initialize_world(starting_grid, pose)

    def _state(self, obs, reward=0.0, done=False):
        u = self.env.unwrapped
        smi, sps = self.backend.syn(self.env)
        return dict(obs=obs, reward=float(reward), done=bool(done), internal=list(self.backend.internals(self.env)),
                    syn=(int(smi), int(sps)), max_int=int(u.max_int), step_no=int(u.step_no))

    def reset(self):
        obs = self.env.reset()
        u = self.env.unwrapped
        task = u._task
        inv = getattr(task, 'invariant', None)
        self.rec['events'].append(('reset', self._state(obs), dict(
            target=np.asarray(task.target_grid), full=getattr(task, 'full_grid', None),
            invariant=None if inv is None else bool(inv), admissible=len(task.admissible), start=_sparse(u.starting_grid))))
        return obs

    def step(self, action):
        obs, reward, done, info = self.env.step(action)
        self.rec['events'].append(('step', self._state(obs, reward, done), None))
        return obs, reward, done, info


class RecordingBackend:
    """Forwards to `live` and records what run_scenario reads into the dict begin() returns (one per scenario)."""

    def __init__(self, live):
        self.live = live
        self.name = live.name
        self.float32_actions = live.float32_actions
        self.Task, self.Subtasks, self.CustomTasks, self.RandomTasks = live.Task, live.Subtasks, live.CustomTasks, live.RandomTasks
        self.current = None

    def begin(self):
        self.current = dict(pre_task=None, events=[])
        return self.current

    def make(self, kw):
        return _RecordingEnv(self.live.make(kw), self.current, self.live)

    def goals(self):
        return self.live.goals()

    def trig(self, crlibm):
        return self.live.trig(crlibm)

    def oracle_device_trig(self, crlibm):
        return self.live.oracle_device_trig(crlibm)

    def internals(self, env):
        return self.live.internals(env.env)

    def syn(self, env):
        return self.live.syn(env.env)


def pack(records):
    """records: [(seed, record)] -> dict of arrays (np.savez_compressed)."""
    grids = _Grids()
    seeds, ev_lo, pre = [], [], []
    f32, f64, ints, gid, rew = [], [], [], [], []
    kinds, task_rows, starts = [], [], []
    for seed, rec in records:
        seeds.append(seed)
        ev_lo.append(len(kinds))
        if rec['pre_task'] is None:
            pre.append((-1, -1, -1))
        else:
            tg, st = rec['pre_task']
            pre.append((-1 if tg is None else grids.add(tg), sum(len(s) for s in starts), len(st)))
            starts.append(st)
        for kind, s, task in rec['events']:
            o = s['obs']
            for key in ('inventory', 'grid'):    # integer-valued in the reference: stored as integers
                v = np.asarray(o[key])
                if not np.array_equal(v, np.asarray(v, np.int64)) or np.abs(v).max(initial=0) > 127:
                    raise ValueError(f'{key} is not a small integer array')
            kinds.append(0 if kind == 'reset' else 1)
            f32.append(np.concatenate([np.asarray(o['agentPos'], np.float32).reshape(5), np.asarray(o['compass'], np.float32).reshape(1)]))
            f64.append(np.asarray(s['internal'], np.float64))
            rew.append(s['reward'])
            ints.append(np.concatenate([np.asarray(o['inventory'], np.int64).reshape(6),
                                        [s['syn'][0], s['syn'][1], s['max_int'], s['step_no'], int(s['done'])]]))
            gid.append(grids.add(o['grid']))
            if task is not None:
                full = task['full']
                task_rows.append((grids.add(task['target']), -1 if full is None else grids.add(full),
                                  -1 if task['invariant'] is None else int(task['invariant']), task['admissible'],
                                  len(task['start'])))
                starts.append(task['start'])
    ev_lo.append(len(kinds))
    return dict(seeds=np.asarray(seeds, np.int64), event_lo=np.asarray(ev_lo, np.int64),
                pre_task=np.asarray(pre, np.int64).reshape(-1, 3), kinds=np.asarray(kinds, np.int8),
                obs_f32_xor=np.ascontiguousarray(_xor_delta(np.asarray(f32, np.float32).reshape(-1, OBS_F32).view(np.uint32)).T),
                internal_xor=np.ascontiguousarray(_xor_delta(np.asarray(f64, np.float64).reshape(-1, 8).view(np.uint64)).T),
                reward=np.asarray(rew, np.float64), ints=np.asarray(ints, np.int32).reshape(-1, INT_COLS),
                grid_id=np.asarray(gid, np.int32), tasks=np.asarray(task_rows, np.int32).reshape(-1, TASK_COLS),
                starts=np.concatenate(starts + [np.zeros((0, 4), np.int32)]).astype(np.int16),
                grids=np.asarray(grids.rows, np.int8).reshape(-1, 9, 11, 11))


# ------------------------------------------------------------------------------------------------ replay
class _Task:
    def __init__(self, target, full, invariant, admissible):
        self.target_grid, self.full_grid, self.invariant = target, full, invariant
        self.admissible = [None] * admissible


class _ReplayEnv:
    """What run_scenario reads from a gym env, served from the records of one scenario."""

    def __init__(self, data, scenario):
        self.d, self.k = data, scenario
        self.i = int(data['event_lo'][scenario])
        self.end = int(data['event_lo'][scenario + 1])
        self.unwrapped = self
        self.max_int = self.step_no = 0
        self.syn = (0, 0)
        self.internal = None
        tg, lo, n = (int(v) for v in data['pre_task'][scenario])
        self._task = None if tg < 0 else _Task(data['grids'][tg].astype(np.int32), None, None, 4)
        self.starting_grid = None if lo < 0 else [tuple(int(v) for v in r) for r in data['starts'][lo:lo + n]]
        # task rows of this scenario: the resets before it in the archive
        self.task_i = int(np.count_nonzero(data['kinds'][:self.i] == 0))

    def set_task(self, task):
        pass

    def set_task_generator(self, gen):
        pass

    def initialize_world(self, starting_grid, pose):
        pass

    def _next(self, kind):
        d, i = self.d, self.i
        if i >= self.end or int(d['kinds'][i]) != kind:
            raise RuntimeError('replay out of step with the recording (scenario %d, event %d)' % (self.k, i))
        self.i += 1
        f = d['obs_f32'][i]
        ints = d['ints'][i]
        obs = {'agentPos': f[:5].copy(), 'compass': f[5:6].copy(), 'inventory': ints[:6].astype(np.float32),
               'grid': d['grids'][d['grid_id'][i]].astype(np.int32)}
        self.internal = [float(x) for x in d['internal'][i]]
        self.syn = (int(ints[6]), int(ints[7]))
        self.max_int, self.step_no = int(ints[8]), int(ints[9])
        return obs, float(d['reward'][i]), bool(ints[10])

    def reset(self):
        obs, _, _ = self._next(0)
        d = self.d
        tg, fg, inv, adm, n = (int(v) for v in d['tasks'][self.task_i])
        self._task = _Task(d['grids'][tg].astype(np.int32), None if fg < 0 else d['grids'][fg].astype(np.int32),
                           None if inv < 0 else bool(inv), adm)
        lo = int(d['starts_lo'][self.task_i])
        self.starting_grid = [tuple(int(v) for v in r) for r in d['starts'][lo:lo + n]]
        self.task_i += 1
        return obs

    def step(self, action):
        obs, reward, done = self._next(1)
        return obs, reward, done, {}


class _Stub:
    def __init__(self, *a, **k):
        pass


class ReplayBackend:
    """The reference as recorded (tests/golden/s13_ref_fuzz.npz): the oracle is live, the reference is data."""
    name = 'reference (recorded)'
    float32_actions = False
    Task = Subtasks = CustomTasks = RandomTasks = _Stub

    def __init__(self, path, goals):
        z = np.load(path)
        d = {k: z[k] for k in z.files}
        d['obs_f32'] = np.ascontiguousarray(_xor_undo(d.pop('obs_f32_xor').T)).view(np.float32)
        d['internal'] = np.ascontiguousarray(_xor_undo(d.pop('internal_xor').T)).view(np.float64)
        # rows of `starts`, in archive order: per scenario its pre-reset starting grid (if recorded), then one block per
        # reset; starts_lo[k] = first row of reset k's block
        lo, pos, k = [], 0, 0
        for sc in range(len(d['seeds'])):
            _, a, n = (int(v) for v in d['pre_task'][sc])
            if a >= 0:
                pos = a + n
            for _ in range(int(np.count_nonzero(d['kinds'][d['event_lo'][sc]:d['event_lo'][sc + 1]] == 0))):
                lo.append(pos)
                pos += int(d['tasks'][k][4])
                k += 1
        d['starts_lo'] = np.asarray(lo, np.int64)
        self.d = d
        self.index = {int(s): i for i, s in enumerate(d['seeds'])}
        self._goals = goals
        self._scenario = None

    def seeds(self):
        return [int(s) for s in self.d['seeds']]

    def select(self, seed):
        self._scenario = self.index[int(seed)]

    def make(self, kw):
        self.env = _ReplayEnv(self.d, self._scenario)
        return self.env

    def replayed_all(self):
        """True when the last scenario consumed every recorded event (run_scenario asked for no more, no fewer)."""
        return self.env.i == self.env.end

    def goals(self):
        return self._goals

    def trig(self, crlibm):
        import contextlib
        return contextlib.nullcontext()

    def oracle_device_trig(self, crlibm):
        return bool(crlibm)      # as against the live reference: correctly rounded reference <-> the product's own trig

    def internals(self, env):
        return env.internal

    def syn(self, env):
        return env.syn
