"""Census of the situations the step path's parity scenarios reach, computed on the CPU from the oracle alone.

Two measurements of one instrumented build of oracle/igw_oracle.c (compiled into a directory of the caller's, never
into oracle/; the normal libigw_oracle.so, the Makefile and oracle.py stay as they are):

  branch outcomes   `gcc --coverage`, read back with `gcov -b`: per function of the step path (STEP_FUNCTIONS) the
                    branch outcomes never taken, named  function | source line | branch k  (the text of the line, not
                    its number, so that an edit elsewhere in the file does not rename them);
  situation bins    what is no branch there -- which face of a block the sight ray stopped at on which level, which
                    face of `collide` fired at which body height, rounding ties, the agent's cell against the kernel's
                    clamp ranges ... -- from the counters igw_oracle.c keeps under -DIGO_CENSUS (off in the normal
                    build, whose object code the flag leaves unchanged).  Their names come from the library itself.

The instrumented library is loaded through a second instance of oracle/oracle.py (its own module object and its own
ctypes handle), so `oracle.oracle` -- what every parity test steps -- is never the instrumented one, and the census
side still has OracleEnv / OracleBatch.  It is stepped single-threaded: the counters are plain increments.
"""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE_DIR = os.path.join(HERE, '..', 'oracle')
SOURCE = os.path.abspath(os.path.join(ORACLE_DIR, 'igw_oracle.c'))
CFLAGS = ['-fPIC', '-std=c11', '-ffp-contract=off', '-fno-fast-math', '-pthread']   # oracle/Makefile's arithmetic

STEP_FUNCTIONS = ('build_zone', 'world_lookup', 'normalize', 'hit_test', 'get_sight_vector', 'get_motion_vector',
                  'collide', 'update_substep', 'update', 'grid_set', 'place_or_remove_block', 'world_step', 'igo_reset',
                  'finish_step', 'igo_step_walking', 'igo_step_walking_dict', 'igo_step_flying')
# the reward path's census (tests/reward_cases.py) reads these as well; a tuple of its own, so that the step census
# (profiles/r15_step_census.json) stays what it was
TASK_FUNCTIONS = ('task_init', 'task_get_intersection', 'task_maximal_intersection', 'task_reset', 'task_step_intersection')


class Census:
    """The instrumented oracle.  `O` is the second oracle module (O.OracleEnv, O.OracleBatch, O.use_device_trig)."""

    def __init__(self, workdir, coverage=True):
        from oracle import oracle as product
        product.build()                      # libigw_trig_host.so, which device-trig mode loads
        self.dir = str(workdir)
        self.coverage = coverage
        obj = os.path.join(self.dir, 'igw_oracle.o')
        so = os.path.join(self.dir, 'libigw_oracle_census.so')
        flags = CFLAGS + ['-DIGO_CENSUS'] + (['-O0', '--coverage', '-DIGO_CENSUS_GCOV'] if coverage else ['-O2'])
        subprocess.run(['gcc'] + flags + ['-c', '-o', obj, SOURCE], check=True, cwd=self.dir)
        subprocess.run(['gcc'] + flags + ['-shared', '-o', so, obj, '-lm'], check=True, cwd=self.dir)
        spec = importlib.util.spec_from_file_location('oracle_census_%x' % id(self), os.path.join(ORACLE_DIR, 'oracle.py'))
        self.O = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(self.O)
        self.O._LIB_PATH = so
        self.O.build = lambda force=False: so
        self.lib = self.O.lib()
        assert self.O is not product and self.lib is not product.lib()
        self.lib.igo_census_names.restype = C.c_char_p
        self.lib.igo_census_read.argtypes = [C.c_void_p]
        names = self.lib.igo_census_names().decode().split('\n')[:-1]
        assert len(names) == self.lib.igo_census_read(None) == len(set(names))
        first = self.lib.igo_census_first_reward_bin()
        self.names, self.reward_names = names[:first], names[first:]    # the step path's bins, the reward path's
        self.lib.igo_census_reset()

    def _read(self):
        out = np.zeros(len(self.names) + len(self.reward_names), np.int64)
        self.lib.igo_census_read(out.ctypes.data_as(C.c_void_p))
        return [int(v) for v in out]

    def bins(self):
        """{bin name: count} of the step path's bins since the library was loaded."""
        return dict(zip(self.names, self._read()))

    def reward_bins(self):
        """{bin name: count} of the reward path's bins since the library was loaded."""
        return dict(zip(self.reward_names, self._read()[len(self.names):]))

    def unreached_bins(self):
        return sorted(k for k, v in self.bins().items() if v == 0)

    def unreached_reward_bins(self):
        return sorted(k for k, v in self.reward_bins().items() if v == 0)

    def branches(self, functions=STEP_FUNCTIONS):
        """{'function | source line | branch k': times taken} of `functions`, everything run so far."""
        assert self.coverage
        self.lib.igo_census_flush()
        subprocess.run(['gcov', '-b', '-c', 'igw_oracle.o'], check=True, cwd=self.dir, stdout=subprocess.DEVNULL)
        return parse_gcov(os.path.join(self.dir, 'igw_oracle.c.gcov'), functions)

    def unreached_branches(self):
        return sorted(k for k, v in self.branches().items() if v == 0)


def parse_gcov(path, functions=STEP_FUNCTIONS):
    out, func, line, k = {}, None, None, 0
    for row in open(path):
        m = re.match(r'function (\w+) called', row)
        if m:
            func = m.group(1)
            continue
        m = re.match(r'\s*[-#=\d*]+:\s*(\d+):(.*)', row)
        if m:
            line, k = ' '.join(m.group(2).split()), 0
            continue
        m = re.match(r'branch\s+\d+ (never executed|taken (\d+))', row)
        if m and func in functions:
            key = f'{func} | {line} | branch {k}'
            assert key not in out, key
            out[key] = int(m.group(2) or 0)
        if m:
            k += 1
    assert len({k.split(' | ')[0] for k in out}) >= min(12, len(functions))   # (normalize, get_sight_vector and the like have no branch)
    return out


class Driver:
    """golden_replay's driver interface over the census oracle (golden_replay.OracleDriver, one thread)."""

    def __init__(self, census, fx):
        self.b = census.O.OracleBatch(len(fx['targets']), **fx['kwargs'])

    def set_tasks(self, targets, starts, invariant=True):
        self.b.set_tasks(targets, starts, invariant=invariant)

    def set_initial_pose(self, poses):
        self.b.set_initial_pose(poses)

    def reset(self, mask):
        self.b.reset(mask)

    def step_walking(self, actions):
        self.b.step_walking(actions)

    def step_flying(self, mv, cam, inv, place):
        self.b.step_flying(mv, cam, inv, place)

    def step_walking_dict(self, buttons, cam):
        self.b.step_walking_dict(buttons, cam)

    def set_task_table(self, targets, starts, full_grids):
        self._table = (targets, starts, full_grids)

    def assign_tasks(self, mask, rows):
        tg, st, fg = self._table
        for e in np.nonzero(mask)[0]:
            self.b.envs[e].set_task(tg[rows[e]], st[rows[e]], fg[rows[e]])

    def outputs(self):
        b = self.b
        return dict(agentPos=b.agentPos, inventory=b.inventory, compass=b.compass, reward=b.reward, done=b.done,
                    grid=b.grid, internal=None)   # (the float64 internals: tests/test_oracle_golden.py, one call per env)


def replay_fixtures(census):
    """Every step fixture of tests/golden through the census oracle (and checked, as tests/test_oracle_golden.py does)."""
    import golden_replay as GR
    steps = 0
    for name in GR.WALK_FIXTURES + GR.FLY_FIXTURES + GR.DICT_FIXTURES:
        fx = GR.load_fixture(name)
        steps += GR.replay(fx, Driver(census, fx))
    census.O.use_device_trig(True)
    try:
        for name in GR.CRLIBM_FIXTURES:
            fx = GR.load_fixture(name)
            steps += GR.replay(fx, Driver(census, fx))
    finally:
        census.O.use_device_trig(False)
    for name in GR.SUBTASK_FIXTURES:
        fx = GR.load_subtasks_fixture(name)
        steps += GR.replay_subtasks(fx, Driver(census, dict(targets=fx['full_grids'], kwargs=fx['kwargs'])))
    return steps
