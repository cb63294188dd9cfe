"""bench.py's plain / --full split and --dump-outputs, on the CPU (the GPU run itself is exercised on the GPU box)."""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_plain_run_times_one_window_and_full_keeps_the_old_defaults():
    import bench
    a = bench.parse_args(['--gpus', '1', '--steps', '20', '--warmup', '5'])
    assert not a.full and a.windows == 1 and a.rehearsals == 3 and a.dump_outputs is None
    a = bench.parse_args(['--steps', '100000', '--warmup', '5'])
    assert a.windows == 1 and a.rehearsals == 0          # a long window: no rehearsal of K steps
    a = bench.parse_args(['--full', '--steps', '100000'])
    assert a.full and a.windows == 15 and a.rehearsals == 3
    a = bench.parse_args(['--windows', '3', '--rehearsals', '1', '--dump-outputs', 'out'])
    assert a.windows == 3 and a.rehearsals == 1 and a.dump_outputs == 'out'


def _fake_env(N, seed=0):
    """The strided views VecGridWorld hands a caller (gridworld_amd/vec_env.py: _make_views), on the CPU."""
    import torch
    g = torch.Generator().manual_seed(seed)
    out = torch.randn((N, 16), generator=g)
    rec = torch.randint(0, 2, (N, 64), generator=g, dtype=torch.uint8)
    grid = torch.randint(-6, 7, (N, 1104), generator=g, dtype=torch.int8)
    return types.SimpleNamespace(num_envs=N, device=torch.device('cpu'), agent_pos=out[:, 0:5], inventory=out[:, 5:11],
                                 compass=out[:, 11], reward=out[:, 12], done=rec[:, 52],
                                 grid=torch.as_strided(grid, (N, 9, 11, 11), (1104, 121, 11, 1)))


def test_dump_outputs_writes_float_arrays_of_a_fixed_sample(tmp_path):
    import bench
    N = 20000
    env = _fake_env(N)
    info = bench.dump_outputs(env, str(tmp_path / 'a'))
    bench.dump_outputs(_fake_env(N), str(tmp_path / 'b'))
    names = ['agentPos', 'compass', 'done', 'env_index', 'grid', 'grid_env_index', 'inventory', 'reward']
    assert sorted(f[:-4] for f in os.listdir(tmp_path / 'a')) == names
    total = 0
    for n in names:
        x, y = np.load(tmp_path / 'a' / (n + '.npy')), np.load(tmp_path / 'b' / (n + '.npy'))
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y)
        total += x.nbytes
    assert total == info['bytes'] <= 64 << 20
    gi = np.load(tmp_path / 'a' / 'grid_env_index.npy').astype(np.int64)
    assert len(gi) == info['grid_envs'] == 8192 and np.all(np.diff(gi) > 0)
    assert np.array_equal(np.load(tmp_path / 'a' / 'grid.npy'), env.grid.numpy()[gi].astype(np.float32))
    assert np.array_equal(np.load(tmp_path / 'a' / 'env_index.npy'), np.arange(N, dtype=np.float64))
    assert np.array_equal(np.load(tmp_path / 'a' / 'done.npy'), env.done.numpy().astype(np.float32))
    assert np.array_equal(np.load(tmp_path / 'a' / 'agentPos.npy'), env.agent_pos.numpy())
