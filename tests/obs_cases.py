"""The batch the observation tests share (tests/test_gpu_render_obs.py, tests/test_render_obs_cpu.py): 48 walking envs
with a time limit of 7 steps, 16 of them on an empty target -- done on every step, so under auto-reset their stack
always restarts -- and 32 on rt20 targets, which under 20 steps of seeded random actions end by the time limit alone
(steps 7 and 14: 64 restarts, confirmed against the oracle by the CPU test)."""
import numpy as np

N, EMPTY, STEPS, MAX_STEPS, SEED = 48, 16, 20, 7, 5


def inputs(n=N):
    """(targets int8 [n, 9, 11, 11], poses f64 [n, 5], actions int32 [STEPS, n]) of the batch, or of a cut of n of
    its envs that keeps the share of empty-target rows (n = 8: two of them, then six rt20 rows)."""
    from gridworld_amd import workloads
    targets = np.zeros((N, 9, 11, 11), np.int8)
    targets[EMPTY:] = workloads.rt20(N - EMPTY, seed=SEED).numpy().astype(np.int8)
    rng = np.random.RandomState(SEED)
    poses = np.stack([rng.uniform(-4, 4, N), np.zeros(N), rng.uniform(-4, 4, N), rng.uniform(-180, 180, N),
                      rng.uniform(-30, 10, N)], 1)
    actions = rng.randint(0, 18, (STEPS, N)).astype(np.int32)
    k = EMPTY * n // N
    rows = np.r_[0:k, EMPTY:EMPTY + n - k]
    return targets[rows], poses[rows], np.ascontiguousarray(actions[:, rows])
