"""Recounts the GPU parity tests share (tests/test_gpu_parity.py, tests/test_gpu_step_cases.py): the persistent vote
histogram and the occupancy bitmap of a VecGridWorld against a fresh count from its int8 grid."""
import numpy as np
import torch


def expected_hist(target_syn, grid_syn):
    """The vote histogram the kernels keep per env, from first principles: for every rotation
    (tasks/task.py:47-56) and every admissible translation (bounding-box rule == tasks/task.py:62-72)
    the intersection count of tasks/task.py:138-145, laid out [rot][dx - dxlo][dz - dzlo] with pitch 11."""
    out = np.zeros(512, np.uint16)
    t = target_syn.astype(np.int32)
    g = grid_syn.astype(np.int32)
    if not t.any():
        return out
    for r in range(4):
        tr = np.rot90(t, k=-r, axes=(1, 2))
        _, xs, zs = np.nonzero(tr)
        dxlo, dxhi, dzlo, dzhi = xs.max() - 10, xs.min(), zs.max() - 10, zs.min()
        for dx in range(dxlo, dxhi + 1):
            for dz in range(dzlo, dzhi + 1):
                st = tr[:, max(dx, 0):11 + min(dx, 0), max(dz, 0):11 + min(dz, 0)]
                sg = g[:, max(-dx, 0):11 + min(-dx, 0), max(-dz, 0):11 + min(-dz, 0)]
                out[r * 121 + (dx - dxlo) * 11 + (dz - dzlo)] = ((st == sg) & (st != 0)).sum()
    return out


def check_hist(env, targets, starts=None, sample=None):
    """Persistent histogram == histogram recomputed from scratch; max_int == its maximum unless the
    reference itself holds a stale cached value (dirty bit)."""
    torch.cuda.synchronize()
    grid = env.grid.cpu().numpy().astype(np.int32)
    hist = env.hist_buf.cpu().numpy().view(np.uint16)
    ts = env.task_state()
    idx = range(env.num_envs) if sample is None else sample
    for e in idx:
        st = np.zeros((9, 11, 11), np.int32) if starts is None else starts[e].astype(np.int32)
        want = expected_hist(targets[e].astype(np.int32) - st, grid[e] - st)
        assert np.array_equal(hist[e], want), f'env {e}: histogram differs from a fresh recount'
        if not ts['dirty'][e]:
            assert ts['max_int'][e] == want.max(), f'env {e}: max_int {ts["max_int"][e]} vs {want.max()}'


def check_occ(env):
    """HBM occupancy rows == the grid in the padded 9 x 13 x 13 bit layout of include/igw.h."""
    torch.cuda.synchronize()
    n = env.num_envs
    g = env.grid.cpu().numpy().reshape(n, 9, 11, 11) != 0
    box = np.zeros((n, 9, 13, 13), bool)
    box[:, :, 1:12, 1:12] = g
    bits = np.zeros((n, 48 * 32), bool)
    bits[:, :9 * 169] = box.reshape(n, -1)
    want = np.packbits(bits.reshape(n, 48, 32), axis=-1, bitorder='little').view(np.uint32)[:, :, 0]
    got = env.occ_buf.cpu().numpy().view(np.uint32)
    assert got.shape == want.shape and np.array_equal(got, want), 'occupancy bitmap out of sync with the grid'
