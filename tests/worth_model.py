"""A numpy model of the worth query's contract (include/igw_worth.h), the yardstick of
tests/test_worth_cpu.py (which pins it to the CPU oracle) and tests/test_gpu_worth.py (which compares the kernel to it).

Per env, with S = grid - start and T = target - start: the vote counts H[r][dx + 10][dz + 10] = the cells of S that equal
the cell of rotation r of T they are paired with under the translation (dx, dz) (target index = grid index + (dx, dz),
tasks/task.py:138-145) are built from oracle.task_eval's four rotations; the admissible translations are that call's
mask; M is the maximum of H over them.  An edit that takes a cell from s0 to s1 removes the cell's votes for s0 and adds
those for s1; the words and `best` follow the header.  Adding edits use max(M, touched + 1) over a window of H -- which is
the definition for counts that only grow -- and removing edits a recount of the edited H."""
import numpy as np

PLANES, ROW, CELLS = 7, 1104, 1089


def votes(rot, s):
    """H int32 [4, 21, 21] of the synthetic grid s [9, 11, 11] against the rotations rot [4, 9, 11, 11]."""
    h = np.zeros((4, 21, 21), np.int32)
    ys, xs, zs = np.nonzero(s)
    for r in range(4):
        for y, x, z in zip(ys, xs, zs):
            tx, tz = np.nonzero(rot[r, y] == s[y, x, z])
            np.add.at(h[r], (tx - x + 10, tz - z + 10), 1)
    return h


def cell_bins(rot, y, x, z, v):
    """(r, dx + 10, dz + 10) index arrays of the bins a cell (y, x, z) of synthetic colour v != 0 votes in."""
    rs, us, vs = [], [], []
    for r in range(4):
        tx, tz = np.nonzero(rot[r, y] == v)
        rs.append(np.full(len(tx), r)), us.append(tx - x + 10), vs.append(tz - z + 10)
    return np.concatenate(rs), np.concatenate(us), np.concatenate(vs)


def encode(right, wrong, ends):
    return ((right & 0xfff) | (wrong + 1) << 12 | ends.astype(np.int32) << 14).astype(np.int16)


def env_worth(target, start, grid, cached, step_no, max_steps):
    """One env: target / start / grid int8 [9, 11, 11] (world block ids).  Returns a dict of
      word int16 [7, 1104]; mprime int32 [7, 9, 11, 11] (m' of every edit, -1 where invalid); M, n_max, target_size;
      and for the coverage floors bool [7, 9, 11, 11] arrays: adds, removes (the edit recounts and only adds / removes
      votes), touched (it touches an admissible bin), touched_max (a removing edit touches a bin that holds M)."""
    from oracle import oracle as O
    t, s = target.astype(np.int8) - start.astype(np.int8), grid.astype(np.int8) - start.astype(np.int8)
    ev = O.task_eval(t, s)
    rot, adm = ev['rot'].reshape(4, 9, 11, 11), ev['adm_mask'].astype(bool)
    tsize = ev['target_size']
    h = votes(rot, s)
    M = int((h * adm).max())
    assert M == ev['max_int']
    n_max = int(((h == M) & adm).sum())
    # adding edits: for every level y and colour v of the target, per grid cell the highest touched admissible count + 1
    top = np.full((15, 9, 11, 11), M, np.int32)          # [v + 7][y][x][z]
    ntouch = np.zeros((15, 9, 11, 11), np.int32)
    hm = np.where(adm, h, -1)
    for y in range(9):
        for v in np.unique(t[y]):
            if v == 0:
                continue
            for r in range(4):
                for tx, tz in zip(*np.nonzero(rot[r, y] == v)):
                    # bin of grid cell (x, z): (tx - x + 10, tz - z + 10), x, z = 0..10
                    win = hm[r, tx:tx + 11, tz:tz + 11][::-1, ::-1]
                    top[v + 7, y] = np.maximum(top[v + 7, y], win + 1)
                    ntouch[v + 7, y] += win >= 0
    g, st = grid.astype(np.int32), start.astype(np.int32)
    word = np.full((PLANES, ROW), -1, np.int16)
    mprime = np.full((PLANES, 9, 11, 11), -1, np.int32)
    flags = {k: np.zeros((PLANES, 9, 11, 11), bool) for k in ('adds', 'removes', 'touched', 'touched_max')}
    yy, xx, zz = np.indices((9, 11, 11))
    time_up = step_no + 1 == max_steps
    for p in range(PLANES):
        valid = (g != 0) if p == 0 else (g == 0)
        s0, s1 = (g - st, -st) if p == 0 else (-st, p - st)
        wrong = (s0 != 0).astype(np.int32) - (s1 != 0)
        m = np.full((9, 11, 11), cached, np.int32)
        adds, removes = valid & (wrong == -1), valid & (wrong == 1)
        va = np.clip(s1 + 7, 0, 14)
        m[adds] = top[va, yy, xx, zz][adds]
        flags['adds'][p] = adds
        flags['touched'][p] = adds & (ntouch[va, yy, xx, zz] > 0)
        for y, x, z in zip(*np.nonzero(removes)):
            b = cell_bins(rot, y, x, z, s0[y, x, z])
            h2 = h.copy()
            np.subtract.at(h2, b, 1)
            assert (h2 >= 0).all()
            m[y, x, z] = (h2 * adm).max()
            ok = adm[b]
            flags['touched'][p, y, x, z] = ok.any()
            flags['touched_max'][p, y, x, z] = M > 0 and (ok & (h[b] == M)).any()
        flags['removes'][p] = removes
        ends = (m == tsize) | time_up
        w = encode(m - cached, wrong, ends)
        word[p, :CELLS] = np.where(valid, w, -1).reshape(-1)
        mprime[p] = np.where(valid, m, -1)
    return dict(word=word, mprime=mprime, M=M, n_max=n_max, target_size=tsize, **flags)


def decode(word):
    """(right, wrong, ends, valid) of words, int32 / bool arrays."""
    w = np.asarray(word).astype(np.int32)
    valid = w >= 0
    right = np.where(valid, ((w & 0xfff) ^ 0x800) - 0x800, 0)
    return right, np.where(valid, ((w >> 12) & 3) - 1, 0), valid & ((w >> 14) & 1 == 1), valid


def best_of(word, right_scale, wrong_scale, allow=None, inventory=None):
    """best int32 [4] of one env's words [7, 1104]: allow uint8 [2, 1104] or None; inventory [6] (stocked) or None."""
    right, wrong, _, valid = decode(word)
    cand = valid.copy()
    cand[:, CELLS:] = False
    if allow is not None:
        a = np.asarray(allow).reshape(2, -1) != 0
        cand[0] &= a[0, :ROW]
        cand[1:] &= a[1, :ROW]
    if inventory is not None:
        cand[1:] &= (np.asarray(inventory) > 0)[:, None]
    n = int(cand.sum())
    if n == 0:
        return np.array([-1, -1, -1, 0], np.int32)
    reward = np.where(right != 0, right.astype(np.float64) * np.float64(right_scale),
                      wrong.astype(np.float64) * np.float64(wrong_scale))
    reward = np.where(cand, reward, -np.inf)
    top = reward.max()
    p, c = np.argwhere(cand & (reward == top))[0]     # the lowest plane, then the lowest cell
    return np.array([p, c, int(word[p, c]), n], np.int32)
