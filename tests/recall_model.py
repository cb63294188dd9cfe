"""Model of the recall query (include/igw_recall.h), written from the contract and not from the
kernel: numpy for the entries, tests/vox_model.py for the planes and the element.

    grids = recall_model.entry_grids(start, words)              # int8 [len + 1, 1089]: entry 0 .. len of one episode
    want = recall_model.recall(records, first, length, starts, init_pose, episode, step, spec, goal=None,
                               goal_index=None, L=None)
    want['obs'], want['next_obs']   CPU tensors [B, K * C, 9, S, S] of spec.dtype
    want['record'] uint8 [B, 64], want['valid'] uint8 [B]       numpy

records: uint8 [n, 64]; first, length, episode, step: integers; starts: int8 [E, >= 1089]; init_pose: float64 [E, 5] (x,
y, z, yaw, pitch); goal: int8 [rows, >= 1089] or None; goal_index: integers [B] or None (row = the episode).  Entry 0 is
the starting grid at the reset pose; entry s >= 1 the grid after the changes of the episode's first s records, at the
float32 agentPos (x, y, z, pitch, yaw) of record s - 1, widened to float64."""
import numpy as np
import torch

import vox_model as VM

CELLS, NONE = 1089, 0xffff


def clean_start(row):
    """A starting row's 1089 cells, a cell outside 0..6 as 0."""
    g = np.asarray(row).reshape(-1)[:CELLS].astype(np.int8)
    return np.where((g >= 0) & (g <= 6), g, 0).astype(np.int8)


def words_of_records(rec):
    """uint16 [n]: the `change` word at byte 40 of records uint8 [n, 64]."""
    return np.ascontiguousarray(rec[:, 40:42]).view(np.uint16)[:, 0]


def entry_grids(start, words):
    """int8 [len(words) + 1, 1089]: the grid at every entry."""
    g = clean_start(start)
    out = [g.copy()]
    for w in np.asarray(words).astype(np.int64):
        if w != NONE and (w & 0x7ff) < CELLS:
            g[w & 0x7ff] = (w >> 11) & 7
        out.append(g.copy())
    return np.stack(out)


def entry_pose(rec, init, s):
    """float64 [4] (x, y, z, yaw) of entry s of an episode whose records are `rec` uint8 [len, 64]."""
    if s == 0:
        return np.asarray(init, np.float64)[:4].copy()
    p = np.ascontiguousarray(rec[s - 1, :20]).view(np.float32).astype(np.float64)
    return np.array([p[0], p[1], p[2], p[4]])


def slots(t, k):
    """(entries of obs's slots, entries of next_obs's slots) of a sample at step t with a stack of k."""
    return [max(0, t - k + j) for j in range(k)], [max(0, t - k + 1 + j) for j in range(k)]


def recall(records, first, length, starts, init_pose, episode, step, spec, goal=None, goal_index=None, L=None):
    records = np.asarray(records).reshape(-1, 64)
    first, length = np.asarray(first).astype(np.int64), np.asarray(length).astype(np.int64)
    episode, step = np.asarray(episode).astype(np.int64), np.asarray(step).astype(np.int64)
    n_rec, E, B, K = len(records), len(first), len(episode), spec.stack
    if L is not None:
        length = np.clip(length, 0, L)
    length = np.maximum(length, 0)
    rows = None if goal is None else np.asarray(goal).reshape(len(goal), -1)[:, :CELLS]
    valid = np.zeros(B, np.uint8)
    keys, index = [], {}          # the distinct (episode, entry, goal row) triples and where each went
    want = []                     # per sample: (entries of obs, entries of next_obs) as indices into keys, or None
    for b in range(B):
        e, t = int(episode[b]), int(step[b])
        ok = 0 <= e < E and 1 <= t <= length[e] and first[e] >= 0 and first[e] + length[e] <= n_rec
        row = -1
        if ok and rows is not None:
            row = e if goal_index is None else int(np.asarray(goal_index)[b])
            ok = 0 <= row < len(rows)
        if not ok:
            want.append(None)
            continue
        valid[b] = 1
        got = []
        for group in slots(t, K):
            ids = []
            for s in group:
                key = (e, s, row)
                if key not in index:
                    index[key] = len(keys)
                    keys.append(key)
                ids.append(index[key])
            got.append(ids)
        want.append(got)
    # every distinct entry once: its grid, its pose, its goal row
    grids_of = {}
    n = len(keys)
    grid, pose = np.zeros((n, CELLS), np.int8), np.zeros((n, 4))
    tgt = np.zeros((n, CELLS), np.int8)
    for i, (e, s, row) in enumerate(keys):
        rec = records[first[e]:first[e] + length[e]]
        if e not in grids_of:
            grids_of[e] = entry_grids(starts[e], words_of_records(rec))
        grid[i] = grids_of[e][s]
        pose[i] = entry_pose(rec, init_pose[e], s)
        if row >= 0:
            tgt[i] = rows[row]
    shape = spec.shape(B)
    per = (spec.channels,) + shape[2:]
    if n:
        planes = VM.convert(torch.from_numpy(VM.planes(grid.reshape(n, 9, 11, 11), pose, {'target': tgt.reshape(n, 9, 11, 11)},
                                                       spec)), spec)
    else:
        planes = VM.convert(torch.zeros((0,) + per, dtype=torch.uint8), spec)
    padding = VM.convert(torch.zeros((1,) + per, dtype=torch.uint8), spec)
    planes = torch.cat([planes, padding])                    # (the last row is a padding slot)
    ids = np.full((2, B, K), n, np.int64)
    record = np.zeros((B, 64), np.uint8)
    for b, got in enumerate(want):
        if got is not None:
            ids[0, b], ids[1, b] = got
            record[b] = records[first[episode[b]] + step[b] - 1]
    pick = lambda i: planes[torch.from_numpy(i.reshape(-1))].reshape(shape).contiguous()  # noqa: E731
    return dict(obs=pick(ids[0]), next_obs=pick(ids[1]), record=record, valid=valid)
