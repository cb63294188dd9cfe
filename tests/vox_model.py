"""Model of the voxel observation (include/igw_vox.h), written from the contract and not from the
kernel.

    new = vox_model.planes(grid, pose, sources, spec)        # uint8 [N, C, 9, S, S], numpy
    stack = vox_model.observe(new, prev, restart, spec)      # [N, K * C, 9, S, S] of spec.dtype, a CPU tensor

grid: integers [N, 9, 11, 11] (or [N, 1089]); pose: float64 [N, >= 4] = x, y, z, yaw (what internals() returns);
sources: name -> integers [N, 9, 11, 11] for the planes other than 'grid' ('target' is the USER's target grid);
spec: a vox.VoxSpec.  observe() follows tests/obs_model.py: the float path is two separate f32 ops, mul then add, then
.to(dtype); prev is the stack the previous call returned (None: every env restarts), restart a mask [N] (None: nobody
restarts; any value != 0 counts).  naive_planes() is the same contract as four nested loops, for the self-check."""
import numpy as np
import torch

AHEAD = ((0, -1), (1, 0), (0, 1), (-1, 0))    # f_q: (dx, dz) of one cell ahead in heading quadrant q
RIGHT = ((1, 0), (0, 1), (-1, 0), (0, -1))    # r_q: ... of one cell to the right


def quadrant(yaw):
    """floor((yaw + 45) / 90) mod 4 in binary64, non-negative."""
    return (np.floor((np.asarray(yaw, np.float64) + 45.0) / 90.0) % 4).astype(np.int64)


def head_cell(pose):
    """(hx, hy, hz) int64 [N] each: rint (round-half-even) of x, y, z plus (5, 1, 5)."""
    p = np.asarray(pose, np.float64)
    return (np.rint(p[:, 0]).astype(np.int64) + 5, np.rint(p[:, 1]).astype(np.int64) + 1,
            np.rint(p[:, 2]).astype(np.int64) + 5)


def channels(values, enc):
    """uint8 [N, 6 or 1, 9, 11, 11] of integers [N, 9, 11, 11]."""
    v = np.asarray(values).astype(np.int64).reshape(-1, 9, 11, 11)
    if enc == 'onehot':
        return np.stack([v == k + 1 for k in range(6)], 1).astype(np.uint8)
    return (v != 0).astype(np.uint8)[:, None]


def world_planes(grid, pose, sources, spec):
    """uint8 [N, C, 9, 11, 11]: every channel in the world's frame."""
    grid = np.asarray(grid).reshape(-1, 9, 11, 11)
    n = grid.shape[0]
    out = [channels(grid if name == 'grid' else sources[name], enc) for name, enc in spec.planes]
    if spec.agent:
        body = np.zeros((n, 1, 9, 11, 11), np.uint8)
        hx, hy, hz = head_cell(pose)
        for i in range(n):
            for y in (hy[i], hy[i] - 1):
                if 0 <= hx[i] <= 10 and 0 <= y <= 8 and 0 <= hz[i] <= 10:
                    body[i, 0, y, hx[i], hz[i]] = 1
        out.append(body)
    return np.concatenate(out, 1)


def planes(grid, pose, sources, spec):
    world = world_planes(grid, pose, sources, spec)
    if spec.frame == 'world':
        return world
    n, c = world.shape[:2]
    r, s_ = spec.radius, spec.size
    hx, _, hz = head_cell(pose)
    q = quadrant(np.asarray(pose, np.float64)[:, 3])
    ahead = r - np.arange(s_)[:, None]          # s of output row u
    right = np.arange(s_)[None, :] - r          # t of output column w
    out = np.zeros((n, c, 9, s_, s_), np.uint8)
    for i in range(n):
        (fx, fz), (rx, rz) = AHEAD[q[i]], RIGHT[q[i]]
        x = hx[i] + ahead * fx + right * rx
        z = hz[i] + ahead * fz + right * rz
        ok = (x >= 0) & (x <= 10) & (z >= 0) & (z <= 10)
        got = world[i][:, :, np.clip(x, 0, 10), np.clip(z, 0, 10)]      # [C, 9, S, S]
        out[i] = np.where(ok[None, None], got, 0)
    return out


def naive_planes(grid, pose, sources, spec):
    """planes(), cell by cell from the header's sentences."""
    grid = np.asarray(grid).reshape(-1, 9, 11, 11)
    n, s_, r = grid.shape[0], spec.size, spec.radius
    out = np.zeros((n, spec.channels, 9, s_, s_), np.uint8)
    for i in range(n):
        px, py, pz, yaw = (float(v) for v in np.asarray(pose, np.float64)[i, :4])
        hx, hy, hz = int(round(px)) + 5, int(round(py)) + 1, int(round(pz)) + 5     # Python's round is half-even
        q = int(np.floor((yaw + 45.0) / 90.0)) % 4
        for y in range(9):
            for u in range(s_):
                for w in range(s_):
                    if spec.frame == 'world':
                        x, z = u, w
                    else:
                        s, t = r - u, w - r
                        x = hx + s * AHEAD[q][0] + t * RIGHT[q][0]
                        z = hz + s * AHEAD[q][1] + t * RIGHT[q][1]
                    if not (0 <= x <= 10 and 0 <= z <= 10):
                        continue
                    ch = 0
                    for name, enc in spec.planes:
                        v = int((grid if name == 'grid' else np.asarray(sources[name]).reshape(-1, 9, 11, 11))[i, y, x, z])
                        if enc == 'onehot':
                            if 1 <= v <= 6:
                                out[i, ch + v - 1, y, u, w] = 1
                            ch += 6
                        else:
                            out[i, ch, y, u, w] = v != 0
                            ch += 1
                    if spec.agent and x == hx and z == hz and y in (hy, hy - 1):
                        out[i, ch, y, u, w] = 1
    return out


def convert(v, spec):
    """The stored value of the uint8 tensor `v` (0 / 1) in spec.dtype."""
    if spec.dtype is torch.uint8:
        return v
    f = v.to(torch.float32)
    f = torch.mul(f, torch.tensor(spec.scale, dtype=torch.float32))
    f = torch.add(f, torch.tensor(spec.bias, dtype=torch.float32))
    return f.to(spec.dtype)


def observe(new, prev, restart, spec, fill=False):
    new = convert(torch.as_tensor(np.ascontiguousarray(new)), spec)      # [N, C, 9, S, S]
    n, c = new.shape[:2]
    k, rest = spec.stack, tuple(new.shape[2:])
    filled = new.unsqueeze(1).expand(n, k, c, *rest)
    if prev is None or fill:
        return filled.reshape(n, k * c, *rest).contiguous()
    shifted = torch.cat([prev.reshape(n, k, c, *rest)[:, 1:], new.unsqueeze(1)], 1)
    if restart is None:
        return shifted.reshape(n, k * c, *rest).contiguous()
    r = torch.as_tensor(np.asarray(restart)).reshape(n).ne(0)
    return torch.where(r.view(n, 1, 1, 1, 1, 1), filled, shifted).reshape(n, k * c, *rest).contiguous()


def bits(t):
    """The raw bits of a tensor as an integer tensor (what torch.equal compares: -0.0 and NaN payloads included)."""
    return t if t.dtype is torch.uint8 else t.view({2: torch.int16, 4: torch.int32}[t.element_size()])
