"""Any grid from any camera: batched views (igw_render_views, include/igw_render.h) and the reference's Visualizer.

    import gridworld_amd as G
    yaw, pitch = G.look_at((9, 6, 9), (0, 1, 0))
    frames = G.render_views(grids, poses)                    # [M, H, W, 3] uint8 on the device, one launch
    vis = G.Visualizer(render_size=(512, 512))
    image = vis.render((9, 6, 9), (yaw, pitch), blocks=[(0, 0, 0, 1), (0, 1, 0, 3)])
    orbit = vis.render_batch(*G.visualizer.split_poses(G.orbit_poses((0, 1, 0), 12, 5, 180)))

The camera is the one of the first-person frame: forward = (sin yaw cos pitch, sin pitch,
-cos yaw cos pitch), 90 degrees of vertical field of view, depth 0.1 .. 30.  There is no CPU fallback: rendering
without a HIP device raises; everything else here (the camera helpers, a Visualizer's world) is host code.
"""
import math

import numpy as np

from . import codec as K
from . import render as R

GRID_SHAPE = (9, 11, 11)
CELLS = 1089
GRID_STRIDE = 1104           # include/igw.h: IGW_GRID_STRIDE, the row stride of grid_buf / task_target / task_start


# ---- cameras ------------------------------------------------------------------------------------------------------
def look_at(eye, target):
    """(yaw, pitch) in degrees of a camera at `eye` whose forward vector points at `target`: with v the unit vector
    from eye to target, pitch = asin(v_y) and yaw = atan2(v_x, -v_z) (straight up or down: yaw 0)."""
    v = np.asarray(target, np.float64).reshape(3) - np.asarray(eye, np.float64).reshape(3)
    n = math.sqrt(float(v @ v))
    if not n > 0.0 or not math.isfinite(n):
        raise ValueError('look_at needs two distinct finite points')
    v = v / n
    pitch = math.degrees(math.asin(max(-1.0, min(1.0, float(v[1])))))
    yaw = math.degrees(math.atan2(float(v[0]), -float(v[2]))) if (v[0] != 0.0 or v[2] != 0.0) else 0.0
    return yaw, pitch


def orbit_poses(centre, radius, height, n, phase=0.0):
    """[n, 5] float64 poses (x, y, z, yaw, pitch) of n eyes evenly spaced on the horizontal circle of `radius` around
    the vertical axis through `centre`, `height` above it, each looking at the centre.  Eye k stands at the angle
    phase + 360 k / n degrees, measured from +x towards +z."""
    c = np.asarray(centre, np.float64).reshape(3)
    n = int(n)
    if n < 0:
        raise ValueError('orbit_poses needs n >= 0')
    out = np.empty((n, 5), np.float64)
    for k in range(n):
        a = math.radians(phase) + 2.0 * math.pi * k / n
        eye = c + np.array([radius * math.cos(a), height, radius * math.sin(a)])
        out[k, :3] = eye
        out[k, 3:] = look_at(eye, c)
    return out


def split_poses(poses):
    """[T, 5] poses -> (positions [T, 3], rotations [T, 2]): the two arguments of Visualizer.render_batch."""
    p = np.asarray(poses, np.float64).reshape(-1, 5)
    return p[:, :3], p[:, 3:]


# ---- batched views ------------------------------------------------------------------------------------------------
def _grid_rows(grids, dev):
    """int8 device tensor and the row stride to hand to igw_render_views: (tensor, stride, n_grids).  A device tensor
    whose cells are contiguous inside each row is used in place."""
    import torch
    t = grids if torch.is_tensor(grids) else torch.from_numpy(np.ascontiguousarray(np.asarray(grids)))
    if t.dtype not in (torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64):
        raise ValueError(f'grids must hold integers, got {t.dtype}')
    if t.dim() == 3 and tuple(t.shape) == GRID_SHAPE:
        t = t.unsqueeze(0)
    if t.dim() == 4 and tuple(t.shape[1:]) == GRID_SHAPE:
        in_place = t.shape[0] == 0 or tuple(t.stride()[1:]) == (121, 11, 1)
    elif t.dim() == 2 and t.shape[1] in (CELLS, GRID_STRIDE):
        in_place = t.shape[0] == 0 or t.stride(1) == 1
    else:
        raise ValueError(f'grids must be [G, 9, 11, 11], [G, 1089] or [G, 1104], got {tuple(t.shape)}')
    n = int(t.shape[0])
    width = CELLS if t.dim() == 4 else int(t.shape[1])
    stride = int(t.stride(0)) if n > 1 else width
    if not (in_place and t.dtype == torch.int8 and t.device == dev and stride >= CELLS):
        t = t.to(device=dev, dtype=torch.int8).contiguous()
        stride = width
    return t, stride, n


def render_views(grids, poses, view_grid=None, size=(64, 64), channels=3, atlas=None, out=None, device='cuda:0',
                 outputs=None, codec=None, quality=90):
    """M views in one launch on the current stream: view v shows grids[view_grid[v]] (grids[v] without view_grid) from
    poses[v].  Returns a uint8 device tensor [M, H, W, channels] with W, H = size, row 0 the top image row.

      grids      int8 [G, 9, 11, 11], [G, 1089] or [G, 1104] (numpy or tensor; cells [y+1][x+5][z+5], ids 0..6).  A
                 device tensor whose rows are contiguous is read in place, whatever its row stride (>= 1089): a dense
                 array, VecGridWorld.grid / grid_buf / task_target / task_start, or a slice of rows of one.
      poses      [M, 5] float64 x, y, z, yaw, pitch (degrees)
      view_grid  [M] row of each view.  A host-side one (list, numpy, CPU tensor) is range-checked here; an int32
                 device tensor is handed over as it is, and a view whose entry is out of range is left undrawn.
      atlas      uint8 [S, S, 4] (render.load_atlas / default_atlas; default: the flat colours), numpy or device tensor
      out        a contiguous uint8 tensor [M, H, W, channels] on `device` to write into (returned)
      outputs    None: the frame alone, as above.  A tuple of names from 'rgb', 'depth', 'label', 'surface': a dict
                 name -> tensor from the one igw_render_views_aux launch (depth float32, label uint8, surface int16,
                 each [M, H, W]; include/igw_render.h gives their values, render.decode_surface / unproject read
                 them); `out` is then a dict of preallocated tensors under the same names, or None.
      codec      'jpeg': (buf, sizes) of codec.encode_jpeg instead of the frames, which are drawn and then encoded at
                 `quality` by a second launch on the same stream; `out` is then the (buf, sizes) pair to encode into.
    """
    import torch
    res = K.encoded(codec, outputs, quality, out,
                    lambda: render_views(grids, poses, view_grid, size, channels, atlas, None, device))
    if res is not None:
        return res
    outputs = R.check_outputs(outputs)
    R.need_device('render_views')
    dev = torch.device(device)
    if dev.type == 'cuda' and dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    g, stride, n_grids = _grid_rows(grids, dev)
    if torch.is_tensor(poses):
        p = poses.to(device=dev, dtype=torch.float64)
    else:
        p = torch.from_numpy(np.ascontiguousarray(np.asarray(poses, np.float64))).to(dev)
    if p.dim() != 2 or p.shape[1] != 5:
        raise ValueError(f'poses must be [M, 5] (x, y, z, yaw, pitch), got {tuple(p.shape)}')
    p = p.contiguous()
    m = int(p.shape[0])
    vg = None
    if view_grid is None:
        if n_grids < m:
            raise ValueError(f'{m} views of {n_grids} grids need a view_grid')
    elif torch.is_tensor(view_grid) and view_grid.device.type == 'cuda':
        if view_grid.dtype != torch.int32 or tuple(view_grid.shape) != (m,) or view_grid.device != dev:
            raise ValueError(f'a device-side view_grid is an int32 tensor [{m}] on {dev}')
        vg = view_grid.contiguous()
    else:
        idx = np.asarray(view_grid.numpy() if torch.is_tensor(view_grid) else view_grid)
        if idx.shape != (m,) or (m and idx.dtype.kind not in 'iu'):
            raise ValueError(f'view_grid must hold {m} integer rows, got {idx.dtype} {idx.shape}')
        if m and (idx.min() < 0 or idx.max() >= n_grids):
            raise ValueError(f'view_grid must index the {n_grids} grids, got {int(idx.min())}..{int(idx.max())}')
        vg = torch.from_numpy(idx.astype(np.int32)).to(dev)
    a = R.device_atlas(atlas, dev)
    with torch.cuda.device(dev):
        return R.launch('views', (g.data_ptr(), stride, n_grids, None if vg is None else vg.data_ptr(), p.data_ptr(), m),
                        m, size, channels, outputs, out, a, dev, torch.cuda.current_stream(dev).cuda_stream)


# ---- the reference's Visualizer -----------------------------------------------------------------------------------
def blocks_to_grid(blocks, y_shift=0, grid=None):
    """int8 [9, 11, 11] grid of a list of blocks (x, y, z, id) in world coordinates, each placed at (x, y + y_shift, z):
    cell [y+1][x+5][z+5].  A later block replaces an earlier one at the same place.  A block outside the build zone
    (x, z in -5..5, y in -1..7) or with an id outside 1..6 raises ValueError."""
    g = np.zeros(GRID_SHAPE, np.int8) if grid is None else grid
    for b in blocks:
        x, y, z, bid = _block(b, y_shift)
        g[y + 1, x + 5, z + 5] = bid
    return g


def _block(b, y_shift=0):
    if len(b) != 4:
        raise ValueError(f'a block is (x, y, z, id), got {b!r}')
    vals = [float(v) for v in b]
    if any(v != int(v) for v in vals):
        raise ValueError(f'a block has integer coordinates and id, got {b!r}')
    x, y, z, bid = (int(v) for v in vals)
    y += y_shift
    if not (-5 <= x <= 5 and -1 <= y <= 7 and -5 <= z <= 5):
        raise ValueError(f'block {tuple(b)} lies outside the build zone (x, z in -5..5, y in -1..7'
                         f'{"" if not y_shift else " after the shift by %d" % y_shift}): the ray caster draws the '
                         f'9 x 11 x 11 zone only')
    if not 1 <= bid <= 6:
        raise ValueError(f'block {tuple(b)}: the id must be one of 1..6 (BLUE .. YELLOW)')
    return x, y, z, bid


class Visualizer:
    """The reference's gridworld.visualizer.Visualizer on the HIP ray caster: a block world and a free camera.

        vis = Visualizer(render_size=(512, 512))
        vis.set_world_state([(0, -1, 0, 1), (0, 0, 0, 3)])
        image = vis.render(position=(6, 4, 6), rotation=look_at((6, 4, 6), (0, 0, 0)))   # numpy uint8 [H, W, 3]

    `position` is the eye (x, y, z), `rotation` is (yaw, pitch) in degrees; both default to zero and persist, like
    the reference's agent.  Blocks are (x, y, z, id) in world coordinates.  `world` maps (x, y, z) to the id and
    `grid()` is the int8 [9, 11, 11] array a render draws, so the bookkeeping can be inspected without a device.

    Differences from the reference:
      * a block outside the 9 x 11 x 11 build zone (x, z in -5..5, y in -1..7) or with an id outside 1..6 raises
        ValueError (the reference would draw it; the ray caster is bounded by the zone);
      * removing a block that is not there is ignored (the reference raises KeyError);
      * the frame is RGB: the reference's frame without its alpha, which render() drops there too;
      * render_batch(positions, rotations, blocks=None) draws T poses of the current world, or T (pose, block list)
        pairs, in ONE launch and returns [T, H, W, 3]; render_video(output, positions, rotations, blocks=None) takes
        the same and writes them as {output}.avi, Motion-JPEG (gridworld_amd/codec.py), where the reference writes an
        mp4 through cv2; there is no postproc_video (no ffmpeg here).
    Without a HIP device render(), render_batch() and render_video() raise render.RenderError.
    """

    def __init__(self, render_size=(64, 64), device='cuda:0', atlas=None):
        self.render_size = (int(render_size[0]), int(render_size[1]))
        if not all(1 <= s <= R.MAX_SIDE for s in self.render_size):
            raise ValueError(f'render_size must be within 1..{R.MAX_SIDE} each way, got {render_size}')
        self.device = device
        self.atlas = None if atlas is None else R.check_atlas(atlas)
        self._atlas_dev = None
        self.position = (0.0, 0.0, 0.0)
        self.rotation = (0.0, 0.0)
        self.world = {}

    # -- state --
    def set_agent_state(self, position=None, rotation=None):
        """Moves the camera: position (x, y, z), rotation (yaw, pitch); None leaves that part as it is."""
        if position is not None:
            self.position = _vector(position, 3, 'position')
        if rotation is not None:
            self.rotation = _vector(rotation, 2, 'rotation')

    def set_world_state(self, blocks, add=True):
        """Adds (add=True; a block replaces one already there) or removes (add=False; the ids are ignored) blocks
        (x, y, z, id).  Nothing changes if any block is invalid."""
        checked = [_block(b) if add else _block((*b[:3], 1)) for b in blocks]
        for x, y, z, bid in checked:
            if add:
                self.world[(x, y, z)] = bid
            else:
                self.world.pop((x, y, z), None)

    def clear(self):
        self.world.clear()

    def grid(self):
        """The int8 [9, 11, 11] grid ([y+1][x+5][z+5]) of the current world: what render() draws."""
        return blocks_to_grid([(x, y, z, bid) for (x, y, z), bid in self.world.items()])

    def pose(self):
        """[5] float64 x, y, z, yaw, pitch of the camera."""
        return np.array([*self.position, *self.rotation], np.float64)

    def replace_world(self, blocks):
        """What render(blocks=) does to the world: it becomes `blocks`, each placed at (x, y - 1, z)."""
        world = {}
        for b in blocks:
            x, y, z, bid = _block(b, -1)
            world[(x, y, z)] = bid
        self.world = world

    # -- frames --
    def _atlas(self):
        import torch
        R.need_device('Visualizer.render')
        if self._atlas_dev is None:
            self._atlas_dev = R.device_atlas(self.atlas, torch.device(self.device))
        return self._atlas_dev

    def render(self, position=None, rotation=None, blocks=None, outputs=None):
        """The frame of the world from the camera: numpy uint8 [H, W, 3].  position / rotation move the camera first
        (and stay); `blocks` REPLACES the world, each block (x, y, z, id) placed at (x, y - 1, z) as in the
        reference (a list of blocks counted from the ground level 0 rather than the world's -1).  outputs (a tuple
        of 'rgb', 'depth', 'label', 'surface'; render_views) gives a dict name -> numpy array instead: the frame
        and / or the [H, W] planes, e.g. surface for picking the cell under a pixel (render.decode_surface)."""
        outputs = R.check_outputs(outputs)
        self.set_agent_state(position, rotation)
        if blocks is not None:
            self.replace_world(blocks)
        out = render_views(self.grid()[None], self.pose()[None], size=self.render_size, atlas=self._atlas(),
                           device=self.device, outputs=outputs)
        return _to_host(out, 0)

    def render_batch(self, positions, rotations, blocks=None, outputs=None):
        """T frames in one launch: numpy uint8 [T, H, W, 3].  positions [T, 3], rotations [T, 2].  blocks=None: the
        current world from the T poses (one grid, T views).  Otherwise `blocks` is a list of T block lists, frame t
        showing blocks[t] the way render(blocks=) places them (y - 1); the world is left holding the last one, and
        the camera the last pose, as after T render() calls.  outputs: as for render(), a dict of [T, ...] arrays."""
        outputs = R.check_outputs(outputs)
        poses, grids = self.batch_inputs(positions, rotations, blocks)
        view_grid = np.zeros(len(poses), np.int32) if blocks is None else None
        out = render_views(grids, poses, view_grid=view_grid, size=self.render_size, atlas=self._atlas(),
                           device=self.device, outputs=outputs)
        return _to_host(out)

    def render_video(self, output, positions, rotations, blocks=None, fps=60, quality=90):
        """The frames of render_batch(positions, rotations, blocks) as a video: ONE render launch, ONE encode launch
        (codec.encode_jpeg at `quality`), then {output}.avi, Motion-JPEG at `fps` (codec.write_avi).  Returns the
        path.  The camera and the world are left as after render_batch."""
        poses, grids = self.batch_inputs(positions, rotations, blocks)
        view_grid = np.zeros(len(poses), np.int32) if blocks is None else None
        buf, sizes = render_views(grids, poses, view_grid=view_grid, size=self.render_size, atlas=self._atlas(),
                                  device=self.device, codec='jpeg', quality=quality)
        return K.write_avi(f'{output}.avi', K.jpeg_bytes(buf, sizes), self.render_size, fps)

    def batch_inputs(self, positions, rotations, blocks=None):
        """(poses [T, 5], grids [1 or T, 9, 11, 11]) that render_batch draws; updates the camera and the world."""
        pos = np.asarray(positions, np.float64).reshape(-1, 3)
        rot = np.asarray(rotations, np.float64).reshape(-1, 2)
        if len(pos) != len(rot):
            raise ValueError(f'{len(pos)} positions but {len(rot)} rotations')
        if blocks is not None and len(blocks) != len(pos):
            raise ValueError(f'{len(pos)} poses but {len(blocks)} block lists')
        poses = np.concatenate([pos, rot], 1)
        if blocks is None:
            grids = self.grid()[None]
        else:
            grids = np.stack([blocks_to_grid(b, -1) for b in blocks]) if len(blocks) else np.zeros((0, *GRID_SHAPE),
                                                                                                    np.int8)
            if len(blocks):
                self.replace_world(blocks[-1])
        if len(poses):
            self.set_agent_state(poses[-1, :3], poses[-1, 3:])
        return poses, grids


def _to_host(res, index=slice(None)):
    """What render_views returned, a tensor or a dict of them, as numpy: all of it, or frame `index`."""
    if isinstance(res, dict):
        return {k: v[index].cpu().numpy() for k, v in res.items()}
    return res[index].cpu().numpy()


def _vector(v, n, name):
    a = np.asarray(v, np.float64).reshape(-1)
    if a.shape != (n,):
        raise ValueError(f'{name} has {n} components, got {v!r}')
    return tuple(float(x) for x in a)
