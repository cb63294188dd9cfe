"""First-person frames: builds and binds libigw_render.so (include/igw_render.h) and provides its texture atlases.

    from gridworld_amd import render
    atlas = render.load_atlas('texture.png')       # the reference's texture file, for the reference's look
    frames = env.render_pov()                       # or VecGridWorld(..., renderer='hip') for obs['pov']
    views = gridworld_amd.render_views(grids, poses)    # any grid from any camera (gridworld_amd/visualizer.py)

The renderer is a separate library: it reads the step path's state buffers (include/igw.h) and is not part of the
step library's build (its sources and build id are its own, so the step library's profiles stay valid).  There is
no CPU fallback: without a HIP device every call raises.
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

from . import build as _build

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc', 'render')
LIB = os.path.join(HERE, 'libigw_render.so')
SOURCES = [os.path.join(CSRC, 'igw_render.hip')]
HEADERS = [os.path.join(CSRC, 'igw_render_frame.h'), os.path.join(HERE, '..', 'include', 'igw_render.h')]
# the training-layout observation is a library of its own (include/igw_render_obs.h): the same ray caster, compiled
# again, so that libigw_render.so and its build id stay what they were
OBS_LIB = os.path.join(HERE, 'libigw_render_obs.so')
OBS_SOURCES = [os.path.join(CSRC, 'igw_render_obs.hip')]
OBS_HEADERS = HEADERS + [os.path.join(CSRC, 'igw_render_obs_stage.h'),
                         os.path.join(HERE, '..', 'include', 'igw_render_obs.h')]
VERSION = 1
MAX_SIDE = 1024
MAX_ATLAS = 256
MAX_EPISODE = 1 << 24
CLEAR_RGBA = (128, 176, 255, 255)   # unorm8 of glClearColor(0.5, 0.69, 1.0, 1), gridworld/render.py:41
_vp, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64
# every symbol include/igw_render.h declares: (result, arguments)
SIGNATURES = {
    'igw_render_version': (C.c_int, []),
    'igw_render_build_id': (C.c_char_p, []),
    'igw_render_last_error': (C.c_char_p, []),
    'igw_render_pov': (C.c_int, [_vp, _vp, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _vp]),
    'igw_render_episodes': (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _i64, _i32, _i32,
                                      _i32, _vp]),
    'igw_render_views': (C.c_int, [_vp, _i64, _i32, _vp, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _vp]),
}
# the siblings with planes: `const igw_render_aux* aux` in front of `stream`
SIGNATURES.update({name + '_aux': (res, args[:-1] + [_vp] + args[-1:])
                   for name, (res, args) in list(SIGNATURES.items()) if args})
EXPORTS = list(SIGNATURES)
# every symbol include/igw_render_obs.h declares; igw_render_pov_obs is the plain pov entry without `channels`, with
# `const igw_render_obs* obs` in front of `stream`
OBS_SIGNATURES = {
    'igw_render_obs_build_id': (C.c_char_p, []),
    'igw_render_obs_last_error': (C.c_char_p, []),
    'igw_render_pov_obs': (C.c_int, [_vp, _vp, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _vp, _vp]),
}
OBS_EXPORTS = list(OBS_SIGNATURES)
# the library as build.py builds it: the step library's FLAGS, an id of its own (igw_render_build_id())
LIBRARY = _build.Library(LIB, SOURCES, HEADERS, 'igw-render-build-id:', 'IGW_RENDER_BUILD_ID', deps=[__file__])
source_hash, built_id, is_stale = LIBRARY.source_hash, LIBRARY.built_id, LIBRARY.is_stale
OBS_LIBRARY = _build.Library(OBS_LIB, OBS_SOURCES, OBS_HEADERS, 'igw-render-obs-build-id:', 'IGW_RENDER_OBS_BUILD_ID',
                             deps=[__file__])


class RenderError(RuntimeError):
    pass


class Aux(C.Structure):
    """igw_render_aux: the three optional planes of the _aux entries (device pointers, None = not wanted)."""
    _fields_ = [('depth', _vp), ('label', _vp), ('surface', _vp)]


class Obs(C.Structure):
    """igw_render_obs: the observation of igw_render_pov_obs (`data` and `restart` are device pointers)."""
    _fields_ = [('data', _vp), ('dtype', _i32), ('gray', _i32), ('stack', _i32), ('fill', _i32),
                ('scale', C.c_float), ('bias', C.c_float), ('restart', _vp), ('restart_stride', _i64)]


OBS_DTYPES = {torch.uint8: 0, torch.float16: 1, torch.bfloat16: 2, torch.float32: 3}   # IGW_OBS_*
MAX_STACK = 8


class ObsSpec:
    """The layout of a training observation (include/igw_render_obs.h: igw_render_obs): `dtype` torch.uint8, float16,
    bfloat16 or float32; gray = one luminance plane in place of R, G, B; stack = K, the last K frames (1..8), oldest
    first; the float types hold value * scale + bias (uint8 takes scale 1, bias 0).  Validated on construction
    (ValueError; no device needed)."""

    def __init__(self, dtype=torch.uint8, gray=False, stack=1, scale=1.0, bias=0.0):
        if isinstance(dtype, str):
            dtype = getattr(torch, dtype, dtype)
        if dtype not in OBS_DTYPES:
            raise ValueError(f'dtype must be torch.uint8, float16, bfloat16 or float32, got {dtype!r}')
        if isinstance(stack, bool) or int(stack) != stack or not 1 <= int(stack) <= MAX_STACK:
            raise ValueError(f'stack must be an integer in 1..{MAX_STACK}, got {stack!r}')
        scale, bias = float(scale), float(bias)
        top = float(np.finfo(np.float32).max)   # (the kernel takes them as float32)
        if not (abs(scale) <= top and abs(bias) <= top):
            raise ValueError(f'scale and bias must be finite float32 values, got {scale!r}, {bias!r}')
        if dtype is torch.uint8 and (scale != 1.0 or bias != 0.0):
            raise ValueError('a uint8 observation takes scale 1 and bias 0')
        self.dtype, self.gray, self.stack, self.scale, self.bias = dtype, bool(gray), int(stack), scale, bias
        self.planes = 1 if self.gray else 3

    @classmethod
    def of(cls, spec):
        """An ObsSpec as it is, or one from a dict of its arguments."""
        if isinstance(spec, cls):
            return spec
        if isinstance(spec, dict):
            return cls(**spec)
        raise ValueError(f'an observation is an ObsSpec or a dict of its arguments, got {type(spec).__name__}')

    def shape(self, n, size):
        """(n, K * planes, H, W) for size = (W, H): slot k holds channels [k * planes, (k + 1) * planes)."""
        return (int(n), self.stack * self.planes, int(size[1]), int(size[0]))

    def __repr__(self):
        return (f'ObsSpec(dtype={self.dtype}, gray={self.gray}, stack={self.stack}, scale={self.scale}, '
                f'bias={self.bias})')


# the outputs of a render call with `outputs=`: 'rgb' is the colour frame, the others the planes (name -> dtype name)
OUTPUTS = ('rgb', 'depth', 'label', 'surface')
PLANE_DTYPES = {'depth': 'float32', 'label': 'uint8', 'surface': 'int16'}
FACES = ('top', 'bottom', 'left', 'right', 'front', 'back')   # the face codes of `surface`; 6 = the ground
GROUND_FACE, CELLS, GROUND_SPAN = 6, 1089, 37


def build(force=False, verbose=False):
    """Builds both renderer libraries; returns the path of libigw_render.so."""
    OBS_LIBRARY.build(force, verbose=verbose)
    return LIBRARY.build(force, verbose=verbose)


BINDING = _build.Binding(LIBRARY, SIGNATURES, RenderError, 'igw_render_last_error', 'igw_render_build_id',
                         'gridworld_amd.render', 'igw_render_pov')
load, check, build_id = BINDING.load, BINDING.check, BINDING.build_id
OBS_BINDING = _build.Binding(OBS_LIBRARY, OBS_SIGNATURES, RenderError, 'igw_render_obs_last_error',
                             'igw_render_obs_build_id', 'gridworld_amd.render', 'igw_render_pov_obs')


def need_device(what):
    import torch
    if not torch.cuda.is_available():
        raise RenderError(f'{what} needs a HIP device (the renderer has no CPU fallback)')


# ---- atlases ----------------------------------------------------------------------------------------------------
# tile (column, row-from-the-bottom) of each texture id in the 4 x 4 atlas (gridworld/utils.py:134-154)
TILES = {-1: (0, 0), 0: (1, 0), 1: (2, 0), 2: (3, 0), 3: (0, 1), 4: (1, 1), 5: (2, 1), 6: (3, 1)}
# the flat colours of the default atlas: WHITE, GREY ground, then BLUE, GREEN, RED, ORANGE, PURPLE, YELLOW
FLAT_COLOURS = {-1: (255, 255, 255), 0: (79, 81, 85), 1: (0, 162, 232), 2: (34, 177, 76), 3: (237, 28, 36),
                4: (255, 127, 39), 5: (163, 73, 164), 6: (255, 242, 0)}


def default_atlas(side=128):
    """uint8 [side, side, 4] with one solid colour per tile (the other tiles black); row 0 is the top image row."""
    a = np.zeros((side, side, 4), np.uint8)
    a[..., 3] = 255
    t = side // 4
    for tid, (tx, ty) in TILES.items():
        r0 = side - (ty + 1) * t      # v = 0 is the bottom image row
        a[r0:r0 + t, tx * t:(tx + 1) * t, :3] = FLAT_COLOURS[tid]
    return a


def check_atlas(atlas):
    """A [S, S, 4] uint8 array with S a multiple of 8 in 8..256 (what igw_render_pov accepts)."""
    a = np.asarray(atlas)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 4 or a.shape[0] != a.shape[1]:
        raise ValueError(f'an atlas is uint8 [S, S, 4], got {a.dtype} {a.shape}')
    if a.shape[0] % 8 or not 8 <= a.shape[0] <= MAX_ATLAS:
        raise ValueError(f'the atlas side must be a multiple of 8 in 8..{MAX_ATLAS}, got {a.shape[0]}')
    return np.ascontiguousarray(a)


def load_atlas(path):
    """A texture atlas from a PNG (through PIL, when it is importable) or a .npy file: uint8 [S, S, 4], row 0 = the top
    image row.  Passing the reference's gridworld/texture.png gives the reference's look."""
    if str(path).lower().endswith('.npy'):
        return check_atlas(np.load(path))
    try:
        from PIL import Image
    except ImportError as e:
        raise RenderError(f'reading {path} needs PIL; convert it to a uint8 [S, S, 4] .npy instead') from e
    with Image.open(path) as im:
        return check_atlas(np.asarray(im.convert('RGBA'), dtype=np.uint8))


def device_atlas(atlas, dev):
    """The atlas a launch reads: a contiguous uint8 [S, S, 4] tensor on `dev` (S as for check_atlas) from a numpy array,
    a CPU tensor, a tensor on `dev` (used in place) or None (the default atlas)."""
    import torch
    if torch.is_tensor(atlas) and atlas.device == dev:
        if atlas.dtype != torch.uint8 or atlas.dim() != 3 or atlas.shape[2] != 4 or atlas.shape[0] != atlas.shape[1] \
                or atlas.shape[0] % 8 or not 8 <= atlas.shape[0] <= MAX_ATLAS:
            raise ValueError(f'an atlas is uint8 [S, S, 4], S a multiple of 8 in 8..{MAX_ATLAS}, got '
                             f'{atlas.dtype} {tuple(atlas.shape)}')
        return atlas.contiguous()
    a = default_atlas() if atlas is None else check_atlas(atlas.cpu().numpy() if torch.is_tensor(atlas) else atlas)
    return torch.from_numpy(a).to(dev)


# ---- rendering ----------------------------------------------------------------------------------------------------
def check_outputs(outputs):
    """The `outputs` argument of a render call: None (the colour frame alone) as it is, otherwise the tuple of names
    asked for, each one of OUTPUTS, none twice (ValueError before any device work)."""
    if outputs is None:
        return None
    if isinstance(outputs, str):
        outputs = (outputs,)
    names = tuple(outputs)
    for k in names:
        if k not in OUTPUTS:
            raise ValueError(f'unknown output {k!r}; the outputs are {OUTPUTS}')
    if len(set(names)) != len(names) or not names:
        raise ValueError(f'outputs must name at least one output and none twice, got {names}')
    return names


def _tensor(shape, dtype, given, dev, stream, name):
    """One tensor of a launch: allocated (on `stream`, when one is given) or `given`, validated: a contiguous tensor of
    that shape and dtype (a torch dtype's name) on `dev`; `name` is what the error message calls it."""
    import torch
    dt = getattr(torch, dtype)
    if given is None:
        with torch.cuda.stream(stream):
            return torch.empty(shape, dtype=dt, device=dev)
    if (not torch.is_tensor(given) or tuple(given.shape) != shape or given.dtype != dt or not given.is_contiguous()
            or given.device != dev):
        raise ValueError(f'{name} must be a contiguous {dtype} tensor {shape} on {dev}')
    return given


def targets(n, size, channels, outputs, out, dev, stream=None):
    """What one launch of n frames writes, (tensors, W, H), after checking `size` = (W, H) and `channels`.
    outputs=None: the uint8 [n, H, W, channels] frame, `out` or a new one.  A tuple of names from OUTPUTS: a dict
    name -> tensor, 'rgb' that frame and the planes [n, H, W] of PLANE_DTYPES; `out` is then None or a dict of
    preallocated tensors holding exactly the names asked for.  With `out` nothing is allocated (the call can be
    captured); what is allocated is allocated on `stream`, when one is given."""
    if channels not in (3, 4):
        raise ValueError(f'channels must be 3 or 4, got {channels}')
    W, H = int(size[0]), int(size[1])
    if not (1 <= W <= MAX_SIDE and 1 <= H <= MAX_SIDE):
        raise ValueError(f'size must be within 1..{MAX_SIDE} each way, got {size}')
    if outputs is None:
        return _tensor((n, H, W, channels), 'uint8', out, dev, stream, 'out'), W, H
    names = check_outputs(outputs)
    if out is not None and (not isinstance(out, dict) or set(out) != set(names)):
        raise ValueError(f'with outputs={names}, out must be a dict holding exactly these names')
    res = {}
    for k in names:
        shape, dtype = ((n, H, W, channels), 'uint8') if k == 'rgb' else ((n, H, W), PLANE_DTYPES[k])
        res[k] = _tensor(shape, dtype, None if out is None else out[k], dev, stream, f'out[{k!r}]')
    return res, W, H


def _call(entry, aux, *args):
    """The one ctypes call of the renderer.  `args` are the plain entry's, the stream last; with `aux` (an Aux) the
    call goes to the entry's _aux sibling, which takes a pointer to it in front of the stream."""
    if aux is not None:
        entry, args = entry + '_aux', (*args[:-1], C.byref(aux), args[-1])
    binding = OBS_BINDING if entry in OBS_SIGNATURES else BINDING   # (the library that exports the entry)
    rc = getattr(binding.load(), entry)(*args)
    if rc:
        binding.check(rc, entry)


def render_into(agent, grid, occ, n, atlas, out, width, height, channels, stream, aux=None):
    """One igw_render_pov call on raw pointers (ints); `atlas` is a device tensor [S, S, 4].  With `aux`, an Aux, one
    igw_render_pov_aux call (out may then be None); so for the two below."""
    _call('igw_render_pov', aux, agent, grid, occ, int(n), atlas.data_ptr(), int(atlas.shape[0]), out, int(width),
          int(height), int(channels), stream)


def render_episodes_into(records, n_records, first, length, frame0, start_grid, init_pose, m, max_length, atlas, out,
                         n_frames, width, height, channels, stream, aux=None):
    """One igw_render_episodes call on raw pointers (ints); `atlas` is a device tensor [S, S, 4]."""
    _call('igw_render_episodes', aux, records, int(n_records), first, length, frame0, start_grid, init_pose, int(m),
          int(max_length), atlas.data_ptr(), int(atlas.shape[0]), out, int(n_frames), int(width), int(height),
          int(channels), stream)


def render_views_into(grids, grid_stride, n_grids, view_grid, pose, m, atlas, out, width, height, channels, stream,
                      aux=None):
    """One igw_render_views call on raw pointers (ints; view_grid may be None); `atlas` is a device tensor [S, S, 4]."""
    _call('igw_render_views', aux, grids, int(grid_stride), int(n_grids), view_grid, pose, int(m), atlas.data_ptr(),
          int(atlas.shape[0]), out, int(width), int(height), int(channels), stream)


def obs_into(agent, grid, occ, n, atlas, out, width, height, obs, stream):
    """One igw_render_pov_obs call on raw pointers (ints); `obs` is an Obs, `out` the frame [n, H, W, 3] or None."""
    _call('igw_render_pov_obs', None, agent, grid, occ, int(n), atlas.data_ptr(), int(atlas.shape[0]), out, int(width),
          int(height), C.byref(obs), stream)


_INTO = {'pov': render_into, 'episodes': render_episodes_into, 'views': render_views_into}


def launch(kind, args, n, size, channels, outputs, out, atlas, dev, stream, alloc_stream=None):
    """One render launch of n frames and what it wrote: the frame tensor, or with `outputs` the dict of targets().
    `kind` is 'pov', 'episodes' or 'views' and `args` that wrapper's arguments in front of `atlas`; `stream` is the raw
    stream of the launch, `alloc_stream` the torch stream to allocate on when it is not the current one.

    The entry rule, here and nowhere else: outputs=None calls the plain entry; a tuple calls the _aux entry with the
    planes not asked for (and `out`, without 'rgb') NULL -- also for ('rgb',), which is the same frame from the other
    kernel.  It touches the device only through data_ptr() and the ctypes call."""
    res, W, H = targets(n, size, channels, outputs, out, dev, alloc_stream)
    if outputs is None:
        rgb, aux = res.data_ptr(), None
    else:
        ptr = lambda k: res[k].data_ptr() if k in res else None  # noqa: E731
        rgb, aux = ptr('rgb'), Aux(ptr('depth'), ptr('label'), ptr('surface'))
    frame = (rgb, n, W, H, channels) if kind == 'episodes' else (rgb, W, H, channels)
    _INTO[kind](*args, atlas, *frame, stream, aux=aux)
    return res


def launch_obs(args, n, size, spec, out, frame, restart, fill, atlas, dev, stream, alloc_stream=None):
    """One igw_render_pov_obs launch of n envs and the observation it wrote, `spec`.shape(n, size) of spec.dtype: `out`
    (the stack the previous launch left, shifted in place) or a new tensor, which is always filled.  `args` are
    obs_into's arguments in front of `atlas`; `frame` is None (no frame: the entry gets out = NULL) or the uint8
    [n, H, W, 3] tensor the frame goes to; `restart` is None or a 1-D uint8 / bool tensor of n elements on `dev`, at
    any stride (env i restarts its stack where element i is not 0); `fill` restarts every env.  With `out` nothing is
    allocated.  It touches the device only through data_ptr() and the ctypes call."""
    W, H = int(size[0]), int(size[1])
    if not (1 <= W <= MAX_SIDE and 1 <= H <= MAX_SIDE):
        raise ValueError(f'size must be within 1..{MAX_SIDE} each way, got {size}')
    name = str(spec.dtype).split('.')[-1]
    data = _tensor(spec.shape(n, (W, H)), name, out, dev, alloc_stream, 'out')
    if frame is not None:
        frame = _tensor((n, H, W, 3), 'uint8', frame, dev, alloc_stream, 'frame')
    ptr, stride = None, 0
    if restart is not None:
        if (not torch.is_tensor(restart) or restart.dtype not in (torch.uint8, torch.bool) or restart.dim() != 1
                or restart.shape[0] != n or restart.device != dev or (n > 1 and restart.stride(0) < 1)):
            raise ValueError(f'restart must be a uint8 or bool tensor [{n}] on {dev}')
        ptr, stride = restart.data_ptr(), max(1, restart.stride(0))
    obs = Obs(data.data_ptr(), OBS_DTYPES[spec.dtype], int(spec.gray), spec.stack, int(bool(fill) or out is None),
              spec.scale, spec.bias, ptr, stride)
    obs_into(*args, atlas, None if frame is None else frame.data_ptr(), W, H, obs, stream)
    return data


# ---- reading the planes ---------------------------------------------------------------------------------------------
def decode_surface(surface):
    """(face, y, x, z) of a `surface` plane (tensor or numpy, any shape): the face code 0..5 (FACES) and the GRID
    indices of the block hit (grid[y, x, z]; world x - 5, y - 1, z - 5), each -1 where the pixel is not a block (sky,
    ground).  For the ground, surface - 6 * 1089 = (qx + 18) * 37 + (qz + 18)."""
    import torch
    if torch.is_tensor(surface):
        s = surface.to(torch.int32)
        block = (s >= 0) & (s < GROUND_FACE * CELLS)
        div = lambda a, b: torch.div(a, b, rounding_mode='floor')  # noqa: E731
        where = torch.where
        minus = torch.full_like(s, -1)
    else:
        s = np.asarray(surface).astype(np.int32)
        block = (s >= 0) & (s < GROUND_FACE * CELLS)
        div = lambda a, b: a // b  # noqa: E731
        where = np.where
        minus = np.full_like(s, -1)
    cell = s % CELLS
    parts = (div(s, CELLS), div(cell, 121), div(cell, 11) % 11, cell % 11)
    return tuple(where(block, p, minus) for p in parts)


def unproject(depth, poses, size=None):
    """World points [M, H, W, 3] (float64 tensor on depth's device) of a depth plane [M, H, W] seen from poses [M, 5]
    (x, y, z, yaw, pitch in degrees): eye + depth * d with the ray d of the camera contract,
    d = f + ((2j+1)/W - 1)(W/H) r + (1 - (2i+1)/H) u for pixel (row i, column j).  NaN where the depth is inf (sky).
    `size` = (W, H), checked against the plane when given.  Pure torch: it runs wherever `depth` lives."""
    import torch
    d = depth if torch.is_tensor(depth) else torch.as_tensor(np.asarray(depth))
    if d.dim() == 2:
        d = d.unsqueeze(0)
    if d.dim() != 3:
        raise ValueError(f'depth must be [M, H, W], got {tuple(d.shape)}')
    M, H, W = d.shape
    if size is not None and (int(size[0]), int(size[1])) != (W, H):
        raise ValueError(f'size {tuple(size)} does not match the depth plane [{M}, {H}, {W}] (size is (W, H))')
    p = poses if torch.is_tensor(poses) else torch.as_tensor(np.asarray(poses, np.float64))
    p = p.to(device=d.device, dtype=torch.float64).reshape(-1, 5)
    if p.shape[0] != M:
        raise ValueError(f'{M} depth planes but {p.shape[0]} poses')
    yaw, pitch = torch.deg2rad(p[:, 3]), torch.deg2rad(p[:, 4])
    sy, cy, sp, cp = torch.sin(yaw), torch.cos(yaw), torch.sin(pitch), torch.cos(pitch)
    zero = torch.zeros_like(sy)
    f = torch.stack([sy * cp, sp, -cy * cp], 1)
    r = torch.stack([cy, zero, sy], 1)
    u = torch.stack([-sy * sp, cp, cy * sp], 1)
    a = ((2 * torch.arange(W, dtype=torch.float64, device=d.device) + 1) / W - 1) * (W / H)
    b = 1 - (2 * torch.arange(H, dtype=torch.float64, device=d.device) + 1) / H
    rays = f[:, None, None, :] + a[None, None, :, None] * r[:, None, None, :] + b[None, :, None, None] * u[:, None, None, :]
    t = d.to(torch.float64)
    pts = p[:, None, None, :3] + t[..., None] * rays
    return torch.where(torch.isfinite(t)[..., None], pts, torch.full_like(pts, float('nan')))


if __name__ == '__main__':
    print(build(force='--force' in sys.argv, verbose=True))
