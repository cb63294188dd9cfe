"""The voxel observation of the vector-state path: builds and binds libigw_vox.so (include/igw_vox.h).

    spec = G.VoxSpec(planes=(('grid', 'onehot'), ('target', 'onehot')), agent=True, dtype=torch.float16, stack=4)
    x = env.vox_obs(spec)                            # [N, K * C, 9, S, S]: what a 3-D convolution takes
    x = env.vox_obs(spec, out=x, restart=env.done)   # shifted in place, nothing allocated
    env = VecGridWorld(n, vox_obs=spec)              # obs['vox_obs'], rewritten after every reset() / step()
    G.vox_channel_names(spec)                        # ['grid:1', ..., 'target:6', 'agent'] of one slot

The library is a separate one, as the renderer's, the codec's and the queries' are: it reads the step path's state
buffers (include/igw.h) and is not part of the step library's build (its sources and build id are its own, so the step
library's profiles stay valid); the element, the frame of a pose, the staging of the planes and the slot writer
(csrc/igw_voxel.h, igw_voxel_table.h, igw_voxel_stage.h) it shares with the recall query's library.  There is no CPU
fallback: without a HIP device the launch fails and the call raises.
"""
import ctypes as C
import sys

import numpy as np
import torch

from . import _out
from . import build as _build

VERSION = 1
MAX_SOURCES, MAX_STACK, MAX_RADIUS, CELLS, LEVELS = 4, 8, 10, 1089, 9
ONEHOT, OCC = 0, 1
WORLD, EGO = 0, 1
ENCODINGS = {'onehot': ONEHOT, 'occ': OCC}
FRAMES = {'world': WORLD, 'ego': EGO}
PLANES = ('grid', 'target', 'want', 'todo')
DTYPES = {torch.uint8: 0, torch.float16: 1, torch.bfloat16: 2, torch.float32: 3}   # IGW_VOX_U8 / F16 / BF16 / F32
_vp, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64


class Source(C.Structure):
    """igw_vox_source (`rows` and `add` are device pointers)."""
    _fields_ = [('rows', _vp), ('add', _vp), ('row_stride', _i64), ('by_task', _i32), ('encoding', _i32)]


class Spec(C.Structure):
    """igw_vox_spec (`data` and `restart` are device pointers)."""
    _fields_ = [('sources', Source * MAX_SOURCES), ('num_sources', _i32), ('agent_plane', _i32), ('frame', _i32),
                ('radius', _i32), ('dtype', _i32), ('stack', _i32), ('fill', _i32), ('reserved', _i32),
                ('scale', C.c_float), ('bias', C.c_float), ('data', _vp), ('restart', _vp), ('restart_stride', _i64)]


class VoxError(RuntimeError):
    pass


# include/igw_vox.h declares igw_vox_obs and the three symbols every library has: (result, arguments)
LIBRARY, BINDING = _build.query('vox', __file__, {
    'igw_vox_obs': (C.c_int, [_vp, _vp, _i32, C.POINTER(Spec), _vp]),
}, VoxError, 'igw_vox_obs', headers=['igw_voxel.h', 'igw_voxel_table.h', 'igw_voxel_stage.h'], device=False)
LIB, SOURCES, HEADERS = LIBRARY.lib, LIBRARY.sources, LIBRARY.headers
SIGNATURES, EXPORTS = BINDING.signatures, list(BINDING.signatures)
build, source_hash, built_id, is_stale = LIBRARY.build, LIBRARY.source_hash, LIBRARY.built_id, LIBRARY.is_stale
load, check, build_id = BINDING.load, BINDING.check, BINDING.build_id


class VoxSpec:
    """The layout of a voxel observation (include/igw_vox.h: igw_vox_spec).  `planes`: up to four (name, encoding)
    pairs -- name 'grid' (the live grid), 'target' (the task's target grid), 'want' / 'todo' (the goal query's rows);
    encoding 'onehot' (6 channels, [v == 1] .. [v == 6]) or 'occ' (1 channel, [v != 0]); a name may appear once per
    encoding.  agent = one more channel, 1 at the two cells of the agent's body.  frame 'world' (S = 11) or 'ego' (the
    x / z window of `radius` R = 1..10 cells around the agent, turned by its heading quadrant; S = 2 R + 1).  `dtype`
    torch.uint8, float16, bfloat16 or float32; the float types hold bit * scale + bias (uint8 takes scale 1, bias 0);
    stack = K, the last K observations (1..8), oldest first.  Validated on construction (ValueError; no device
    needed)."""

    def __init__(self, planes=(('grid', 'onehot'), ('target', 'onehot')), agent=True, frame='world', radius=5,
                 dtype=torch.uint8, stack=1, scale=1.0, bias=0.0):
        try:
            planes = tuple((str(name), str(enc)) for name, enc in planes)
        except (TypeError, ValueError):
            raise ValueError(f'planes must be (name, encoding) pairs, got {planes!r}') from None
        if not 1 <= len(planes) <= MAX_SOURCES:
            raise ValueError(f'planes must name 1..{MAX_SOURCES} (name, encoding) pairs, got {len(planes)}')
        for name, enc in planes:
            if name not in PLANES:
                raise ValueError(f'a plane is one of {PLANES}, got {name!r}')
            if enc not in ENCODINGS:
                raise ValueError(f'an encoding is one of {tuple(ENCODINGS)}, got {enc!r}')
        if len(set(planes)) != len(planes):
            raise ValueError(f'a plane may appear once per encoding, got {planes!r}')
        if frame not in FRAMES:
            raise ValueError(f'frame must be one of {tuple(FRAMES)}, got {frame!r}')
        if isinstance(radius, bool) or int(radius) != radius or not 1 <= int(radius) <= MAX_RADIUS:
            raise ValueError(f'radius must be an integer in 1..{MAX_RADIUS}, got {radius!r}')
        if isinstance(dtype, str):
            dtype = getattr(torch, dtype, dtype)
        if dtype not in DTYPES:
            raise ValueError(f'dtype must be torch.uint8, float16, bfloat16 or float32, got {dtype!r}')
        if isinstance(stack, bool) or int(stack) != stack or not 1 <= int(stack) <= MAX_STACK:
            raise ValueError(f'stack must be an integer in 1..{MAX_STACK}, got {stack!r}')
        scale, bias = float(scale), float(bias)
        top = float(np.finfo(np.float32).max)   # (the kernel takes them as float32)
        if not (abs(scale) <= top and abs(bias) <= top):
            raise ValueError(f'scale and bias must be finite float32 values, got {scale!r}, {bias!r}')
        if dtype is torch.uint8 and (scale != 1.0 or bias != 0.0):
            raise ValueError('a uint8 observation takes scale 1 and bias 0')
        self.planes, self.agent, self.frame, self.radius = planes, bool(agent), frame, int(radius)
        self.dtype, self.stack, self.scale, self.bias = dtype, int(stack), scale, bias
        self.channels = sum(6 if enc == 'onehot' else 1 for _, enc in planes) + int(self.agent)
        self.size = 11 if frame == 'world' else 2 * self.radius + 1

    @classmethod
    def of(cls, spec):
        """A VoxSpec as it is, or one from a dict of its arguments."""
        if isinstance(spec, cls):
            return spec
        if isinstance(spec, dict):
            return cls(**spec)
        raise ValueError(f'a voxel observation is a VoxSpec or a dict of its arguments, got {type(spec).__name__}')

    def needs(self):
        """The goal query's outputs among the planes' names."""
        return tuple(k for k in ('want', 'todo') if any(name == k for name, _ in self.planes))

    def shape(self, n):
        """(n, K * C, 9, S, S): slot k holds channels [k * C, (k + 1) * C)."""
        return (int(n), self.stack * self.channels, LEVELS, self.size, self.size)

    def __repr__(self):
        return (f'VoxSpec(planes={self.planes}, agent={self.agent}, frame={self.frame!r}, radius={self.radius}, '
                f'dtype={self.dtype}, stack={self.stack}, scale={self.scale}, bias={self.bias})')


def vox_channel_names(spec):
    """The C channels of one slot of `spec` (a VoxSpec or a dict), in order: 'grid:1' .. 'grid:6' for a one-hot plane
    (the colour id), the plane's name for an occupancy plane, 'agent'."""
    spec = VoxSpec.of(spec)
    names = []
    for name, enc in spec.planes:
        names += [f'{name}:{k}' for k in range(1, 7)] if enc == 'onehot' else [name]
    return names + (['agent'] if spec.agent else [])


def vox_into(agent, aux, n, spec, stream):
    """One igw_vox_obs call on raw pointers (ints) and a filled Spec."""
    rc = BINDING.load().igw_vox_obs(agent, aux, int(n), C.byref(spec), stream)
    if rc:
        BINDING.check(rc, 'igw_vox_obs')


def rows_of(name, t, n):
    """(pointer, row stride in bytes) of a source given as an int8 tensor [n, 9, 11, 11] -- contiguous or a view of
    wider rows, as `grid` and the goal query's planes are -- or [n, >= 1089]."""
    ok = torch.is_tensor(t) and t.dtype == torch.int8 and t.shape[0] == n and (
        (t.dim() == 4 and tuple(t.shape[1:]) == (9, 11, 11) and tuple(t.stride()[1:]) == (121, 11, 1)) or
        (t.dim() == 2 and t.shape[1] >= CELLS and t.stride(1) == 1))
    if not ok or (n > 1 and t.stride(0) < CELLS):
        raise ValueError(f'{name} must be an int8 tensor [{n}, 9, 11, 11] with dense cells (rows of >= 1089 bytes)')
    return t.data_ptr(), max(CELLS, t.stride(0))


def launch(agent, aux, n, spec, sources, out, restart, fill, dev, stream, alloc_stream=None):
    """One igw_vox_obs launch over n envs and the observation it wrote, `spec`.shape(n) of spec.dtype: `out` (the stack
    the previous launch left, shifted in place) or a new tensor, which is always filled.  `agent` / `aux`: the record
    tensors' rows; `sources`: per plane of the spec (rows pointer, add pointer or None, row stride, by_task);
    `restart`: None or a 1-D uint8 / bool tensor of n elements on `dev`, at any stride.  With `out` nothing is
    allocated.  It touches the device only through data_ptr() and the ctypes call."""
    res, (data,) = _out.outputs('vox_obs', ('obs',), ('obs',), {'obs': _out.spec(spec.shape(n), spec.dtype)},
                                None if out is None else {'obs': out}, dev, alloc_stream)
    ptr, stride = None, 0
    if restart is not None:
        if (not torch.is_tensor(restart) or restart.dtype not in (torch.uint8, torch.bool) or restart.dim() != 1
                or restart.shape[0] != n or restart.device != dev or (n > 1 and restart.stride(0) < 1)):
            raise ValueError(f'restart must be a uint8 or bool tensor [{n}] on {dev}')
        ptr, stride = restart.data_ptr(), max(1, restart.stride(0))
    s = Spec()
    for k, ((_, enc), (rows, add, row_stride, by_task)) in enumerate(zip(spec.planes, sources)):
        s.sources[k] = Source(rows, add, int(row_stride), int(bool(by_task)), ENCODINGS[enc])
    s.num_sources, s.agent_plane, s.frame, s.radius = len(spec.planes), int(spec.agent), FRAMES[spec.frame], spec.radius
    s.dtype, s.stack, s.fill, s.scale, s.bias = DTYPES[spec.dtype], spec.stack, int(bool(fill) or out is None), \
        spec.scale, spec.bias
    s.data, s.restart, s.restart_stride = data, ptr, stride
    vox_into(agent.data_ptr(), aux.data_ptr(), n, s, stream)
    return res['obs']


if __name__ == '__main__':
    print(build(force='--force' in sys.argv, verbose=True))
