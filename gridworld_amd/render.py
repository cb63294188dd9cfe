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

from . import build as _build

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc', 'render')
LIB = os.path.join(HERE, 'libigw_render.so')
SOURCES = [os.path.join(CSRC, 'igw_render.hip')]
HEADERS = [os.path.join(CSRC, 'igw_render_frame.h'), os.path.join(HERE, '..', 'include', 'igw_render.h')]
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
EXPORTS = list(SIGNATURES)
# the library as build.py builds it: the step library's FLAGS, an id of its own (igw_render_build_id())
LIBRARY = _build.Library(LIB, SOURCES, HEADERS, 'igw-render-build-id:', 'IGW_RENDER_BUILD_ID', deps=[__file__])
source_hash, built_id, is_stale = LIBRARY.source_hash, LIBRARY.built_id, LIBRARY.is_stale


class RenderError(RuntimeError):
    pass


def build(force=False, verbose=False):
    return LIBRARY.build(force, verbose=verbose)


_lib = None


def load(build_if_missing=True):
    """Loads libigw_render.so, building it first if it is missing or stale; a failed compile raises."""
    global _lib
    if _lib is not None:
        return _lib
    if build_if_missing:
        LIBRARY.build_for_load(RenderError)
    if not os.path.exists(LIB):
        raise RenderError('libigw_render.so not found; run `python -m gridworld_amd.render`')
    L = C.CDLL(LIB)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    _lib = L
    return L


def build_id():
    return load().igw_render_build_id().decode()


def check(code, what='igw_render_pov'):
    if code != 0:
        msg = load().igw_render_last_error()
        raise RenderError(f'{what} failed ({code}): {msg.decode() if msg else ""}')


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
def frame_tensor(n, size, channels, out, dev, stream=None):
    """The frames of one launch, (out, W, H): checks `size` = (W, H) and `channels`, then allocates (on `stream`, when
    one is given) or validates `out`, a contiguous uint8 tensor [n, H, W, channels] on `dev`."""
    import torch
    if channels not in (3, 4):
        raise ValueError(f'channels must be 3 or 4, got {channels}')
    W, H = int(size[0]), int(size[1])
    if not (1 <= W <= MAX_SIDE and 1 <= H <= MAX_SIDE):
        raise ValueError(f'size must be within 1..{MAX_SIDE} each way, got {size}')
    shape = (n, H, W, channels)
    if out is None:
        with torch.cuda.stream(stream):
            out = torch.empty(shape, dtype=torch.uint8, device=dev)
    elif (not torch.is_tensor(out) or tuple(out.shape) != shape or out.dtype != torch.uint8
          or not out.is_contiguous() or out.device != dev):
        raise ValueError(f'out must be a contiguous uint8 tensor {shape} on {dev}')
    return out, W, H


def _call(entry, *args):
    rc = getattr(load(), entry)(*args)
    if rc:
        check(rc, entry)


def render_into(agent, grid, occ, n, atlas, out, width, height, channels, stream):
    """One igw_render_pov call on raw pointers (ints); `atlas` is a device tensor [S, S, 4]."""
    _call('igw_render_pov', agent, grid, occ, int(n), atlas.data_ptr(), int(atlas.shape[0]), out, int(width),
          int(height), int(channels), stream)


def render_episodes_into(records, n_records, first, length, frame0, start_grid, init_pose, m, max_length, atlas, out,
                         n_frames, width, height, channels, stream):
    """One igw_render_episodes call on raw pointers (ints); `atlas` is a device tensor [S, S, 4]."""
    _call('igw_render_episodes', records, int(n_records), first, length, frame0, start_grid, init_pose, int(m),
          int(max_length), atlas.data_ptr(), int(atlas.shape[0]), out, int(n_frames), int(width), int(height),
          int(channels), stream)


def render_views_into(grids, grid_stride, n_grids, view_grid, pose, m, atlas, out, width, height, channels, stream):
    """One igw_render_views call on raw pointers (ints; view_grid may be None); `atlas` is a device tensor [S, S, 4]."""
    _call('igw_render_views', grids, int(grid_stride), int(n_grids), view_grid, pose, int(m), atlas.data_ptr(),
          int(atlas.shape[0]), out, int(width), int(height), int(channels), stream)


if __name__ == '__main__':
    print(build(force='--force' in sys.argv, verbose=True))
