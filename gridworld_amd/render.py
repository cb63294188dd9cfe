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
import hashlib
import os
import subprocess
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
EXPORTS = ['igw_render_version', 'igw_render_build_id', 'igw_render_last_error', 'igw_render_pov',
           'igw_render_episodes', 'igw_render_views']
_MARK = b'igw-render-build-id:'


class RenderError(RuntimeError):
    pass


def source_hash():
    """sha256 (16 hex digits) over the renderer's source, its header and the compiler flags: igw_render_build_id()."""
    h = hashlib.sha256()
    for f in sorted(SOURCES + HEADERS, key=os.path.basename):
        h.update(os.path.basename(f).encode() + b'\0')
        with open(f, 'rb') as fh:
            h.update(fh.read())
    h.update(' '.join(_build.FLAGS).encode())
    return h.hexdigest()[:16]


def built_id(lib=LIB):
    """igw_render_build_id() of a library file, read without loading it."""
    try:
        with open(lib, 'rb') as f:
            data = f.read()
        i = data.find(_MARK)
        if i < 0:
            return None
        return data[i + len(_MARK):data.index(b'\0', i)].decode()
    except (OSError, ValueError):
        return None


def is_stale(lib=LIB):
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    deps = SOURCES + HEADERS + [os.path.abspath(__file__)]
    return any(os.path.getmtime(d) > t for d in deps) or built_id(lib) != source_hash()


def build(force=False, verbose=False):
    """hipcc with the step library's FLAGS, under an exclusive file lock, installed by an atomic rename."""
    if not force and not is_stale():
        return LIB
    import fcntl
    with open(LIB + '.lock', 'w') as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if not force and not is_stale():
                return LIB
            tmp = f'{LIB}.tmp.{os.getpid()}'
            cmd = ([_build.hipcc()] + _build.FLAGS + ['-DIGW_RENDER_BUILD_ID="igw-render-build-id:%s"' % source_hash(),
                                                      '-o', tmp] + SOURCES)
            if verbose:
                print(' '.join(cmd))
            subprocess.run(cmd, check=True)
            os.replace(tmp, LIB)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return LIB


_lib = None


def load(build_if_missing=True):
    """Loads libigw_render.so, building it first if it is missing or stale; a failed compile raises."""
    global _lib
    if _lib is not None:
        return _lib
    if build_if_missing:
        try:
            build()
        except subprocess.CalledProcessError as e:
            raise RenderError(f'hipcc failed to build libigw_render.so: {e}') from e
        except Exception as e:  # no hipcc: an existing library is still usable, a missing one is fatal
            if not os.path.exists(LIB):
                raise RenderError(f'libigw_render.so is missing and could not be built: {e}') from e
    if not os.path.exists(LIB):
        raise RenderError('libigw_render.so not found; run `python -m gridworld_amd.render`')
    L = C.CDLL(LIB)
    vp, i32 = C.c_void_p, C.c_int32
    L.igw_render_version.restype = C.c_int
    L.igw_render_build_id.restype = C.c_char_p
    L.igw_render_last_error.restype = C.c_char_p
    L.igw_render_pov.argtypes = [vp, vp, vp, i32, vp, i32, vp, i32, i32, i32, vp]
    L.igw_render_pov.restype = C.c_int
    i64 = C.c_int64
    L.igw_render_episodes.argtypes = [vp, i64, vp, vp, vp, vp, vp, i32, i32, vp, i32, vp, i64, i32, i32, i32, vp]
    L.igw_render_episodes.restype = C.c_int
    L.igw_render_views.argtypes = [vp, i64, i32, vp, vp, i32, vp, i32, vp, i32, i32, i32, vp]
    L.igw_render_views.restype = C.c_int
    _lib = L
    return L


def build_id():
    return load().igw_render_build_id().decode()


def check(code, what='igw_render_pov'):
    if code != 0:
        msg = load().igw_render_last_error()
        raise RenderError(f'{what} failed ({code}): {msg.decode() if msg else ""}')


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


# ---- rendering ----------------------------------------------------------------------------------------------------
def render_into(agent, grid, occ, n, atlas, out, width, height, channels, stream):
    """One igw_render_pov call on raw pointers (ints); `atlas` is a device tensor [S, S, 4]."""
    L = load()
    rc = L.igw_render_pov(agent, grid, occ, int(n), atlas.data_ptr(), int(atlas.shape[0]), out, int(width),
                          int(height), int(channels), stream)
    if rc:
        check(rc)


def render_episodes_into(records, n_records, first, length, frame0, start_grid, init_pose, m, max_length, atlas, out,
                         n_frames, width, height, channels, stream):
    """One igw_render_episodes call on raw pointers (ints); `atlas` is a device tensor [S, S, 4]."""
    L = load()
    rc = L.igw_render_episodes(records, int(n_records), first, length, frame0, start_grid, init_pose, int(m),
                               int(max_length), atlas.data_ptr(), int(atlas.shape[0]), out, int(n_frames), int(width),
                               int(height), int(channels), stream)
    if rc:
        check(rc, 'igw_render_episodes')


def render_views_into(grids, grid_stride, n_grids, view_grid, pose, m, atlas, out, width, height, channels, stream):
    """One igw_render_views call on raw pointers (ints; view_grid may be None); `atlas` is a device tensor [S, S, 4]."""
    L = load()
    rc = L.igw_render_views(grids, int(grid_stride), int(n_grids), view_grid, pose, int(m), atlas.data_ptr(),
                            int(atlas.shape[0]), out, int(width), int(height), int(channels), stream)
    if rc:
        check(rc, 'igw_render_views')


if __name__ == '__main__':
    print(build(force='--force' in sys.argv, verbose=True))
