"""The aim query of the step path: builds and binds libigw_aim.so (include/igw_aim.h).

    a = env.aim()                                   # {'place', 'break'}: int32 [N, 9, 11, 11], the cheapest turn per cell
    a = env.aim(max_turns=6, brk=False)             # a smaller window, one plane
    turns, dyaw, dpitch = aim_decode(a['place'])    # -1 where no turn reaches the cell
    action = aim_action(a['place'], cells)          # the next action towards placing at cells[i]: 12..15, then 17

The library is a separate one, as the renderer's, the codec's, the query's and the goal's are: it reads the step path's
state buffers (include/igw.h) and is not part of the step library's build (its sources and build id are its own, so
the step library's profiles stay valid).  There is no CPU fallback: without a HIP device the launch fails and the call
raises.
"""
import ctypes as C
import os
import sys

from . import build as _build

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIB = os.path.join(HERE, 'libigw_aim.so')
SOURCES = [os.path.join(CSRC, 'aim', 'igw_aim.hip')]
HEADERS = [os.path.join(CSRC, f) for f in ('igw_device.h', 'igw_trig.h', 'igw_trig_lut.h', 'igw_trig_tables.h')] + \
          [os.path.join(HERE, '..', 'include', 'igw.h'), os.path.join(HERE, '..', 'include', 'igw_aim.h')]
VERSION = 1
ROW = 1104          # int32 words per env and plane
CELLS = 1089
MAX_TURNS = 72
HALF = 36           # di = -36..35, dj = -36..36; a code holds di + 36 and dj + 36
NONE = -1
_vp, _i32 = C.c_void_p, C.c_int32
# every symbol include/igw_aim.h declares: (result, arguments)
SIGNATURES = {
    'igw_aim_version': (C.c_int, []),
    'igw_aim_build_id': (C.c_char_p, []),
    'igw_aim_last_error': (C.c_char_p, []),
    'igw_aim': (C.c_int, [_vp, _vp, _i32, _i32, _vp, _vp, _vp]),
}
EXPORTS = list(SIGNATURES)
LIBRARY = _build.Library(LIB, SOURCES, HEADERS, 'igw-aim-build-id:', 'IGW_AIM_BUILD_ID', deps=[__file__])
source_hash, built_id, is_stale = LIBRARY.source_hash, LIBRARY.built_id, LIBRARY.is_stale


class AimError(RuntimeError):
    pass


def build(force=False, verbose=False):
    """Builds libigw_aim.so; returns its path."""
    return LIBRARY.build(force, verbose=verbose)


BINDING = _build.Binding(LIBRARY, SIGNATURES, AimError, 'igw_aim_last_error', 'igw_aim_build_id',
                         'gridworld_amd.aim', 'igw_aim')
load, check, build_id = BINDING.load, BINDING.check, BINDING.build_id


def aim_into(agent, occ, n, max_turns, place, brk, stream):
    """One igw_aim call on raw pointers (ints; place or brk may be None)."""
    rc = BINDING.load().igw_aim(agent, occ, int(n), int(max_turns), place, brk, stream)
    if rc:
        BINDING.check(rc, 'igw_aim')


def plane(n, dev, stream=None):
    """A new output plane as aim() returns it: an int32 [n, 9, 11, 11] view of 1104-word rows."""
    import torch
    with torch.cuda.stream(stream):
        base = torch.empty((n, ROW), dtype=torch.int32, device=dev)
    return torch.as_strided(base, (n, 9, 11, 11), (ROW, 121, 11, 1))


def launch(agent, occ, n, max_turns, place, brk, out, dev, stream, alloc_stream=None):
    """One igw_aim launch over n envs; returns the dict of the planes asked for, 'place' and / or 'break'.  `agent` /
    `occ` are the state tensors' rows; place / brk are bools; `out` (a dict or None) holds planes to write, as an
    earlier call returned them; what it lacks is allocated, so with every plane given nothing is.  It touches the
    device only through data_ptr() and the ctypes call."""
    import torch
    if not 0 <= int(max_turns) <= MAX_TURNS:
        raise ValueError(f'max_turns must be 0..{MAX_TURNS}, not {max_turns}')
    names = [k for k, w in (('place', place), ('break', brk)) if w]
    if not names:
        raise ValueError('aim: place and brk are both off, nothing to compute')
    out = dict(out or {})
    unknown = [k for k in out if k not in names]
    if unknown:
        raise ValueError(f'out holds {unknown}, the call writes {names}')
    shape, strides = (n, 9, 11, 11), (ROW, 121, 11, 1)
    for k, t in out.items():
        if (not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != torch.int32 or t.device != dev
                or (n > 0 and tuple(t.stride()) != strides) or t.data_ptr() % 16):
            raise ValueError(f'out[{k!r}] must be an int32 tensor {shape} with strides {strides} on {dev}, 16-byte '
                             'aligned (what aim() returns)')
    for k in names:
        if k not in out:
            out[k] = plane(n, dev, alloc_stream)
    ptr = lambda k: out[k].data_ptr() if k in out else None  # noqa: E731
    aim_into(agent.data_ptr(), occ.data_ptr(), n, max_turns, ptr('place'), ptr('break'), stream)
    return {k: out[k] for k in names}


def aim_decode(code):
    """(turns, dyaw_steps, dpitch_steps) of the codes of aim(), integer tensors of the codes' shape: the camera actions
    to play are |dyaw_steps| times 12 (negative) or 13 and |dpitch_steps| times 14 (negative) or 15.  Where the code is
    -1 (no turn reaches the cell) turns is -1 and the steps are 0."""
    import torch
    code = torch.as_tensor(code)
    none = code < 0
    zero = torch.zeros_like(code)
    turns = torch.where(none, torch.full_like(code, NONE), code >> 16)
    return turns, torch.where(none, zero, (code & 0xff) - HALF), torch.where(none, zero, ((code >> 8) & 0xff) - HALF)


def aim_action(code, cells, kind='place'):
    """The next action of the sequence that aim() names for cell cells[i] of env i: int32 [N].  `code` is a plane of
    aim() ([N, 9, 11, 11], or anything with 1089 cells per env), `cells` an integer tensor [N] of flat cell indices, -1
    for none.  12 while the yaw has to go down, else 13 while it has to go up, then 14 / 15 for the pitch, then 17
    (kind='place') or 16 (kind='break') once the camera points there; 0 where the cell is -1 or cannot be reached.
    Plain torch on the codes' device."""
    import torch
    if kind not in ('place', 'break'):
        raise ValueError("kind must be 'place' or 'break'")
    cells = torch.as_tensor(cells, device=code.device).long()
    flat = code.reshape(code.shape[0], -1)
    picked = flat.gather(1, cells.clamp(0, flat.shape[1] - 1).unsqueeze(1)).squeeze(1)
    picked = torch.where((cells < 0) | (cells >= flat.shape[1]), torch.full_like(picked, NONE), picked)
    turns, di, dj = aim_decode(picked)
    act = torch.full_like(picked, 17 if kind == 'place' else 16)
    act = torch.where(dj > 0, torch.full_like(act, 15), act)
    act = torch.where(dj < 0, torch.full_like(act, 14), act)
    act = torch.where(di > 0, torch.full_like(act, 13), act)
    act = torch.where(di < 0, torch.full_like(act, 12), act)
    return torch.where(turns < 0, torch.zeros_like(act), act).to(torch.int32)


if __name__ == '__main__':
    print(build(force='--force' in sys.argv, verbose=True))
