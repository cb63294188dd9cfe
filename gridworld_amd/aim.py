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
import sys

from . import _out
from . import build as _build

VERSION = 1
ROW = 1104          # int32 words per env and plane
CELLS = 1089
MAX_TURNS = 72
HALF = 36           # di = -36..35, dj = -36..36; a code holds di + 36 and dj + 36
NONE = -1
OUTPUTS = ('place', 'break')   # in the order igw_aim takes them
_vp, _i32 = C.c_void_p, C.c_int32


class AimError(RuntimeError):
    pass


# include/igw_aim.h declares igw_aim and the three symbols every library has: (result, arguments)
LIBRARY, BINDING = _build.query('aim', __file__, {
    'igw_aim': (C.c_int, [_vp, _vp, _i32, _i32, _vp, _vp, _vp]),
}, AimError, 'igw_aim')
LIB, SOURCES, HEADERS = LIBRARY.lib, LIBRARY.sources, LIBRARY.headers
SIGNATURES, EXPORTS = BINDING.signatures, list(BINDING.signatures)
build, source_hash, built_id, is_stale = LIBRARY.build, LIBRARY.source_hash, LIBRARY.built_id, LIBRARY.is_stale
load, check, build_id = BINDING.load, BINDING.check, BINDING.build_id


def aim_into(agent, occ, n, max_turns, place, brk, stream):
    """One igw_aim call on raw pointers (ints; place or brk may be None)."""
    rc = BINDING.load().igw_aim(agent, occ, int(n), int(max_turns), place, brk, stream)
    if rc:
        BINDING.check(rc, 'igw_aim')


def _specs(n):
    """name -> _out.spec of a plane: an int32 [n, 9, 11, 11] view of 1104-word rows, 16-byte aligned."""
    import torch
    plane = _out.spec((n, 9, 11, 11), torch.int32, (ROW, 121, 11, 1), 16, (n, ROW))
    return {'place': plane, 'break': plane}


def plane(n, dev, stream=None):
    """A new output plane as aim() returns it."""
    return _out.outputs('aim', OUTPUTS, ('place',), _specs(n), None, dev, stream)[0]['place']


def launch(agent, occ, n, max_turns, place, brk, out, dev, stream, alloc_stream=None):
    """One igw_aim launch over n envs; returns the dict of the planes asked for, 'place' and / or 'break'.  `agent` /
    `occ` are the state tensors' rows; place / brk are bools; `out` (a dict or None) holds planes to write, as an
    earlier call returned them; what it lacks is allocated, so with every plane given nothing is.  It touches the
    device only through data_ptr() and the ctypes call."""
    if not 0 <= int(max_turns) <= MAX_TURNS:
        raise ValueError(f'max_turns must be 0..{MAX_TURNS}, not {max_turns}')
    names = [k for k, w in (('place', place), ('break', brk)) if w]
    if not names:
        raise ValueError('aim: place and brk are both off, nothing to compute')
    res, ptrs = _out.outputs('aim', OUTPUTS, names, _specs(n), out, dev, alloc_stream)
    aim_into(agent.data_ptr(), occ.data_ptr(), n, max_turns, *ptrs, stream)
    return res


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
