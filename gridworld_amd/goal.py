"""The goal query of the step path: builds and binds libigw_goal.so (include/igw_goal.h).

    g = env.goal()                                  # align int8 [N, 3], fit int16 [N, 4], todo int8 [N, 9, 11, 11]
    g = env.goal(want=True, gain=True)              # + want, gain float32 [N, 18], ends uint8 [N, 18]
    VecGridWorld(..., goal=True)                    # reset() / step() also return obs['align'], ['fit'], ['todo']
    goal_world(g['want'], start)                    # the block ids wanted in the world, -1 elsewhere

The library is a separate one, as the renderer's, the codec's and the query's are: it reads the step path's state
buffers (include/igw.h) and is not part of the step library's build (its sources and build id are its own, so the step
library's profiles stay valid).  There is no CPU fallback: without a HIP device the launch fails and the call raises.
"""
import ctypes as C
import sys

from . import _out
from . import build as _build

VERSION = 1
ACTIONS = 18
GRID_STRIDE = 1104
OUTPUTS = ('align', 'fit', 'want', 'todo', 'gain', 'ends')   # in the order igw_goal takes them
_vp, _i32, _f64 = C.c_void_p, C.c_int32, C.c_double


class GoalError(RuntimeError):
    pass


# include/igw_goal.h declares igw_goal and the three symbols every library has: (result, arguments)
LIBRARY, BINDING = _build.query('goal', __file__, {
    'igw_goal': (C.c_int, [_vp] * 8 + [_i32, _f64, _f64, _i32, _i32] + [_vp] * 9),
}, GoalError, 'igw_goal', headers=['igw_vote.h'])
LIB, SOURCES, HEADERS = LIBRARY.lib, LIBRARY.sources, LIBRARY.headers
SIGNATURES, EXPORTS = BINDING.signatures, list(BINDING.signatures)
build, source_hash, built_id, is_stale = LIBRARY.build, LIBRARY.source_hash, LIBRARY.built_id, LIBRARY.is_stale
load, check, build_id = BINDING.load, BINDING.check, BINDING.build_id


def goal_into(state, n, right_scale, wrong_scale, max_steps, select_and_place, mask, look, outputs, stream):
    """One igw_goal call on raw pointers (ints): `state` the eight state / task-table pointers in the header's order,
    `outputs` the six of OUTPUTS (None = not wanted); mask / look may be None without gain and ends."""
    rc = BINDING.load().igw_goal(*state, int(n), float(right_scale), float(wrong_scale), int(max_steps),
                                 int(bool(select_and_place)), mask, look, *outputs, stream)
    if rc:
        BINDING.check(rc, 'igw_goal')


def _specs(n):
    """name -> _out.spec of the tensor a caller sees: `align` is an [n, 3] view of four bytes per env, `want` / `todo`
    [n, 9, 11, 11] views of 1104-byte rows (the layout of `grid`); the pad byte and the rows' padding are zeros."""
    import torch
    grid = _out.spec((n, 9, 11, 11), torch.int8, (GRID_STRIDE, 121, 11, 1), 16, (n, GRID_STRIDE), zero=True)
    flat = lambda cols, dtype, width, align: _out.spec((n, cols), dtype, (width, 1), align, (n, width), zero=True)  # noqa: E731
    return {'align': flat(3, torch.int8, 4, 4), 'fit': flat(4, torch.int16, 4, 8), 'want': grid, 'todo': grid,
            'gain': flat(ACTIONS, torch.float32, ACTIONS, 4), 'ends': flat(ACTIONS, torch.uint8, ACTIONS, 1)}


def outputs(n, names, dev, stream=None):
    """New tensors for the outputs `names`, as goal() returns them."""
    return _out.outputs('goal', OUTPUTS, names, _specs(n), None, dev, stream)[0]


def launch(state, n, reward, mask, look, names, out, dev, stream, alloc_stream=None):
    """One igw_goal launch over n envs; returns the dict name -> tensor of `names` (a subset of OUTPUTS).  `state`:
    the eight state / task-table tensors' rows; `reward` = (right_scale, wrong_scale, max_steps, select_and_place);
    mask / look: the tensors igw_action_mask wrote (None without gain / ends).  `out` (a dict or None) holds tensors
    to write, as an earlier call returned them; what it lacks is allocated.  It touches the device only through
    data_ptr() and the ctypes call."""
    res, ptrs = _out.outputs('goal', OUTPUTS, names, _specs(n), out, dev, alloc_stream)
    goal_into([t.data_ptr() for t in state], n, *reward, _out.ptr(mask), _out.ptr(look), ptrs, stream)
    return res


def goal_world(want, start):
    """The world colours wanted: `want` (the aligned synthetic target, goal()['want']) + `start` (the starting grid,
    broadcastable to it) where that is a block id 0..6, -1 elsewhere (a synthetic value that no single block gives)."""
    import torch
    w = want.to(torch.int16) + torch.as_tensor(start, device=want.device).to(torch.int16)
    return torch.where((w >= 0) & (w <= 6), w, torch.full_like(w, -1)).to(torch.int8)


if __name__ == '__main__':
    print(build(force='--force' in sys.argv, verbose=True))
