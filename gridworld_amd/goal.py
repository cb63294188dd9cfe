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
import os
import sys

from . import build as _build

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIB = os.path.join(HERE, 'libigw_goal.so')
SOURCES = [os.path.join(CSRC, 'goal', 'igw_goal.hip')]
HEADERS = [os.path.join(CSRC, f) for f in ('igw_device.h', 'igw_trig.h', 'igw_trig_lut.h', 'igw_trig_tables.h',
                                            'igw_vote.h')] + \
          [os.path.join(HERE, '..', 'include', 'igw.h'), os.path.join(HERE, '..', 'include', 'igw_goal.h')]
VERSION = 1
ACTIONS = 18
GRID_STRIDE = 1104
OUTPUTS = ('align', 'fit', 'want', 'todo', 'gain', 'ends')   # in the order igw_goal takes them
_vp, _i32, _f64 = C.c_void_p, C.c_int32, C.c_double
# every symbol include/igw_goal.h declares: (result, arguments)
SIGNATURES = {
    'igw_goal_version': (C.c_int, []),
    'igw_goal_build_id': (C.c_char_p, []),
    'igw_goal_last_error': (C.c_char_p, []),
    'igw_goal': (C.c_int, [_vp] * 8 + [_i32, _f64, _f64, _i32, _i32] + [_vp] * 9),
}
EXPORTS = list(SIGNATURES)
LIBRARY = _build.Library(LIB, SOURCES, HEADERS, 'igw-goal-build-id:', 'IGW_GOAL_BUILD_ID', deps=[__file__])
source_hash, built_id, is_stale = LIBRARY.source_hash, LIBRARY.built_id, LIBRARY.is_stale


class GoalError(RuntimeError):
    pass


def build(force=False, verbose=False):
    """Builds libigw_goal.so; returns its path."""
    return LIBRARY.build(force, verbose=verbose)


BINDING = _build.Binding(LIBRARY, SIGNATURES, GoalError, 'igw_goal_last_error', 'igw_goal_build_id',
                         'gridworld_amd.goal', 'igw_goal')
load, check, build_id = BINDING.load, BINDING.check, BINDING.build_id


def goal_into(state, n, right_scale, wrong_scale, max_steps, select_and_place, mask, look, outputs, stream):
    """One igw_goal call on raw pointers (ints): `state` the eight state / task-table pointers in the header's order,
    `outputs` the six of OUTPUTS (None = not wanted); mask / look may be None without gain and ends."""
    rc = BINDING.load().igw_goal(*state, int(n), float(right_scale), float(wrong_scale), int(max_steps),
                                 int(bool(select_and_place)), mask, look, *outputs, stream)
    if rc:
        BINDING.check(rc, 'igw_goal')


def _specs(n):
    """name -> (shape, strides, dtype) of the tensor a caller sees, and the alignment igw_goal asks of it."""
    import torch
    grid = ((n, 9, 11, 11), (GRID_STRIDE, 121, 11, 1), torch.int8, 16)
    return {'align': ((n, 3), (4, 1), torch.int8, 4), 'fit': ((n, 4), (4, 1), torch.int16, 8), 'want': grid, 'todo': grid,
            'gain': ((n, ACTIONS), (ACTIONS, 1), torch.float32, 4), 'ends': ((n, ACTIONS), (ACTIONS, 1), torch.uint8, 1)}


def outputs(n, names, dev, stream=None):
    """New tensors for the outputs `names`, as goal() returns them: `align` is an [n, 3] view of four bytes per env,
    `want` / `todo` [n, 9, 11, 11] views of 1104-byte rows (the layout of `grid`)."""
    import torch
    res = {}
    with torch.cuda.stream(stream):
        for k in names:
            shape, strides, dtype, _ = _specs(n)[k]
            base = torch.zeros((n, strides[0]), dtype=dtype, device=dev)
            res[k] = torch.as_strided(base, shape, strides)
    return res


def launch(state, n, reward, mask, look, names, out, dev, stream, alloc_stream=None):
    """One igw_goal launch over n envs; returns the dict name -> tensor of `names` (a subset of OUTPUTS).  `state`:
    the eight state / task-table tensors' rows; `reward` = (right_scale, wrong_scale, max_steps, select_and_place);
    mask / look: the tensors igw_action_mask wrote (None without gain / ends).  `out` (a dict or None) holds tensors
    to write, as an earlier call returned them; what it lacks is allocated.  It touches the device only through
    data_ptr() and the ctypes call."""
    import torch
    out = dict(out or {})
    unknown = [k for k in out if k not in names]
    if unknown:
        raise ValueError(f'out holds {unknown}, the call writes {list(names)}')
    specs = _specs(n)
    for k, t in out.items():
        shape, strides, dtype, al = specs[k]
        if (not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dtype or t.device != dev
                or (n > 0 and tuple(t.stride()) != strides) or t.data_ptr() % al):
            raise ValueError(f'out[{k!r}] must be a {dtype} tensor {shape} with strides {strides} on {dev}, '
                             f'{al}-byte aligned (what goal() returns)')
    out.update(outputs(n, [k for k in names if k not in out], dev, alloc_stream))
    ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    goal_into([t.data_ptr() for t in state], n, *reward, ptr(mask), ptr(look), [ptr(out.get(k)) for k in OUTPUTS], stream)
    return {k: out[k] for k in OUTPUTS if k in names}


def goal_world(want, start):
    """The world colours wanted: `want` (the aligned synthetic target, goal()['want']) + `start` (the starting grid,
    broadcastable to it) where that is a block id 0..6, -1 elsewhere (a synthetic value that no single block gives)."""
    import torch
    w = want.to(torch.int16) + torch.as_tensor(start, device=want.device).to(torch.int16)
    return torch.where((w >= 0) & (w <= 6), w, torch.full_like(w, -1)).to(torch.int8)


if __name__ == '__main__':
    print(build(force='--force' in sys.argv, verbose=True))
