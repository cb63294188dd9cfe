"""State queries of the step path: builds and binds libigw_query.so (include/igw_query.h).

    mask = env.action_mask()                        # uint8 [N, 18]: which Discrete(18) actions would act
    mask, look, actions = env.action_mask(look=True, sample=(seed, t))
    VecGridWorld(..., action_mask=True)             # reset() / step() also return obs['action_mask']

The library is a separate one, as the renderer's are: it reads the step path's state buffers (include/igw.h) and is not
part of the step library's build (its sources and build id are its own, so the step library's profiles stay valid).
There is no CPU fallback: without a HIP device the launch fails and the call raises.
"""
import ctypes as C
import sys

from . import _out
from . import build as _build

VERSION = 1
ACTIONS = 18
# the 18 actions of Discrete(18) (the walking action space with discretize=True), by index
ACTION_NAMES = ('noop', 'forward', 'back', 'left', 'right', 'jump', 'hotbar_1', 'hotbar_2', 'hotbar_3', 'hotbar_4',
                'hotbar_5', 'hotbar_6', 'camera_left', 'camera_right', 'camera_up', 'camera_down', 'break', 'place')
PROBES = (6, 7, 8, 9, 10, 11, 16, 17)   # the actions that can change the grid
OUTPUTS = ('mask', 'look', 'actions')    # in the order igw_action_mask takes them
_vp, _i32, _i64, _u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64


class QueryError(RuntimeError):
    pass


# include/igw_query.h declares igw_action_mask and the three symbols every library has: (result, arguments)
LIBRARY, BINDING = _build.query('query', __file__, {
    'igw_action_mask': (C.c_int, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _u64, _u64, _i64, _vp]),
}, QueryError, 'igw_action_mask')
LIB, SOURCES, HEADERS = LIBRARY.lib, LIBRARY.sources, LIBRARY.headers
SIGNATURES, EXPORTS = BINDING.signatures, list(BINDING.signatures)
build, source_hash, built_id, is_stale = LIBRARY.build, LIBRARY.source_hash, LIBRARY.built_id, LIBRARY.is_stale
load, check, build_id = BINDING.load, BINDING.check, BINDING.build_id


def action_mask_into(agent, occ, n, select_and_place, mask, look, actions, seed, t, env_offset, stream):
    """One igw_action_mask call on raw pointers (ints; look and actions may be None)."""
    rc = BINDING.load().igw_action_mask(agent, occ, int(n), int(bool(select_and_place)), mask, look, actions,
                                        int(seed) & (2 ** 64 - 1), int(t) & (2 ** 64 - 1), int(env_offset), stream)
    if rc:
        BINDING.check(rc, 'igw_action_mask')


def launch(agent, occ, n, select_and_place, out, look, sample, env_offset, dev, stream, alloc_stream=None):
    """One igw_action_mask launch over n envs and what it wrote: the mask uint8 [n, 18], then the look tensor int16
    [n, 2] and / or the sampled actions int32 [n] when asked for (a tuple in that order; the mask alone otherwise).
    `agent` / `occ` are the state tensors' rows; `out` is None or the mask tensor, or with look / sample a tuple of
    the tensors to write in the order they are returned (None entries are allocated); look is a bool; `sample` None or
    (seed, t).  With every output given nothing is allocated, so the call can be captured.  It touches the device only
    through data_ptr() and the ctypes call."""
    import torch
    names = [k for k, w in zip(OUTPUTS, (True, look, sample is not None)) if w]
    given = list(out) if isinstance(out, (tuple, list)) else [out]
    if len(given) > len(names):
        raise ValueError(f'out is {len(given)} tensors, the call writes {len(names)}')
    specs = {'mask': _out.spec((n, ACTIONS), torch.uint8), 'look': _out.spec((n, 2), torch.int16),
             'actions': _out.spec((n,), torch.int32)}
    res, ptrs = _out.outputs('action_mask', OUTPUTS, names, specs, {k: t for k, t in zip(names, given) if t is not None},
                             dev, alloc_stream)
    seed, t = (0, 0) if sample is None else sample
    action_mask_into(agent.data_ptr(), occ.data_ptr(), n, select_and_place, *ptrs, seed, t, env_offset, stream)
    got = tuple(res.values())
    return got[0] if len(got) == 1 else got


if __name__ == '__main__':
    print(build(force='--force' in sys.argv, verbose=True))
