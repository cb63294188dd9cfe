"""State queries of the step path: builds and binds libigw_query.so (include/igw_query.h).

    mask = env.action_mask()                        # uint8 [N, 18]: which Discrete(18) actions would act
    mask, look, actions = env.action_mask(look=True, sample=(seed, t))
    VecGridWorld(..., action_mask=True)             # reset() / step() also return obs['action_mask']

The library is a separate one, as the renderer's are: it reads the step path's state buffers (include/igw.h) and is not
part of the step library's build (its sources and build id are its own, so the step library's profiles stay valid).
There is no CPU fallback: without a HIP device the launch fails and the call raises.
"""
import ctypes as C
import os
import sys

from . import build as _build

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIB = os.path.join(HERE, 'libigw_query.so')
SOURCES = [os.path.join(CSRC, 'query', 'igw_query.hip')]
HEADERS = [os.path.join(CSRC, f) for f in ('igw_device.h', 'igw_trig.h', 'igw_trig_lut.h', 'igw_trig_tables.h')] + \
          [os.path.join(HERE, '..', 'include', 'igw.h'), os.path.join(HERE, '..', 'include', 'igw_query.h')]
VERSION = 1
ACTIONS = 18
# the 18 actions of Discrete(18) (the walking action space with discretize=True), by index
ACTION_NAMES = ('noop', 'forward', 'back', 'left', 'right', 'jump', 'hotbar_1', 'hotbar_2', 'hotbar_3', 'hotbar_4',
                'hotbar_5', 'hotbar_6', 'camera_left', 'camera_right', 'camera_up', 'camera_down', 'break', 'place')
PROBES = (6, 7, 8, 9, 10, 11, 16, 17)   # the actions that can change the grid
_vp, _i32, _i64, _u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
# every symbol include/igw_query.h declares: (result, arguments)
SIGNATURES = {
    'igw_query_version': (C.c_int, []),
    'igw_query_build_id': (C.c_char_p, []),
    'igw_query_last_error': (C.c_char_p, []),
    'igw_action_mask': (C.c_int, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _u64, _u64, _i64, _vp]),
}
EXPORTS = list(SIGNATURES)
LIBRARY = _build.Library(LIB, SOURCES, HEADERS, 'igw-query-build-id:', 'IGW_QUERY_BUILD_ID', deps=[__file__])
source_hash, built_id, is_stale = LIBRARY.source_hash, LIBRARY.built_id, LIBRARY.is_stale


class QueryError(RuntimeError):
    pass


def build(force=False, verbose=False):
    """Builds libigw_query.so; returns its path."""
    return LIBRARY.build(force, verbose=verbose)


BINDING = _build.Binding(LIBRARY, SIGNATURES, QueryError, 'igw_query_last_error', 'igw_query_build_id',
                         'gridworld_amd.query', 'igw_action_mask')
load, check, build_id = BINDING.load, BINDING.check, BINDING.build_id


def action_mask_into(agent, occ, n, select_and_place, mask, look, actions, seed, t, env_offset, stream):
    """One igw_action_mask call on raw pointers (ints; look and actions may be None)."""
    rc = BINDING.load().igw_action_mask(agent, occ, int(n), int(bool(select_and_place)), mask, look, actions,
                                        int(seed) & (2 ** 64 - 1), int(t) & (2 ** 64 - 1), int(env_offset), stream)
    if rc:
        BINDING.check(rc, 'igw_action_mask')


def _tensor(shape, dtype, given, dev, stream, name):
    """One output of a launch: allocated (on `stream`, when one is given) or `given`, validated."""
    import torch
    if given is None:
        with torch.cuda.stream(stream):
            return torch.empty(shape, dtype=dtype, device=dev)
    if (not torch.is_tensor(given) or tuple(given.shape) != shape or given.dtype != dtype or not given.is_contiguous()
            or given.device != dev):
        raise ValueError(f'{name} must be a contiguous {dtype} tensor {shape} on {dev}')
    return given


def launch(agent, occ, n, select_and_place, out, look, sample, env_offset, dev, stream, alloc_stream=None):
    """One igw_action_mask launch over n envs and what it wrote: the mask uint8 [n, 18], then the look tensor int16
    [n, 2] and / or the sampled actions int32 [n] when asked for (a tuple in that order; the mask alone otherwise).
    `agent` / `occ` are the state tensors' rows; `out` is None or the mask tensor, or with look / sample a tuple of
    the tensors to write in the order they are returned (None entries are allocated); look is a bool; `sample` None or
    (seed, t).  With every output given nothing is allocated, so the call can be captured.  It touches the device only
    through data_ptr() and the ctypes call."""
    import torch
    want = [True, bool(look), sample is not None]
    given = list(out) if isinstance(out, (tuple, list)) else [out]
    if len(given) > sum(want):
        raise ValueError(f'out holds {len(given)} tensors, the call writes {sum(want)}')
    given += [None] * (sum(want) - len(given))
    spec = (((n, ACTIONS), torch.uint8, 'the mask'), ((n, 2), torch.int16, 'look'), ((n,), torch.int32, 'actions'))
    res, it = [], iter(given)
    for w, (shape, dtype, name) in zip(want, spec):
        res.append(_tensor(shape, dtype, next(it), dev, alloc_stream, name) if w else None)
    seed, t = (0, 0) if sample is None else sample
    ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    action_mask_into(agent.data_ptr(), occ.data_ptr(), n, select_and_place, res[0].data_ptr(), ptr(res[1]), ptr(res[2]),
                     seed, t, env_offset, stream)
    got = tuple(r for r in res if r is not None)
    return got[0] if len(got) == 1 else got


if __name__ == '__main__':
    print(build(force='--force' in sys.argv, verbose=True))
