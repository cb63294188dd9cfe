"""The peek query of the step path: builds and binds libigw_peek.so (include/igw_peek.h).

    p = env.peek(actions)                           # actions int [K, H] (shared) or [N, K, H]
    p['reward'] float32 [N, K, H]   p['ends'] int16 [N, K]   p['change'] int16 [N, K, H]
    p['pose'] float32 [N, K, 5]     p['ret'] float32 [N, K]
    p = env.peek(actions, gamma=0.97, outputs=('ret', 'ends'))
    cell, colour = peek_decode(p['change'])         # -1 / -1 where a step changed nothing
    k = peek_best(p['ret'])                         # the lowest k of the best return per env

The library is a separate one, as the renderer's, the codec's, the query's, the goal's and the aim's are: it reads the
step path's state buffers (include/igw.h) and is not part of the step library's build (its sources and build id are its
own, so the step library's profiles stay valid).  There is no CPU fallback: without a HIP device the launch fails and
the call raises.
"""
import ctypes as C
import functools
import sys

from . import _out
from . import build as _build

VERSION = 1
ACTIONS = 18
MAX_H = 32
MAX_K = 4096
OUTPUTS = ('reward', 'ends', 'change', 'pose', 'ret')   # in the order igw_peek takes them
NONE = -1
SHARED_HEADERS = ['igw_vote.h', 'peek/igw_peek_core.h', 'peek/igw_peek_body.h']   # the kernel, as peek_dict builds it too
_vp, _i32, _f64 = C.c_void_p, C.c_int32, C.c_double


class PeekError(RuntimeError):
    pass


# include/igw_peek.h declares igw_peek and the three symbols every library has: (result, arguments)
LIBRARY, BINDING = _build.query('peek', __file__, {
    'igw_peek': (C.c_int, [_vp] * 9 + [_i32, _i32, _i32, _vp, _i32, _f64, _f64, _i32, _i32, _f64] + [_vp] * 6),
}, PeekError, 'igw_peek', headers=SHARED_HEADERS)
LIB, SOURCES, HEADERS = LIBRARY.lib, LIBRARY.sources, LIBRARY.headers
SIGNATURES, EXPORTS = BINDING.signatures, list(BINDING.signatures)
build, source_hash, built_id, is_stale = LIBRARY.build, LIBRARY.source_hash, LIBRARY.built_id, LIBRARY.is_stale
load, check, build_id = BINDING.load, BINDING.check, BINDING.build_id
check_outputs = functools.partial(_out.check_outputs, 'peek', OUTPUTS, string=False)


def peek_into(state, n, k, h, actions, per_env, right_scale, wrong_scale, max_steps, select_and_place, gamma, outputs,
              stream):
    """One igw_peek call on raw pointers (ints): `state` the nine state / task-table pointers in the header's order,
    `outputs` the five of OUTPUTS (None = not wanted)."""
    rc = BINDING.load().igw_peek(*state, int(n), int(k), int(h), actions, int(bool(per_env)), float(right_scale),
                                 float(wrong_scale), int(max_steps), int(bool(select_and_place)), float(gamma), *outputs,
                                 stream)
    if rc:
        BINDING.check(rc, 'igw_peek')


def shape_of(actions, n):
    """(K, H, per_env) of an action tensor or array for a range of n envs; ValueError for a wrong rank, a first
    dimension that is not n, or K / H out of range."""
    shape = tuple(actions.shape)
    if len(shape) not in (2, 3):
        raise ValueError(f'peek: actions must be [K, H] or [N, K, H], got shape {shape}')
    if len(shape) == 3 and shape[0] != n:
        raise ValueError(f'peek: actions {shape} are per env, so their first dimension must be the {n} envs')
    k, h = shape[-2:]
    if not 1 <= k <= MAX_K:
        raise ValueError(f'peek: K must be 1..{MAX_K}, got {k}')
    if not 1 <= h <= MAX_H:
        raise ValueError(f'peek: H must be 1..{MAX_H}, got {h}')
    return k, h, len(shape) == 3


def _specs(n, k, h):
    """name -> _out.spec of the contiguous tensor a caller sees."""
    import torch
    return {'reward': _out.spec((n, k, h), torch.float32), 'ends': _out.spec((n, k), torch.int16),
            'change': _out.spec((n, k, h), torch.int16), 'pose': _out.spec((n, k, 5), torch.float32),
            'ret': _out.spec((n, k), torch.float32)}


def launch(state, n, actions, reward, gamma, names, out, dev, stream, alloc_stream=None):
    """One igw_peek launch over n envs; returns the dict name -> tensor of `names` (a subset of OUTPUTS).  `state`: the
    nine state / task-table tensors' rows; `actions`: a contiguous int32 device tensor [K, H] or [n, K, H]; `reward` =
    (right_scale, wrong_scale, max_steps, select_and_place).  `out` (a dict or None) holds tensors to write, as an
    earlier call returned them; what it lacks is allocated, so with every output given nothing is.  It touches the
    device only through data_ptr() and the ctypes call."""
    names = check_outputs(names)
    k, h, per_env = shape_of(actions, n)
    res, ptrs = _out.outputs('peek', OUTPUTS, names, _specs(n, k, h), out, dev, alloc_stream)
    peek_into([t.data_ptr() for t in state], n, k, h, actions.data_ptr(), per_env, *reward, gamma, ptrs, stream)
    return res


def peek_decode(change):
    """(cell, colour) of the codes of peek()['change'], int32 tensors of the codes' shape: the flat grid cell 0..1088 a
    step changed and the block id now in it (0: a break); -1 and -1 where the step changed nothing."""
    import torch
    code = torch.as_tensor(change).to(torch.int32)
    none = code < 0
    minus = torch.full_like(code, NONE)
    return torch.where(none, minus, code & 0x7ff), torch.where(none, minus, code >> 11)


def peek_best(ret):
    """The lowest k of the largest return per env: int64 [N] from peek()['ret'] [N, K].  A NaN return (a |gamma| so
    large that g_h overflows: inf * 0.0) ranks below every number, so a row of nothing but NaN answers 0.  Plain
    torch."""
    import torch
    ret = torch.as_tensor(ret)
    ret = torch.where(torch.isnan(ret), torch.full_like(ret, float('-inf')), ret)
    best = ret.max(dim=1, keepdim=True).values
    k = torch.arange(ret.shape[1], device=ret.device).expand_as(ret)
    return torch.where(ret == best, k, torch.full_like(k, ret.shape[1] - 1)).min(dim=1).values


if __name__ == '__main__':
    print(build(force='--force' in sys.argv, verbose=True))
