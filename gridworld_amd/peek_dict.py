"""The peek query for the flying and the walking Dict action spaces: builds and binds libigw_peek_dict.so
(include/igw_peek_dict.h).

    p = env.peek_dict(dict(movement=mv, camera=cam, inventory=inv, placement=pl))   # flying: [K, H, ...] or [N, K, H, ...]
    p = env.peek_dict(dict(buttons=b, camera=cam), gamma=0.97, outputs=('ret', 'ends'))   # walking, discretize=False
    p['reward'] float32 [N, K, H]   p['ends'] int16 [N, K]   p['change'] int16 [N, K, H]
    p['pose'] float32 [N, K, 5]     p['ret'] float32 [N, K]          # peek's dict: peek_decode / peek_best work on it

The library is a separate one beside libigw_peek.so (the Discrete(18) space): it reads the step path's state buffers
(include/igw.h) and is part of no other library's build (its sources and build id are its own, so the step library's and
the peek library's stay valid).  There is no CPU fallback: without a HIP device the launch fails and the call raises.
"""
import ctypes as C
import functools
import sys

from . import _out
from . import build as _build
from . import peek as _peek

CSRC = _build.CSRC
VERSION = 1
MAX_H = _peek.MAX_H
MAX_K = _peek.MAX_K
OUTPUTS = _peek.OUTPUTS   # in the order the entries take them
# the action arguments of each space in the order its entry takes them: (key, dtype name, shape behind [.., K, H])
SPACES = {
    'flying': ('igw_peek_flying', (('movement', 'float32', (3,)), ('camera', 'float32', (2,)),
                                   ('inventory', 'int32', ()), ('placement', 'int32', ()))),
    'walking_dict': ('igw_peek_walking_dict', (('buttons', 'uint8', (8,)), ('camera', 'float32', (2,)))),
}
_vp, _i32, _f64 = C.c_void_p, C.c_int32, C.c_double
_tail = [_i32, _f64, _f64, _i32, _i32, _f64] + [_vp] * 6   # per_env .. gamma, the five outputs, the stream


class PeekDictError(RuntimeError):
    pass


# include/igw_peek_dict.h declares the two entries and the three symbols every library has: (result, arguments)
LIBRARY, BINDING = _build.query('peek_dict', __file__, {
    'igw_peek_flying': (C.c_int, [_vp] * 9 + [_i32, _i32, _i32] + [_vp] * 4 + _tail),
    'igw_peek_walking_dict': (C.c_int, [_vp] * 9 + [_i32, _i32, _i32] + [_vp] * 2 + _tail),
}, PeekDictError, 'igw_peek_dict', headers=_peek.SHARED_HEADERS, include=['igw_peek.h'])
LIB, SOURCES, HEADERS = LIBRARY.lib, LIBRARY.sources, LIBRARY.headers
SIGNATURES, EXPORTS = BINDING.signatures, list(BINDING.signatures)
build, source_hash, built_id, is_stale = LIBRARY.build, LIBRARY.source_hash, LIBRARY.built_id, LIBRARY.is_stale
load, check, build_id = BINDING.load, BINDING.check, BINDING.build_id
check_outputs = functools.partial(_out.check_outputs, 'peek_dict', OUTPUTS, string=False)


def peek_into(space, state, n, k, h, actions, per_env, right_scale, wrong_scale, max_steps, select_and_place, gamma,
              outputs, stream):
    """One igw_peek_flying / igw_peek_walking_dict call on raw pointers (ints): `space` a key of SPACES, `state` the
    nine state / task-table pointers in the header's order, `actions` the space's action pointers in its entry's order,
    `outputs` the five of OUTPUTS (None = not wanted)."""
    entry = SPACES[space][0]
    rc = getattr(BINDING.load(), entry)(*state, int(n), int(k), int(h), *actions, int(bool(per_env)), float(right_scale),
                                        float(wrong_scale), int(max_steps), int(bool(select_and_place)), float(gamma),
                                        *outputs, stream)
    if rc:
        BINDING.check(rc, entry)


def shape_of(space, actions, n):
    """(K, H, per_env) of an action dict (tensors, arrays or nested lists) of the space for a range of n envs; ValueError for
    missing or extra keys, a ragged list, a wrong rank or trailing shape, leading shapes that differ, a first dimension that is not n,
    or K / H out of range."""
    import numpy as np
    fields = SPACES[space][1]
    keys = [key for key, _, _ in fields]
    if not isinstance(actions, dict) or sorted(actions) != sorted(keys):
        got = sorted(actions) if isinstance(actions, dict) else type(actions).__name__
        raise ValueError(f'peek_dict: the {space} action space takes a dict with the keys {keys}, got {got}')
    lead = None
    for key, _, tail in fields:
        x = actions[key]
        shape = tuple(x.shape) if hasattr(x, 'shape') else np.shape(x)   # (a ragged list: numpy's ValueError)
        cut = len(shape) - len(tail)
        if cut not in (2, 3) or shape[cut:] != tail:
            dims = ', '.join(map(str, tail))
            raise ValueError(f'peek_dict: {key} must be [K, H{", " + dims if dims else ""}] or '
                             f'[N, K, H{", " + dims if dims else ""}], got shape {shape}')
        if lead is None:
            lead = shape[:cut]
        elif shape[:cut] != lead:
            raise ValueError(f'peek_dict: every entry must have the same leading shape, got {lead} for {keys[0]} and '
                             f'{shape[:cut]} for {key}')
    if len(lead) == 3 and lead[0] != n:
        raise ValueError(f'peek_dict: actions {lead} are per env, so their first dimension must be the {n} envs')
    k, h = lead[-2:]
    if not 1 <= k <= MAX_K:
        raise ValueError(f'peek_dict: K must be 1..{MAX_K}, got {k}')
    if not 1 <= h <= MAX_H:
        raise ValueError(f'peek_dict: H must be 1..{MAX_H}, got {h}')
    return k, h, len(lead) == 3


def device_actions(space, actions, dev):
    """The space's action entries as contiguous device tensors of the ABI dtypes, in the entry's order: an entry that
    already is one is passed on as it is, anything else (arrays, lists, other dtypes or devices, strided views) is
    converted -- which allocates."""
    import numpy as np
    import torch
    bufs = []
    for key, dtype, _ in SPACES[space][1]:
        x, dt = actions[key], getattr(torch, dtype)
        if not (type(x) is torch.Tensor and x.dtype is dt and x.device == dev and x.is_contiguous()):
            if not torch.is_tensor(x):
                x = np.asarray(x)
                x = torch.from_numpy(x if x.flags.writeable else x.copy())
            if key in ('buttons', 'inventory', 'placement') and not (x.is_floating_point() or x.dtype in (dt, torch.bool)):
                # an integer too wide for an id field or a button byte stays what it is to the parser -- an invalid id, a
                # pressed button -- instead of wrapping into the valid range (movement and camera are plain casts)
                if key == 'buttons':
                    x = torch.cat([x[..., :7].ne(0).to(torch.int64), x[..., 7:].to(torch.int64).clamp(-1, 255) & 255], -1)
                else:
                    x = torch.where((x < 0) | (x > 6), torch.full_like(x, -1), x)
            x = x.to(device=dev, dtype=dt).contiguous()
        bufs.append(x)
    return bufs


def launch(space, state, n, actions, reward, gamma, names, out, dev, stream, alloc_stream=None):
    """One launch over n envs; returns the dict name -> tensor of `names` (a subset of OUTPUTS).  `space`: a key of
    SPACES; `state`: the nine state / task-table tensors' rows; `actions`: the dict of the space's entries (shape_of's
    rules), converted by device_actions; `reward` = (right_scale, wrong_scale, max_steps, select_and_place).  `out` (a
    dict or None) holds tensors to write, as an earlier call returned them; what it lacks is allocated, so with every
    output given and the actions already device tensors of the ABI dtypes nothing is.  Returns (result, action
    buffers): the launch reads the buffers asynchronously, so the caller keeps them."""
    import torch
    names = check_outputs(names)
    k, h, per_env = shape_of(space, actions, n)
    res, ptrs = _out.outputs('peek_dict', OUTPUTS, names, _peek._specs(n, k, h), out, dev, alloc_stream)
    with torch.cuda.stream(alloc_stream):
        bufs = device_actions(space, actions, dev)
    peek_into(space, [t.data_ptr() for t in state], n, k, h, [b.data_ptr() for b in bufs], per_env, *reward, gamma, ptrs,
              stream)
    return res, bufs


if __name__ == '__main__':
    print(build(force='--force' in sys.argv, verbose=True))
