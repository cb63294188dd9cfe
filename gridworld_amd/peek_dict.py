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
import os
import sys

from . import build as _build
from . import peek as _peek

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIB = os.path.join(HERE, 'libigw_peek_dict.so')
SOURCES = [os.path.join(CSRC, 'peek_dict', 'igw_peek_dict.hip')]
HEADERS = [os.path.join(CSRC, f) for f in ('igw_device.h', 'igw_trig.h', 'igw_trig_lut.h', 'igw_trig_tables.h',
                                            'igw_vote.h', os.path.join('peek', 'igw_peek_core.h'),
                                            os.path.join('peek', 'igw_peek_body.h'))] + \
          [os.path.join(HERE, '..', 'include', f) for f in ('igw.h', 'igw_peek.h', 'igw_peek_dict.h')]
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
# every symbol include/igw_peek_dict.h declares: (result, arguments)
SIGNATURES = {
    'igw_peek_dict_version': (C.c_int, []),
    'igw_peek_dict_build_id': (C.c_char_p, []),
    'igw_peek_dict_last_error': (C.c_char_p, []),
    'igw_peek_flying': (C.c_int, [_vp] * 9 + [_i32, _i32, _i32] + [_vp] * 4 + _tail),
    'igw_peek_walking_dict': (C.c_int, [_vp] * 9 + [_i32, _i32, _i32] + [_vp] * 2 + _tail),
}
EXPORTS = list(SIGNATURES)
LIBRARY = _build.Library(LIB, SOURCES, HEADERS, 'igw-peek-dict-build-id:', 'IGW_PEEK_DICT_BUILD_ID', deps=[__file__])
source_hash, built_id, is_stale = LIBRARY.source_hash, LIBRARY.built_id, LIBRARY.is_stale


class PeekDictError(RuntimeError):
    pass


def build(force=False, verbose=False):
    """Builds libigw_peek_dict.so; returns its path."""
    return LIBRARY.build(force, verbose=verbose)


BINDING = _build.Binding(LIBRARY, SIGNATURES, PeekDictError, 'igw_peek_dict_last_error', 'igw_peek_dict_build_id',
                         'gridworld_amd.peek_dict', 'igw_peek_dict')
load, check, build_id = BINDING.load, BINDING.check, BINDING.build_id


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


def check_outputs(names):
    """The outputs asked for, in OUTPUTS' order; ValueError for none or an unknown one."""
    names = tuple(names)
    unknown = [k for k in names if k not in OUTPUTS]
    if unknown or not names:
        raise ValueError(f'peek_dict: outputs names some of {OUTPUTS}, at least one, got {names!r}')
    return tuple(k for k in OUTPUTS if k in names)


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
    out = dict(out or {})
    unknown = [key for key in out if key not in names]
    if unknown:
        raise ValueError(f'out holds {unknown}, the call writes {list(names)}')
    specs = _peek._specs(n, k, h)
    for key, t in out.items():
        shape, dtype = specs[key]
        if (not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dtype or t.device != dev
                or not t.is_contiguous()):
            raise ValueError(f'out[{key!r}] must be a contiguous {dtype} tensor {shape} on {dev} (what peek_dict() '
                             'returns)')
    with torch.cuda.stream(alloc_stream):
        bufs = device_actions(space, actions, dev)
        for key in names:
            if key not in out:
                out[key] = torch.empty(specs[key][0], dtype=specs[key][1], device=dev)
    ptr = lambda key: out[key].data_ptr() if key in names else None  # noqa: E731
    peek_into(space, [t.data_ptr() for t in state], n, k, h, [b.data_ptr() for b in bufs], per_env, *reward, gamma,
              [ptr(key) for key in OUTPUTS], stream)
    return {key: out[key] for key in names}, bufs


if __name__ == '__main__':
    print(build(force='--force' in sys.argv, verbose=True))
