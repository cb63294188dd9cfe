"""The worth query of the step path: builds and binds libigw_worth.so (include/igw_worth.h).

    w = env.worth()                                 # word int16 [N, 7, 9, 11, 11], best int32 [N, 4]
    w = env.worth(outputs=('best',), allow=allow, stocked=True)   # the best-paid edit the agent can make
    d = worth_decode(w['word'])                     # right, wrong, ends, valid, gain (NaN where invalid)
    worth_plane_names                               # ('break', 'place1', ..., 'place6')

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
PLANES = 7
ROW = 1104          # int16 words per env and plane
CELLS = 1089
OUTPUTS = ('word', 'best')   # in the order igw_worth takes them
worth_plane_names = ('break',) + tuple(f'place{k}' for k in range(1, 7))
_vp, _i32, _f64 = C.c_void_p, C.c_int32, C.c_double


class WorthError(RuntimeError):
    pass


# include/igw_worth.h declares igw_worth and the three symbols every library has: (result, arguments)
LIBRARY, BINDING = _build.query('worth', __file__, {
    'igw_worth': (C.c_int, [_vp] * 8 + [_i32, _i32, _vp, _i32, _f64, _f64, _vp, _vp, _vp]),
}, WorthError, 'igw_worth', headers=['igw_vote.h'])
LIB, SOURCES, HEADERS = LIBRARY.lib, LIBRARY.sources, LIBRARY.headers
SIGNATURES, EXPORTS = BINDING.signatures, list(BINDING.signatures)
build, source_hash, built_id, is_stale = LIBRARY.build, LIBRARY.source_hash, LIBRARY.built_id, LIBRARY.is_stale
load, check, build_id = BINDING.load, BINDING.check, BINDING.build_id
check_outputs = functools.partial(_out.check_outputs, 'worth', OUTPUTS)


def worth_into(state, n, max_steps, allow, stocked, right_scale, wrong_scale, word, best, stream):
    """One igw_worth call on raw pointers (ints): `state` the eight state / task-table pointers in the header's order;
    allow, word or best may be None."""
    rc = BINDING.load().igw_worth(*state, int(n), int(max_steps), allow, int(bool(stocked)), float(right_scale),
                                  float(wrong_scale), word, best, stream)
    if rc:
        BINDING.check(rc, 'igw_worth')


def _specs(n):
    """name -> _out.spec of the tensor a caller sees: `word` is an [n, 7, 9, 11, 11] view of seven 1104-word rows per env
    (each in the layout of `grid`); both are 16-byte aligned."""
    import torch
    return {'word': _out.spec((n, PLANES, 9, 11, 11), torch.int16, (PLANES * ROW, ROW, 121, 11, 1), 16, (n, PLANES * ROW)),
            'best': _out.spec((n, 4), torch.int32, (4, 1), 16)}


def launch(state, n, reward, allow, stocked, names, out, dev, stream, alloc_stream=None):
    """One igw_worth launch over n envs; returns the dict name -> tensor of `names` (a subset of OUTPUTS).  `state`:
    the eight state / task-table tensors' rows; `reward` = (right_scale, wrong_scale, max_steps); `allow`: a uint8
    tensor [n, 2, 9, 11, 11] with 1104-byte rows or contiguous [n, 2, 1104], or None.  `out` (a dict or None) holds
    tensors to write, as an earlier call returned them; what it lacks is allocated.  It touches the device only
    through data_ptr() and the ctypes call."""
    import torch
    if allow is not None:
        ok = torch.is_tensor(allow) and allow.dtype == torch.uint8 and allow.device == dev and allow.data_ptr() % 16 == 0
        if ok and tuple(allow.shape) == (n, 2, 9, 11, 11):
            ok = n == 0 or tuple(allow.stride()) == (2 * ROW, ROW, 121, 11, 1)
        elif ok:
            ok = tuple(allow.shape) == (n, 2, ROW) and allow.is_contiguous()
        if not ok:
            raise ValueError(f'allow must be a uint8 tensor on {dev}: [{n}, 2, 9, 11, 11] with 1104-byte rows (strides '
                             f'{(2 * ROW, ROW, 121, 11, 1)}) or contiguous [{n}, 2, {ROW}], 16-byte aligned')
    res, ptrs = _out.outputs('worth', OUTPUTS, names, _specs(n), out, dev, alloc_stream)
    right, wrong, max_steps = reward
    worth_into([t.data_ptr() for t in state], n, max_steps, _out.ptr(allow), stocked, right, wrong, *ptrs, stream)
    return res


def allow_from_aim(aim, out=None):
    """The `allow` gate of worth() from the planes of aim(): uint8 [N, 2, 9, 11, 11] with 1104-byte rows, plane 0 =
    aim['break'] >= 0, plane 1 = aim['place'] >= 0.  Plain torch on the planes' device."""
    import torch
    n, dev = aim['break'].shape[0], aim['break'].device
    if out is None:
        out = torch.as_strided(torch.zeros((n, 2 * ROW), dtype=torch.uint8, device=dev), (n, 2, 9, 11, 11),
                               (2 * ROW, ROW, 121, 11, 1))
    out[:, 0] = aim['break'] >= 0
    out[:, 1] = aim['place'] >= 0
    return out


def worth_decode(word, right_scale=1, wrong_scale=0.1):
    """The fields of worth()'s words, as a dict of tensors (or numpy arrays, for a numpy `word`) of the words' shape:
    right int16, wrong int8 (-1, 0, 1), ends bool, valid bool (the word is not -1), and gain float32: the reward the
    step would return, right != 0 ? right * right_scale : wrong * wrong_scale, formed in binary64 as the step forms
    it and rounded once; NaN where the edit is invalid (where right, wrong are 0 and ends False)."""
    import numpy as np
    import torch
    as_numpy = not torch.is_tensor(word)
    w = torch.as_tensor(np.asarray(word) if as_numpy else word).to(torch.int32)
    valid = w >= 0
    right = torch.where(valid, ((w & 0xfff) ^ 0x800) - 0x800, torch.zeros_like(w))
    wrong = torch.where(valid, ((w >> 12) & 3) - 1, torch.zeros_like(w))
    ends = valid & (((w >> 14) & 1) != 0)
    r64, w64 = right.to(torch.float64), wrong.to(torch.float64)
    gain = torch.where(right != 0, r64 * float(right_scale), w64 * float(wrong_scale)).to(torch.float32)
    gain = torch.where(valid, gain, torch.full_like(gain, float('nan')))
    res = dict(right=right.to(torch.int16), wrong=wrong.to(torch.int8), ends=ends, valid=valid, gain=gain)
    return {k: v.cpu().numpy() for k, v in res.items()} if as_numpy else res


def worth_encode(right, wrong, ends):
    """The word of (right, wrong, ends): integers / arrays -> numpy int16 (the inverse of worth_decode on valid words)."""
    import numpy as np
    w = (np.asarray(right).astype(np.int32) & 0xfff) | (np.asarray(wrong).astype(np.int32) + 1) << 12 | \
        np.asarray(ends).astype(np.int32) << 14
    return w.astype(np.int16)


if __name__ == '__main__':
    print(build(force='--force' in sys.argv, verbose=True))
