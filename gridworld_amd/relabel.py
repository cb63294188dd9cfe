"""The relabel query of the episode log: builds and binds libigw_relabel.so (include/igw_relabel.h).

    r = env.relabel('final')                        # hindsight: the target was what the episode ended up building
    r = env.relabel(G.relabel_future(r['length'], 4, seed=0))     # HER's "future" strategy, four goals per episode
    r = G.relabel(records, first, length, starts, at=at)          # the stateless form, on any record buffer
    r['reward'] [E, G, L], r['done'], r['end'] [E, G], r['ret'], r['target'] [E, G, 9, 11, 11]

The library is a separate one, as the renderer's, the codec's and the other queries' are: it reads trajectory records
(include/igw.h: igw_set_trajectory_log), starting grids and candidate targets, no env state, and is not part of the step
library's build (its sources and build id are its own, so the step library's profiles stay valid).  There is no CPU
fallback: without a HIP device the launch fails and the call raises.
"""
import ctypes as C
import functools
import sys

from . import _out
from . import build as _build
from ._out import _is

VERSION = 1
ROW = 1104          # bytes of a grid row
CELLS = 1089
RECORD = 64         # bytes of a trajectory record
MAX_G = 256
OUTPUTS = ('reward', 'done', 'progress', 'end', 'ret', 'target_size', 'target')   # in the order igw_relabel takes them
DEFAULT = ('reward', 'done', 'end', 'ret')
_vp, _i32, _i64, _f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double


class RelabelError(RuntimeError):
    pass


# include/igw_relabel.h declares igw_relabel and the three symbols every library has: (result, arguments)
LIBRARY, BINDING = _build.query('relabel', __file__, {
    'igw_relabel': (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _f64, _f64, _i32, _f64] + [_vp] * 8),
}, RelabelError, 'igw_relabel', headers=['igw_vote.h'])
LIB, SOURCES, HEADERS = LIBRARY.lib, LIBRARY.sources, LIBRARY.headers
SIGNATURES, EXPORTS = BINDING.signatures, list(BINDING.signatures)
build, source_hash, built_id, is_stale = LIBRARY.build, LIBRARY.source_hash, LIBRARY.built_id, LIBRARY.is_stale
load, check, build_id = BINDING.load, BINDING.check, BINDING.build_id
check_outputs = functools.partial(_out.check_outputs, 'relabel', OUTPUTS)
grid_rows = functools.partial(_out.grid_rows, 'relabel: grids')


def relabel_into(records, n_records, first, length, starts, targets, at, e, g, l, right_scale, wrong_scale, max_steps,
                 gamma, outputs, stream):
    """One igw_relabel call on raw pointers (ints; targets or at is None): `outputs` the seven of OUTPUTS (None = not
    wanted)."""
    rc = BINDING.load().igw_relabel(records, int(n_records), first, length, starts, targets, at, int(e), int(g), int(l),
                                    float(right_scale), float(wrong_scale), int(max_steps), float(gamma), *outputs, stream)
    if rc:
        BINDING.check(rc, 'igw_relabel')


def _specs(e, g, l):
    """name -> _out.spec of the tensor a caller sees: `target` is an [E, G, 9, 11, 11] view of 1104-byte rows (each in
    the layout of `grid`), 16-byte aligned."""
    import torch
    step = lambda dtype: _out.spec((e, g, l), dtype, (g * l, l, 1))  # noqa: E731
    pair = lambda dtype: _out.spec((e, g), dtype, (g, 1))  # noqa: E731
    return {'reward': step(torch.float32), 'done': step(torch.uint8), 'progress': step(torch.int16),
            'end': pair(torch.int32), 'ret': pair(torch.float32), 'target_size': pair(torch.int16),
            'target': _out.spec((e, g, 9, 11, 11), torch.int8, (g * ROW, ROW, 121, 11, 1), 16, (e, g * ROW))}


def outputs(e, g, l, names, dev, stream=None):
    """New tensors for the outputs `names`, as relabel() returns them."""
    return _out.outputs('relabel', OUTPUTS, names, _specs(e, g, l), None, dev, stream)[0]


def launch(records, first, length, starts, targets, at, pad, reward, gamma, names, out, dev, stream, alloc_stream=None):
    """One igw_relabel launch; returns the dict name -> tensor of `names` (a subset of OUTPUTS).  Every input is a
    contiguous device tensor of the header's dtype: records uint8 [..., 64], first int64 [E], length int32 [E], starts
    int8 [E, 1104], and targets int8 [E, G, 1104] or at int32 [E, G] (the other None); `pad` is L; `reward` = (right_scale,
    wrong_scale, max_steps).  `out` (a dict or None) holds tensors to write, as an earlier call returned them; what it
    lacks is allocated.  It touches the device only through data_ptr() and the ctypes call."""
    import math
    import torch
    names = check_outputs(names)
    e = int(first.shape[0])
    if not (torch.is_tensor(records) and records.dtype == torch.uint8 and records.device == dev and records.is_contiguous()
            and records.dim() >= 1 and records.shape[-1] == RECORD):
        raise ValueError(f'relabel: records must be a contiguous uint8 tensor [..., {RECORD}] on {dev}')
    if not _is(first, torch.int64, (e,), dev) or not _is(length, torch.int32, (e,), dev):
        raise ValueError(f'relabel: first must be an int64 and length an int32 tensor [{e}] on {dev}')
    if not _is(starts, torch.int8, (e, ROW), dev):
        raise ValueError(f'relabel: starts must be an int8 tensor [{e}, {ROW}] on {dev}')
    if (targets is None) == (at is None):
        raise ValueError('relabel: give exactly one of targets and at')
    goals = targets if at is None else at
    if not torch.is_tensor(goals) or goals.dim() < 2 or goals.shape[0] != e:
        raise ValueError(f'relabel: the goals must be a tensor [{e}, G, ...]')
    g = int(goals.shape[1])
    if not 1 <= g <= MAX_G:
        raise ValueError(f'relabel: G must be 1..{MAX_G}, got {g}')
    if at is None and not _is(targets, torch.int8, (e, g, ROW), dev):
        raise ValueError(f'relabel: targets must be an int8 tensor [{e}, {g}, {ROW}] on {dev}')
    if at is not None and not _is(at, torch.int32, (e, g), dev):
        raise ValueError(f'relabel: at must be an int32 tensor [{e}, {g}] on {dev}')
    l = int(pad)
    if l < 1 or e * g * l >= 1 << 40:
        raise ValueError(f'relabel: pad must be >= 1 and E * G * pad below 2^40, got {pad}')
    right, wrong, max_steps = reward
    if not 1 <= int(max_steps) <= 65534:
        raise ValueError(f'relabel: max_steps must be 1..65534, got {max_steps}')
    if not math.isfinite(float(gamma)):
        raise ValueError(f'relabel: gamma must be finite, got {gamma}')
    res, ptrs = _out.outputs('relabel', OUTPUTS, names, _specs(e, g, l), out, dev, alloc_stream)
    if e:   # (the tensors of no episode have no address to pass)
        relabel_into(records.data_ptr(), records.numel() // RECORD, first.data_ptr(), length.data_ptr(), starts.data_ptr(),
                     _out.ptr(targets), _out.ptr(at), e, g, l, right, wrong, max_steps, gamma, ptrs, stream)
    return res


def relabel(records, first, length, starts, targets=None, at=None, *, right_scale=1, wrong_scale=0.1, max_steps=250,
            gamma=1.0, outputs=DEFAULT, out=None, pad=None):
    """Rewards of logged episodes under other targets, the stateless device form: one igw_relabel
    launch on the current stream of the records' device.
      records  uint8 device tensor [..., 64]: trajectory records (what enable_trajectory_log returns, or any buffer of
               that layout; only the `change` word of a record is read)
      first    [E] index of each episode's first record; length [E] its steps; starts [E, 9, 11, 11] (or [E, 1089] /
               [E, 1104]) the grid it started from
      targets  [E, G, 9, 11, 11] (or [E, G, 1089] / [E, G, 1104]) user targets, or
      at       [E, G] integers: goal g is the episode's own grid at that entry (0 = the start, length = the final grid)
    Returns a dict of the `outputs` named: reward float32 / done uint8 / progress int16 [E, G, L] (+0 past an episode's
    length), end int32 [E, G] (the first done step, 0 for none), ret float32 [E, G] (discounted by `gamma` up to `end`),
    target_size int16 [E, G], target int8 [E, G, 9, 11, 11] (the goal grids used).  L is `pad`; by default the log's
    capacity (records.shape[-2]) when records has that dimension, else max(length), which waits for the device.
    Inputs that already are contiguous device tensors of the library's dtypes are passed as they are; `out` holds
    tensors to write, as an earlier call returned them."""
    import torch
    if not torch.is_tensor(records) or not records.is_cuda:
        raise ValueError('relabel: records must be a device tensor')
    dev = records.device
    conv = lambda x, dt: (x if torch.is_tensor(x) else torch.as_tensor(x)).to(device=dev, dtype=dt).contiguous()  # noqa: E731
    first, length = conv(first, torch.int64).reshape(-1), conv(length, torch.int32).reshape(-1)
    e = first.shape[0]
    starts = grid_rows(starts, dev, (e,))
    if targets is not None and at is None:
        if not hasattr(targets, 'shape') or len(targets.shape) < 3:
            raise ValueError('relabel: targets must be [E, G, 9, 11, 11], [E, G, 1089] or [E, G, 1104]')
        targets = grid_rows(targets, dev, (e, int(targets.shape[1])))
    elif at is not None and targets is None:
        at = conv(at, torch.int32)
    else:
        raise ValueError('relabel: give exactly one of targets and at')
    if pad is None:
        pad = records.shape[-2] if records.dim() >= 3 else max(int(length.max()) if e else 1, 1)
    stream = torch.cuda.current_stream(dev).cuda_stream
    return launch(records.contiguous(), first, length, starts, targets, at, pad, (right_scale, wrong_scale, max_steps),
                  gamma, check_outputs(outputs), out, dev, stream)


def relabel_future(length, k, seed=0):
    """HER's "future" strategy per episode: an int32 tensor [E, k] of entries drawn uniformly from 1..length[e] (0 where
    length[e] is 0) with a torch generator seeded by `seed` on length's device; pass it to relabel() as `at` / `goals`.
    The kernel itself stays deterministic."""
    import torch
    length = torch.as_tensor(length)
    if length.dim() != 1 or length.is_floating_point() or int(k) < 1:
        raise ValueError('relabel_future: length must be an integer tensor [E] and k >= 1')
    gen = torch.Generator(device=length.device)
    gen.manual_seed(int(seed))
    u = torch.rand((length.shape[0], int(k)), generator=gen, device=length.device, dtype=torch.float64)
    n = length.to(torch.float64).clamp(min=0)[:, None]
    return torch.minimum((u * n).floor() + 1, n).to(torch.int32)


class _Callable(type(sys)):
    """The module as the package's attribute of the same name: G.relabel(...) is the function, G.relabel.build() and the
    rest of the module stay reachable."""

    def __call__(self, *args, **kw):
        return relabel(*args, **kw)


sys.modules[__name__].__class__ = _Callable

if __name__ == '__main__':
    print(build(force='--force' in sys.argv, verbose=True))
