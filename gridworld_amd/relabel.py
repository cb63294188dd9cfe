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
import os
import sys

from . import build as _build

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIB = os.path.join(HERE, 'libigw_relabel.so')
SOURCES = [os.path.join(CSRC, 'relabel', 'igw_relabel.hip')]
HEADERS = [os.path.join(CSRC, f) for f in ('igw_device.h', 'igw_trig.h', 'igw_trig_lut.h', 'igw_trig_tables.h',
                                            'igw_vote.h')] + \
          [os.path.join(HERE, '..', 'include', 'igw.h'), os.path.join(HERE, '..', 'include', 'igw_relabel.h')]
VERSION = 1
ROW = 1104          # bytes of a grid row
CELLS = 1089
RECORD = 64         # bytes of a trajectory record
MAX_G = 256
OUTPUTS = ('reward', 'done', 'progress', 'end', 'ret', 'target_size', 'target')   # in the order igw_relabel takes them
DEFAULT = ('reward', 'done', 'end', 'ret')
_vp, _i32, _i64, _f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
# every symbol include/igw_relabel.h declares: (result, arguments)
SIGNATURES = {
    'igw_relabel_version': (C.c_int, []),
    'igw_relabel_build_id': (C.c_char_p, []),
    'igw_relabel_last_error': (C.c_char_p, []),
    'igw_relabel': (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _f64, _f64, _i32, _f64] + [_vp] * 8),
}
EXPORTS = list(SIGNATURES)
LIBRARY = _build.Library(LIB, SOURCES, HEADERS, 'igw-relabel-build-id:', 'IGW_RELABEL_BUILD_ID', deps=[__file__])
source_hash, built_id, is_stale = LIBRARY.source_hash, LIBRARY.built_id, LIBRARY.is_stale


class RelabelError(RuntimeError):
    pass


def build(force=False, verbose=False):
    """Builds libigw_relabel.so; returns its path."""
    return LIBRARY.build(force, verbose=verbose)


BINDING = _build.Binding(LIBRARY, SIGNATURES, RelabelError, 'igw_relabel_last_error', 'igw_relabel_build_id',
                         'gridworld_amd.relabel', 'igw_relabel')
load, check, build_id = BINDING.load, BINDING.check, BINDING.build_id


def relabel_into(records, n_records, first, length, starts, targets, at, e, g, l, right_scale, wrong_scale, max_steps,
                 gamma, outputs, stream):
    """One igw_relabel call on raw pointers (ints; targets or at is None): `outputs` the seven of OUTPUTS (None = not
    wanted)."""
    rc = BINDING.load().igw_relabel(records, int(n_records), first, length, starts, targets, at, int(e), int(g), int(l),
                                    float(right_scale), float(wrong_scale), int(max_steps), float(gamma), *outputs, stream)
    if rc:
        BINDING.check(rc, 'igw_relabel')


def check_outputs(outputs):
    """The outputs named, in the library's order; ValueError for none or an unknown one."""
    names = (outputs,) if isinstance(outputs, str) else tuple(outputs)
    unknown = [k for k in names if k not in OUTPUTS]
    if unknown or not names:
        raise ValueError(f'relabel: outputs names one or more of {OUTPUTS}, got {outputs!r}')
    return tuple(k for k in OUTPUTS if k in names)


def _specs(e, g, l):
    """name -> (shape, strides, elements per episode, dtype) of the tensor a caller sees."""
    import torch
    step = ((e, g, l), (g * l, l, 1), g * l)
    pair = ((e, g), (g, 1), g)
    return {'reward': step + (torch.float32,), 'done': step + (torch.uint8,), 'progress': step + (torch.int16,),
            'end': pair + (torch.int32,), 'ret': pair + (torch.float32,), 'target_size': pair + (torch.int16,),
            'target': ((e, g, 9, 11, 11), (g * ROW, ROW, 121, 11, 1), g * ROW, torch.int8)}


def outputs(e, g, l, names, dev, stream=None):
    """New tensors for the outputs `names`, as relabel() returns them: `target` is an [E, G, 9, 11, 11] view of 1104-byte
    rows (each in the layout of `grid`)."""
    import torch
    res = {}
    with torch.cuda.stream(stream):
        for k in names:
            shape, strides, row, dtype = _specs(e, g, l)[k]
            res[k] = torch.as_strided(torch.empty((e, row), dtype=dtype, device=dev), shape, strides)
    return res


def _is(t, dtype, shape, dev):
    import torch
    return (torch.is_tensor(t) and t.dtype == dtype and tuple(t.shape) == tuple(shape) and t.device == dev
            and t.is_contiguous())


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
    out = dict(out or {})
    unknown = [k for k in out if k not in names]
    if unknown:
        raise ValueError(f'out holds {unknown}, the call writes {list(names)}')
    specs = _specs(e, g, l)
    for k, t in out.items():
        shape, strides, _, dtype = specs[k]
        if (not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dtype or t.device != dev
                or (t.numel() > 0 and tuple(t.stride()) != strides) or (k == 'target' and t.data_ptr() % 16)):
            raise ValueError(f'out[{k!r}] must be a {dtype} tensor {shape} with strides {strides} on {dev} (what relabel() '
                             'returns; target 16-byte aligned)')
    out.update(outputs(e, g, l, [k for k in names if k not in out], dev, alloc_stream))
    ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    if e:   # (the tensors of no episode have no address to pass)
        relabel_into(records.data_ptr(), records.numel() // RECORD, first.data_ptr(), length.data_ptr(), starts.data_ptr(),
                     ptr(targets), ptr(at), e, g, l, right, wrong, max_steps, gamma,
                     [out[k].data_ptr() if k in names else None for k in OUTPUTS], stream)
    return {k: out[k] for k in names}


def grid_rows(x, dev, lead):
    """An integer tensor or array [*lead, 9, 11, 11], [*lead, 1089] or [*lead, 1104] -> a contiguous int8 device tensor
    [*lead, 1104] (the one given, if it is that already)."""
    import numpy as np
    import torch
    t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
    lead = tuple(lead)
    if tuple(t.shape) == lead + (9, 11, 11):
        t = t.reshape(lead + (CELLS,))
    if tuple(t.shape) == lead + (ROW,):
        return t.to(device=dev, dtype=torch.int8).contiguous()
    if tuple(t.shape) != lead + (CELLS,):
        raise ValueError(f'relabel: grids must be {lead + (9, 11, 11)}, {lead + (CELLS,)} or {lead + (ROW,)}, got {tuple(t.shape)}')
    rows = torch.zeros(lead + (ROW,), dtype=torch.int8, device=dev)
    rows[..., :CELLS] = t.to(device=dev, dtype=torch.int8)
    return rows


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
