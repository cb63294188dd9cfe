"""The recall query of the episode log: builds and binds libigw_recall.so (include/igw_recall.h).

    spec = G.VoxSpec(planes=(('grid', 'onehot'), ('target', 'onehot')), agent=True, dtype=torch.float16, stack=4)
    r = env.relabel(G.relabel_future(...), outputs=('reward', 'done', 'target'))    # the HER loop: rewards,
    m = env.recall(spec, batch=4096, seed=step, goals=r, goal=g)                    # observations,
    m['obs'], m['next_obs'] [B, K * C, 9, S, S], m['action'], m['reward_relabel']   # and the learner
    m = G.recall(records, first, length, starts, init_pose, episode, step, spec)    # the stateless form

The library is a separate one, as the renderer's, the codec's and the other queries' are: it reads trajectory records
(include/igw.h: igw_set_trajectory_log), starting grids, reset poses and goal rows, no env state, and is not part of the
step library's build (its sources and build id are its own, so the step library's profiles stay valid); the element,
the frame of a pose, the staging of the planes and the slot writer (csrc/igw_voxel.h, igw_voxel_table.h,
igw_voxel_stage.h) it shares with the voxel observation's library.  There is no CPU fallback: without a HIP device the
launch fails and the call raises.
"""
import ctypes as C
import functools
import sys

from . import _out
from . import build as _build
from . import vox as _vox
from ._out import _is

VERSION = 1
ROW = 1104          # bytes of a grid row
CELLS = 1089
RECORD = 64         # bytes of a trajectory record
MAX_PLANES, MAX_STACK, MAX_RADIUS = 4, 8, 10
GRID, GOAL = 0, 1
SOURCES_OF = {'grid': GRID, 'target': GOAL}         # a VoxSpec's plane names the query knows
OUTPUTS = ('obs', 'next_obs', 'record', 'valid')    # in the order igw_recall takes them
DEFAULT = ('obs', 'next_obs', 'record')
ENV_DEFAULT = OUTPUTS                               # env.recall draws samples that may be padding: it returns `valid` too
SPACES = ('walking', 'flying', 'walking_dict')
NO_CLAMP = (1 << 31) - 1
_vp, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64


class Plane(C.Structure):
    """igw_recall_plane."""
    _fields_ = [('source', _i32), ('encoding', _i32)]


class Spec(C.Structure):
    """igw_recall_spec."""
    _fields_ = [('planes', Plane * MAX_PLANES), ('num_planes', _i32), ('agent_plane', _i32), ('frame', _i32),
                ('radius', _i32), ('dtype', _i32), ('stack', _i32), ('scale', C.c_float), ('bias', C.c_float)]


class RecallError(RuntimeError):
    pass


# include/igw_recall.h declares igw_recall and the three symbols every library has: (result, arguments)
LIBRARY, BINDING = _build.query('recall', __file__, {
    'igw_recall': (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _i32, _vp, _i64, _i64, _vp,
                             C.POINTER(Spec), _vp, _vp, _vp, _vp, _vp]),
}, RecallError, 'igw_recall', headers=['igw_voxel.h', 'igw_voxel_table.h', 'igw_voxel_stage.h'], device=False)
LIB, SOURCES, HEADERS = LIBRARY.lib, LIBRARY.sources, LIBRARY.headers
SIGNATURES, EXPORTS = BINDING.signatures, list(BINDING.signatures)
build, source_hash, built_id, is_stale = LIBRARY.build, LIBRARY.source_hash, LIBRARY.built_id, LIBRARY.is_stale
load, check, build_id = BINDING.load, BINDING.check, BINDING.build_id
check_outputs = functools.partial(_out.check_outputs, 'recall', OUTPUTS)
grid_rows = functools.partial(_out.grid_rows, 'recall: starts')


def spec_of(spec):
    """(VoxSpec, filled Spec) of a VoxSpec or a dict of its arguments.  ValueError for a 'want' / 'todo' plane: those are
    the goal query's rows of the LIVE state; the goal query on a historic state is out of scope."""
    spec = _vox.VoxSpec.of(spec)
    other = [name for name, _ in spec.planes if name not in SOURCES_OF]
    if other:
        raise ValueError(f"recall: the planes {other} are the goal query's rows of the live state, which a logged entry "
                         f"does not have; a recalled observation takes the planes {tuple(SOURCES_OF)}")
    s = Spec()
    for k, (name, enc) in enumerate(spec.planes):
        s.planes[k] = Plane(SOURCES_OF[name], _vox.ENCODINGS[enc])
    s.num_planes, s.agent_plane, s.frame, s.radius = len(spec.planes), int(spec.agent), _vox.FRAMES[spec.frame], spec.radius
    s.dtype, s.stack, s.scale, s.bias = _vox.DTYPES[spec.dtype], spec.stack, spec.scale, spec.bias
    return spec, s


def needs_goal(spec):
    return any(name == 'target' for name, _ in spec.planes)


def recall_into(records, n_records, first, length, starts, init_pose, e, l, episode, step, b, goal, goal_stride,
                n_goal_rows, goal_index, spec, outputs, stream):
    """One igw_recall call on raw pointers (ints or None) and a filled Spec: `outputs` the four of OUTPUTS (None = not
    wanted)."""
    rc = BINDING.load().igw_recall(records, int(n_records), first, length, starts, init_pose, int(e), int(l), episode,
                                   step, int(b), goal, int(goal_stride), int(n_goal_rows), goal_index, C.byref(spec),
                                   *outputs, stream)
    if rc:
        BINDING.check(rc, 'igw_recall')


def _specs(spec, b):
    """name -> _out.spec of the contiguous tensor a caller sees; `record` is 4-byte aligned (decode() views it)."""
    import torch
    obs = _out.spec(spec.shape(b), spec.dtype)
    return {'obs': obs, 'next_obs': obs, 'record': _out.spec((b, RECORD), torch.uint8, align=4),
            'valid': _out.spec((b,), torch.uint8)}


def outputs(spec, b, names, dev, stream=None):
    """New tensors for the outputs `names`, as recall() returns them."""
    return _out.outputs('recall', OUTPUTS, names, _specs(spec, b), None, dev, stream)[0]


def goal_rows(t):
    """(pointer, row stride in bytes, rows) of goal rows given as an int8 tensor [..., 9, 11, 11] with dense cells --
    contiguous or a view of wider rows, as relabel's `target` is -- or [..., >= 1089]: the leading dimensions are one
    run of rows at one stride."""
    import torch
    ok = torch.is_tensor(t) and t.dtype == torch.int8
    if ok and t.dim() >= 4 and tuple(t.shape[-3:]) == (9, 11, 11) and tuple(t.stride()[-3:]) == (121, 11, 1):
        lead, strides = tuple(t.shape[:-3]), tuple(t.stride()[:-3])
    elif ok and t.dim() >= 2 and t.shape[-1] >= CELLS and t.stride(-1) == 1:
        lead, strides = tuple(t.shape[:-1]), tuple(t.stride()[:-1])
    else:
        ok = False
    if ok:
        n, stride = 1, None
        for size, st in zip(reversed(lead), reversed(strides)):
            if size != 1:
                if stride is None:
                    stride = st
                elif st != stride * n:
                    ok = False
            n *= size
        stride = CELLS if stride is None else stride
        ok = ok and stride >= CELLS
    if not ok:
        raise ValueError('recall: goal must be an int8 tensor [..., 9, 11, 11] with dense cells or [..., >= 1089], its rows '
                         'at one stride of >= 1089 bytes')
    return t.data_ptr(), stride, n


def decode(record, space='walking'):
    """Views of a record tensor uint8 [B, 64] (4-byte aligned; include/igw.h's layout): reward float32 [B], done uint8
    [B], inventory int16 [B, 6], agent_pos float32 [B, 5] (x, y, z, pitch, yaw), and the action as executed -- walking:
    action int32 [B]; flying: movement float32 [B, 3], camera float32 [B, 2] (inventory and placement sit in the bits of
    byte 43: `action_bits`); walking_dict: buttons uint8 [B, 8], camera float32 [B, 2].  Nothing is copied."""
    import torch
    if space not in SPACES:
        raise ValueError(f'recall: space is one of {SPACES}, got {space!r}')
    f32, i16 = record.view(torch.float32), record.view(torch.int16)
    res = dict(agent_pos=f32[:, 0:5], reward=f32[:, 5], inventory=i16[:, 14:20], done=record[:, 42],
               action_bits=record[:, 43])
    if space == 'walking':
        res['action'] = record.view(torch.int32)[:, 11]
    elif space == 'flying':
        res.update(movement=f32[:, 11:14], camera=f32[:, 14:16])
    else:
        res.update(buttons=record[:, 44:52], camera=f32[:, 13:15])
    return res


def launch(records, first, length, starts, init_pose, episode, step, spec, goal, goal_index, cap, names, out, dev, stream,
           alloc_stream=None, space='walking'):
    """One igw_recall launch; returns the dict name -> tensor of `names` (a subset of OUTPUTS) plus decode()'s views of
    `record` when that is among them.  Every input is a contiguous device tensor of the header's dtype: records uint8
    [..., 64], first int64 [E], length int32 [E], starts int8 [E, 1104], init_pose float64 [E, 5], episode / step int32
    [B], goal None or what goal_rows() takes, goal_index None or int64 [B]; `cap` is L.  `out` (a dict or None) holds
    tensors to write, as an earlier call returned them; what it lacks is allocated.  It touches the device only through
    data_ptr() and the ctypes call."""
    import torch
    names = check_outputs(names)
    spec, s = spec_of(spec)
    if space not in SPACES:
        raise ValueError(f'recall: space is one of {SPACES}, got {space!r}')
    e = int(first.shape[0]) if torch.is_tensor(first) and first.dim() == 1 else -1
    if not (torch.is_tensor(records) and records.dtype == torch.uint8 and records.device == dev and records.is_contiguous()
            and records.dim() >= 1 and records.shape[-1] == RECORD):
        raise ValueError(f'recall: records must be a contiguous uint8 tensor [..., {RECORD}] on {dev}')
    if e < 0 or not _is(first, torch.int64, (e,), dev) or not _is(length, torch.int32, (e,), dev):
        raise ValueError(f'recall: first must be an int64 and length an int32 tensor [E] on {dev}')
    if not _is(starts, torch.int8, (e, ROW), dev):
        raise ValueError(f'recall: starts must be an int8 tensor [{e}, {ROW}] on {dev}')
    if not _is(init_pose, torch.float64, (e, 5), dev):
        raise ValueError(f'recall: init_pose must be a float64 tensor [{e}, 5] on {dev}')
    b = int(episode.shape[0]) if torch.is_tensor(episode) and episode.dim() == 1 else -1
    if b < 0 or not _is(episode, torch.int32, (b,), dev) or not _is(step, torch.int32, (b,), dev):
        raise ValueError(f'recall: episode and step must be int32 tensors [B] on {dev}')
    if int(cap) < 1:
        raise ValueError(f'recall: pad must be >= 1, got {cap}')
    gptr, gstride, grows = None, 0, 0
    if goal is not None:
        if not torch.is_tensor(goal) or goal.device != dev:
            raise ValueError(f'recall: goal must be an int8 tensor on {dev}')
        gptr, gstride, grows = goal_rows(goal)
    elif needs_goal(spec):
        raise ValueError("recall: a 'target' plane reads the goal rows: pass goal=")
    if goal_index is not None and (goal is None or not _is(goal_index, torch.int64, (b,), dev)):
        raise ValueError(f'recall: goal_index goes with goal and must be an int64 tensor [{b}] on {dev}')
    res, ptrs = _out.outputs('recall', OUTPUTS, names, _specs(spec, b), out, dev, alloc_stream)
    if b:   # (the tensors of no sample have no address to pass)
        recall_into(records.data_ptr(), records.numel() // RECORD, first.data_ptr(), length.data_ptr(), starts.data_ptr(),
                    init_pose.data_ptr(), e, min(int(cap), NO_CLAMP), episode.data_ptr(), step.data_ptr(), b, gptr, gstride,
                    grows, _out.ptr(goal_index), s, ptrs, stream)
    if 'record' in res:
        res.update(decode(res['record'], space))
    return res


def recall(records, first, length, starts, init_pose, episode, step, spec, goal=None, goal_index=None, outputs=DEFAULT,
           out=None, *, pad=None, space='walking'):
    """Voxel observations of logged transitions, the stateless device form: one igw_recall launch
    on the current stream of the records' device.
      records    uint8 device tensor [..., 64]: trajectory records (what enable_trajectory_log returns, or any buffer of
                 that layout)
      first      [E] index of each episode's first record; length [E] its steps; starts [E, 9, 11, 11] (or [E, 1089] /
                 [E, 1104]) the grid it started from; init_pose [E, 5] x, y, z, yaw, pitch of its reset
      episode    [B] and step [B]: sample b is step t = step[b] (1 .. length) of episode episode[b]
      spec       a VoxSpec (or a dict of its arguments) with planes 'grid' and 'target'; 'target' is the sample's goal row
      goal       int8 device rows [..., 9, 11, 11] / [..., >= 1089] (relabel's `target`, or any targets in the user's
                 frame); goal_index [B] the row of each sample, by default its episode
    Returns a dict of the `outputs` named: obs / next_obs [B, K * C, 9, S, S] of spec.dtype -- what a live vox_obs stack
    of K showed before and after the step, on the LOG's float32 poses --, record uint8 [B, 64] (the step's record, with
    decode()'s views of it: action, reward, done, inventory, agent_pos for `space`), valid uint8 [B] (0: a padding sample
    -- an episode, step or goal row out of range -- whose observations are all `bias` and whose record is zeros).
    `length` is clamped to `pad` (default: the log's capacity records.shape[-2] when records has that dimension, else not
    at all).  Inputs that already are contiguous device tensors of the library's dtypes are passed as they are; `out`
    holds tensors to write, as an earlier call returned them: with every output given nothing is allocated."""
    import torch
    if not torch.is_tensor(records) or not records.is_cuda:
        raise ValueError('recall: records must be a device tensor')
    spec, _ = spec_of(spec)
    names = check_outputs(outputs)
    dev = records.device
    conv = lambda x, dt: (x if torch.is_tensor(x) else torch.as_tensor(x)).to(device=dev, dtype=dt).contiguous()  # noqa: E731
    first, length = conv(first, torch.int64).reshape(-1), conv(length, torch.int32).reshape(-1)
    e = first.shape[0]
    starts = grid_rows(starts, dev, (e,))
    init_pose = conv(init_pose, torch.float64).reshape(e, 5)
    episode, step = conv(episode, torch.int32).reshape(-1), conv(step, torch.int32).reshape(-1)
    if goal_index is not None:
        goal_index = conv(goal_index, torch.int64).reshape(-1)
    if pad is None:
        pad = records.shape[-2] if records.dim() >= 3 else NO_CLAMP
    stream = torch.cuda.current_stream(dev).cuda_stream
    return launch(records.contiguous(), first, length, starts, init_pose, episode, step, spec, goal, goal_index, pad,
                  names, out, dev, stream, space=space)


def sample(length, batch, seed=0):
    """`batch` (episode, step) pairs drawn with a torch generator seeded by `seed` on length's device: the episode
    uniform over the E of `length` (int32 [E]), the step 1 + floor(u * max(length[e], 1)), so an episode of no steps
    yields a step its length does not hold (a padding sample).  int32 [batch] each; nothing comes to the host."""
    import torch
    gen = torch.Generator(device=length.device)
    gen.manual_seed(int(seed))
    e = int(length.shape[0])
    u = torch.rand((2, int(batch)), generator=gen, device=length.device, dtype=torch.float64)
    episode = (u[0] * e).floor().clamp(0, max(e - 1, 0)).long()
    n = length.index_select(0, episode).clamp(min=1).to(torch.float64)
    step = torch.minimum((u[1] * n).floor() + 1, n)
    return episode.to(torch.int32), step.to(torch.int32)


class _Callable(type(sys)):
    """The module as the package's attribute of the same name: G.recall(...) is the function, G.recall.build() and the
    rest of the module stay reachable."""

    def __call__(self, *args, **kw):
        return recall(*args, **kw)


sys.modules[__name__].__class__ = _Callable

if __name__ == '__main__':
    print(build(force='--force' in sys.argv, verbose=True))
