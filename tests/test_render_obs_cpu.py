"""CPU side of the training-layout observation ("Training-layout observations"): the entry as a
cross-compiled artefact (libigw_render_obs.so: exports, struct layout, argument checks, code-object gates of its
kernel; libigw_render.so and its build id untouched), the host layer
(ObsSpec, the VecGridWorld arguments, render.launch_obs on a stand-in library) and the model's luminance.  The GPU
comparison of kernel against model is tests/test_gpu_render_obs.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import jpeg_model as J
import obs_cases as OC
import obs_model as OM
from render_checks import LLVM, _buffers, _kernel_gates

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'igw_render_obs.h')


# ---- the library ----------------------------------------------------------------------------------------------------
def test_the_obs_entry_is_declared_exported_and_detectable():
    from gridworld_amd import render as R
    src = open(HEADER).read()
    assert re.search(r'#define IGW_RENDER_HAS_OBS 1\b', src)
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = sorted(set(re.findall(r'\b(igw_render_[a-z0-9_]+)\s*\(', code)))
    assert sorted(R.OBS_EXPORTS) == declared and 'igw_render_pov_obs' in declared
    L = R.OBS_BINDING.load()
    for name in declared:
        assert hasattr(L, name)
    assert R.OBS_BINDING.build_id() == R.OBS_LIBRARY.source_hash() == R.OBS_LIBRARY.built_id()
    assert not R.OBS_LIBRARY.is_stale()
    # its build id covers the ray caster it compiles and its own files; the render library is made of what it was
    # made of (version 1, no new source), so its build id and the profiles that carry it stay valid
    names = lambda files: {os.path.basename(f) for f in files}  # noqa: E731
    assert names(R.OBS_SOURCES + R.OBS_HEADERS) == {'igw_render_obs.hip', 'igw_render_obs_stage.h', 'igw_render_obs.h',
                                                    'igw_render_frame.h', 'igw_render.h'}
    assert names(R.SOURCES + R.HEADERS) == {'igw_render.hip', 'igw_render_frame.h', 'igw_render.h'}
    assert R.load().igw_render_version() == 1 and not hasattr(R.load(), 'igw_render_pov_obs')
    assert [R.OBS_DTYPES[d] for d in (torch.uint8, torch.float16, torch.bfloat16, torch.float32)] == [0, 1, 2, 3]
    assert re.search(r'IGW_OBS_U8 = 0, IGW_OBS_F16 = 1, IGW_OBS_BF16 = 2, IGW_OBS_F32 = 3', src)


def test_the_ctypes_mirror_has_the_headers_size_and_offsets(tmp_path):
    from gridworld_amd import render as R
    fields = [f[0] for f in R.Obs._fields_]
    prog = tmp_path / 'layout.c'
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "igw_render_obs.h"\nint main(void) {\n'
                    '    printf("%zu %d\\n", sizeof(igw_render_obs), IGW_RENDER_OBS_BYTES);\n'
                    + ''.join(f'    printf("{f} %zu\\n", offsetof(igw_render_obs, {f}));\n' for f in fields)
                    + '    return 0;\n}\n')
    exe = str(tmp_path / 'layout')
    subprocess.check_call([os.path.join(LLVM, 'clang'), '-I', os.path.join(ROOT, 'include'), str(prog), '-o', exe])
    out = subprocess.check_output([exe], text=True).split('\n')
    size, stated = map(int, out[0].split())
    assert size == stated == ctypes.sizeof(R.Obs) == 48
    for line, f in zip(out[1:], fields):
        name, off = line.split()
        assert name == f and int(off) == getattr(R.Obs, f).offset, line
    # the struct holds nothing the mirror does not name
    body = re.search(r'typedef struct igw_render_obs \{(.*?)\}', re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S),
                     re.S).group(1)
    assert re.findall(r'(\w+)\s*[,;]', body) == fields


def _obs(p16, **kw):
    from gridworld_amd import render as R
    a = dict(data=p16, dtype=0, gray=0, stack=1, fill=0, scale=1.0, bias=0.0, restart=None, restart_stride=0)
    a.update(kw)
    return R.Obs(*[a[f[0]] for f in R.Obs._fields_])


def test_the_obs_entry_rejects_bad_arguments_and_a_missing_device():
    from gridworld_amd import render as R
    L = R.OBS_BINDING.load()
    buf, p16 = _buffers()

    def call(obs, n=1, out=p16, grid=p16, w=64, h=64):
        return L.igw_render_pov_obs(p16, grid, p16, n, p16, 128, out, w, h, None if obs is None else ctypes.byref(obs),
                                    None)
    bad = [dict(dtype=4), dict(dtype=-1), dict(stack=0), dict(stack=9), dict(scale=2.0), dict(bias=1.0),
           dict(dtype=1, scale=float('inf')), dict(dtype=3, bias=float('nan')), dict(dtype=2, scale=float('nan')),
           dict(data=None), dict(dtype=1, data=p16 + 1), dict(dtype=2, data=p16 + 3), dict(dtype=3, data=p16 + 2),
           dict(restart=p16, restart_stride=0)]
    for kw in bad:
        assert call(_obs(p16, **kw)) == -1, kw
        assert L.igw_render_obs_last_error()
    assert call(None) == -1
    # the sibling's own checks hold too
    assert call(_obs(p16), n=-1) == -1 and call(_obs(p16), grid=p16 + 4) == -1 and call(_obs(p16), w=0) == -1
    good = [dict(), dict(dtype=1, scale=1 / 255, data=p16 + 2), dict(dtype=3, bias=-128.0, stack=8, data=p16 + 4),
            dict(data=p16 + 1, gray=1, stack=4, restart=p16 + 52, restart_stride=64), dict(dtype=2, fill=1)]
    for kw in good:
        for out in (p16, None):        # the frame is optional
            if torch.cuda.is_available():
                assert call(_obs(p16, **kw), n=0, out=out) == 0, kw
            else:
                assert call(_obs(p16, **kw), out=out) == -2 and b'no CPU fallback' in L.igw_render_obs_last_error(), kw
                assert call(_obs(p16, **kw), n=0, out=out) == -2


def _code_object(lib, tmp_path, tag):
    """(notes, disassembly) of the gfx950 code object inside the library file `lib`."""
    tools = [os.path.join(LLVM, t) for t in ('llvm-objcopy', 'clang-offload-bundler', 'llvm-readelf', 'llvm-objdump')]
    fat, co = str(tmp_path / (tag + '.bin')), str(tmp_path / (tag + '.co'))
    subprocess.check_call([tools[0], '--dump-section', '.hip_fatbin=' + fat, lib])
    subprocess.check_call([tools[1], '--type=o', '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--input=' + fat,
                           '--output=' + co, '--unbundle'])
    return (subprocess.check_output([tools[2], '--notes', co], text=True),
            subprocess.check_output([tools[3], '-d', co], text=True))


def test_the_obs_kernel_passes_the_code_object_gates(tmp_path):
    """No scratch, no spills, the plain kernel's LDS and registers; its stores are vector stores of 4, 8 and 16 bytes
    (four pixels of u8, f16 / bf16, f32) with the 1-, 2- and 4-byte stores of the scalar head and tail."""
    from gridworld_amd import render as R
    R.build()
    notes, asm = _code_object(R.LIB, tmp_path, 'render')
    _, val, plain = _kernel_gates(notes, asm, 'igw_render_pov_kernel')
    notes, asm = _code_object(R.OBS_LIB, tmp_path, 'obs')
    assert len(notes.split('- .agpr_count:')) == 2            # the library holds this one kernel
    _, oval, body = _kernel_gates(notes, asm, 'igw_obs_pov_kernel')
    assert oval('private_segment_fixed_size') == 0 and oval('vgpr_spill_count') == 0 and oval('sgpr_spill_count') == 0
    assert oval('group_segment_fixed_size') == val('group_segment_fixed_size')
    assert oval('vgpr_count') <= val('vgpr_count') + 8       # the ray caster keeps its occupancy
    for ins in ('global_store_dwordx4', 'global_store_dwordx2', 'global_store_dword ', 'global_store_short',
                'global_store_byte', 'global_load_dwordx4', 'global_load_dwordx2'):
        assert ins in body, ins
    # scale and bias are two roundings: the stage adds no fused multiply-add on f32 to the ray caster's own (the
    # expansions of its divisions)
    fused = r'\bv_(fma|mad|fmac|mac)_f32'
    assert len(re.findall(fused, body)) == len(re.findall(fused, plain))


# ---- ObsSpec and the env's arguments ----------------------------------------------------------------------------------
def test_obs_spec_validates_on_construction_and_gives_the_shape():
    import gridworld_amd as G
    from gridworld_amd import render as R
    assert G.ObsSpec is R.ObsSpec
    s = G.ObsSpec()
    assert (s.dtype, s.gray, s.stack, s.scale, s.bias) == (torch.uint8, False, 1, 1.0, 0.0)
    assert s.shape(5, (64, 32)) == (5, 3, 32, 64)
    assert G.ObsSpec(torch.float16, gray=True, stack=4, scale=1 / 255).shape(2, (13, 7)) == (2, 4, 7, 13)
    assert G.ObsSpec(torch.bfloat16, stack=3, scale=2 / 255, bias=-1).shape(2, (8, 8)) == (2, 9, 8, 8)
    for bad in (dict(dtype=torch.int32), dict(dtype=torch.float64), dict(dtype='half2'), dict(stack=0), dict(stack=9),
                dict(stack=2.5), dict(scale=2.0), dict(bias=1.0), dict(dtype=torch.float16, scale=float('inf')),
                dict(dtype=torch.float32, bias=float('nan')), dict(dtype=torch.float32, scale=1e39)):
        with pytest.raises(ValueError):
            G.ObsSpec(**bad)
    assert R.ObsSpec.of(dict(dtype=torch.float32, stack=2)).stack == 2 and R.ObsSpec.of(s) is s
    with pytest.raises(ValueError):
        R.ObsSpec.of('gray')


def test_the_env_refuses_the_combinations_that_cannot_be_drawn():
    """Each raises ValueError before any device work (so also on a machine without a GPU)."""
    import gridworld_amd as G
    spec = G.ObsSpec(gray=True, stack=4)
    for kw in (dict(pov_obs=spec),                                                # needs renderer='hip'
               dict(renderer='hip', pov_obs=spec, pov_outputs=('rgb', 'depth')),  # planes are not in this layout
               dict(renderer='hip', pov_obs=spec, pov_outputs=('depth',)),
               dict(renderer='hip', pov_frame=False),                             # nothing left to draw
               dict(pov_frame=False),
               dict(renderer='hip', pov_obs=dict(stack=9)),
               dict(renderer='hip', pov_obs=dict(dtype=torch.uint8, scale=0.5)),
               dict(renderer='hip', pov_obs='gray')):
        with pytest.raises(ValueError):
            G.VecGridWorld(4, **kw)


# ---- the host path: render.launch_obs on a stand-in library -----------------------------------------------------------
class Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


def test_launch_obs_reaches_the_obs_entry_with_the_struct_it_describes(monkeypatch):
    from gridworld_amd import render as R
    rec = Recorder()
    monkeypatch.setattr(R.OBS_BINDING, 'lib', rec)
    cpu, n, W, H = torch.device('cpu'), 5, 24, 16
    atlas = torch.zeros((16, 16, 4), dtype=torch.uint8)
    head = (0x1000, 0x2000, 0x3000, n)
    spec = R.ObsSpec(torch.float16, gray=True, stack=4, scale=1 / 255, bias=-0.5)
    records = torch.zeros((n, 64), dtype=torch.uint8)
    out = torch.zeros(spec.shape(n, (W, H)), dtype=torch.float16)
    frame = torch.zeros((n, H, W, 3), dtype=torch.uint8)
    res = R.launch_obs(head, n, (W, H), spec, out, frame, records[:, 52], False, atlas, cpu, 0x77)
    assert res is out and len(rec.calls) == 1
    name, args = rec.calls[0]
    assert name == 'igw_render_pov_obs' and len(args) == len(R.OBS_SIGNATURES[name][1])
    assert args[:4] == head and args[4:6] == (atlas.data_ptr(), 16)
    assert args[6:9] == (frame.data_ptr(), W, H) and args[-1] == 0x77
    o = args[-2]._obj
    assert isinstance(o, R.Obs)
    assert (o.data, o.dtype, o.gray, o.stack, o.fill) == (out.data_ptr(), 1, 1, 4, 0)
    assert (o.scale, o.bias) == (float(np.float32(1 / 255)), -0.5)
    assert (o.restart, o.restart_stride) == (records.data_ptr() + 52, 64)
    # no out: a new tensor, which is always a fill; no frame: out = NULL; no restart: NULL
    res = R.launch_obs(head, n, (W, H), spec, None, None, None, False, atlas, cpu, 0x77)
    o = rec.calls[1][1][-2]._obj
    assert tuple(res.shape) == (n, 4, H, W) and res.dtype == torch.float16 and o.data == res.data_ptr()
    assert o.fill == 1 and o.restart is None and rec.calls[1][1][6] is None
    mask = torch.zeros(n, dtype=torch.bool)
    R.launch_obs(head, n, (W, H), spec, out, None, mask, True, atlas, cpu, 0x77)
    o = rec.calls[2][1][-2]._obj
    assert (o.fill, o.restart, o.restart_stride) == (1, mask.data_ptr(), 1)
    for kw in (dict(out=out.float()), dict(out=out[:, :2]), dict(out=out.permute(0, 1, 3, 2)),
               dict(frame=frame[..., :2]), dict(restart=torch.zeros(n + 1, dtype=torch.uint8)),
               dict(restart=torch.zeros(n, dtype=torch.int32)), dict(restart=torch.zeros((n, 1), dtype=torch.uint8)),
               dict(size=(0, H)), dict(size=(W, 1025))):
        a = dict(out=out, frame=None, restart=None, size=(W, H))
        a.update(kw)
        with pytest.raises(ValueError):
            R.launch_obs(head, n, a['size'], spec, a['out'], a['frame'], a['restart'], False, atlas, cpu, 0x77)
    assert len(rec.calls) == 3


# ---- the model ------------------------------------------------------------------------------------------------------
def test_the_models_luminance_on_the_cube_corners_and_against_the_codecs_y():
    corners = torch.tensor([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], dtype=torch.uint8)
    want = {(0, 0, 0): 0, (0, 0, 255): 29, (0, 255, 0): 150, (0, 255, 255): 179, (255, 0, 0): 76, (255, 0, 255): 105,
            (255, 255, 0): 226, (255, 255, 255): 255}
    got = OM.luminance(corners)
    assert got.dtype == torch.uint8
    for c, y in zip(corners.tolist(), got.tolist()):
        assert want[tuple(c)] == y == (19595 * c[0] + 38470 * c[1] + 7471 * c[2] + 32768) >> 16
    assert 19595 + 38470 + 7471 == 65536                              # white stays 255, grey levels stay themselves
    rng = np.random.RandomState(3)
    rgb = rng.randint(0, 256, (40, 50, 3)).astype(np.uint8)
    assert np.array_equal(OM.luminance(torch.from_numpy(rgb)).numpy(), J.ycc(rgb)[..., 0])


def test_the_model_fills_shifts_and_converts_as_the_contract_says():
    from gridworld_amd import render as R
    rng = np.random.RandomState(4)
    f = [torch.from_numpy(rng.randint(0, 256, (3, 5, 7, 3)).astype(np.uint8)) for _ in range(3)]
    spec = R.ObsSpec(torch.float32, stack=3, scale=2 / 255, bias=-1)
    s0 = OM.observe(f[0], None, None, spec)
    assert s0.shape == (3, 9, 5, 7) and s0.dtype == torch.float32
    chw = lambda x: (x.permute(0, 3, 1, 2).float() * np.float32(2 / 255)) + np.float32(-1)  # noqa: E731
    for k in range(3):
        assert torch.equal(s0[:, 3 * k:3 * k + 3], chw(f[0]))
    s1 = OM.observe(f[1], s0, None, spec)
    assert torch.equal(s1[:, :6], s0[:, 3:]) and torch.equal(s1[:, 6:], chw(f[1]))
    s2 = OM.observe(f[2], s1, torch.tensor([0, 255, 0], dtype=torch.uint8), spec)
    assert torch.equal(s2[0, :6], s1[0, 3:]) and torch.equal(s2[2, 6:], chw(f[2])[2])
    for k in range(3):
        assert torch.equal(s2[1, 3 * k:3 * k + 3], chw(f[2])[1])
    g = OM.observe(f[0], None, None, R.ObsSpec(gray=True, stack=2))
    assert g.shape == (3, 2, 5, 7) and torch.equal(g[:, 0], OM.luminance(f[0])) and torch.equal(g[:, 1], g[:, 0])
    h = OM.observe(f[0], None, None, R.ObsSpec(torch.bfloat16, scale=1 / 255))
    assert h.dtype == torch.bfloat16 and OM.bits(h).dtype == torch.int16


def test_the_shared_batch_restarts_64_times_by_the_time_limit_alone():
    """The oracle on the batch of tests/obs_cases.py: the empty-target rows are done on every step, the others only at
    steps 7 and 14 -- so the GPU test's bound of 32..96 restarts can be met neither by never nor by always restarting."""
    from oracle import oracle as O
    targets, poses, actions = OC.inputs()
    b = O.OracleBatch(OC.N, max_steps=OC.MAX_STEPS)
    b.set_tasks(targets)
    b.set_initial_pose(poses)
    b.reset()
    done = []
    for t in range(OC.STEPS):
        b.step_walking(actions[t], autoreset=True)
        done.append(b.done.copy())
    done = np.stack(done)
    assert done[:, :OC.EMPTY].all()
    assert done[:, OC.EMPTY:].sum() == 64
    assert [t for t in range(OC.STEPS) if done[t, OC.EMPTY:].any()] == [6, 13]
