"""CPU side of the codec library (include/igw_codec.h) as a cross-compiled artefact: its exports and signatures, the
argument checks that come ahead of the device check, igw_jpeg_bound, the gfx950 code object's gates, and the build ids
of the step and render libraries, which the codec must not move."""
import ctypes
import os
import re
import subprocess

import pytest

from render_checks import LLVM, _buffers, _forbidden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# build.source_hash() / render.source_hash() of the commit the codec was added to
STEP_ID, RENDER_ID = '58449f9385b3ae9a', 'a477b6523498158f'
C_TYPES = {'int': ctypes.c_int, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'const char*': ctypes.c_char_p,
           'const uint8_t*': ctypes.c_void_p, 'uint8_t*': ctypes.c_void_p, 'int32_t*': ctypes.c_void_p,
           'void*': ctypes.c_void_p}


def _declared():
    """name -> (result type, [argument types]) of every function include/igw_codec.h declares."""
    src = open(os.path.join(ROOT, 'include', 'igw_codec.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    out = {}
    for res, name, args in re.findall(r'^([a-z0-9_ ]+?\*?)\s*\b(igw_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', src, re.M):
        args = [] if args.strip() == 'void' else [re.sub(r'\s*\b\w+$', '', a.strip()) for a in args.split(',')]
        out[name] = (res.strip(), args)
    return out


def test_codec_library_exports_its_declared_symbols_with_their_signatures():
    from gridworld_amd import codec as K
    L = K.load()
    decl = _declared()
    assert sorted(decl) == sorted(K.EXPORTS) and len(decl) == 5
    for name, (res, args) in decl.items():
        assert hasattr(L, name), name
        want_res, want_args = K.SIGNATURES[name]
        assert C_TYPES[res] is want_res, name
        assert [C_TYPES[a] for a in args] == want_args, name
    assert L.igw_codec_version() == K.VERSION == 1
    assert K.build_id() == K.source_hash() == K.built_id()
    assert not K.is_stale()


def test_jpeg_bound_needs_no_device_and_covers_the_worst_block():
    from gridworld_amd import codec as K
    L = K.load()
    for w, h in ((1, 1), (64, 64), (96, 40), (1024, 1024)):
        blocks = 3 * ((w + 7) // 8) * ((h + 7) // 8)
        b = L.igw_jpeg_bound(w, h)
        # a block's longest sequence is 22 + 63 * 26 bits (the longest DC and AC codes with their extra bits); every
        # byte of it may be stuffed; the header, the padded last byte and EOI come on top
        assert b % 16 == 0 and b >= K.HEADER_BYTES + 2 * (blocks * (22 + 63 * 26) // 8 + 1) + 2
        assert K.jpeg_bound(w, h) == b
        assert K.HEADER_BYTES + 2 <= K.default_stride(w, h) <= b
    for w, h in ((0, 8), (8, 0), (1025, 8), (8, 1025), (-1, -1)):
        assert L.igw_jpeg_bound(w, h) == 0
    with pytest.raises(ValueError):
        K.jpeg_bound(0, 8)


def test_jpeg_encode_rejects_bad_arguments_ahead_of_the_device_check():
    import torch
    from gridworld_amd import codec as K
    L = K.load()
    buf, p16 = _buffers()
    ok = dict(frames=p16, n=1, w=64, h=64, c=3, q=90, out=p16, stride=4096, sizes=p16)

    def call(**kw):
        a = dict(ok, **kw)
        return L.igw_jpeg_encode(a['frames'], a['n'], a['w'], a['h'], a['c'], a['q'], a['out'], a['stride'],
                                 a['sizes'], None)
    for bad in (dict(c=2), dict(c=5), dict(w=0), dict(h=0), dict(w=1025), dict(h=1025), dict(q=0), dict(q=101),
                dict(n=-1), dict(n=1 << 31), dict(stride=624), dict(stride=0), dict(stride=-4096), dict(frames=0),
                dict(out=0), dict(sizes=0), dict(sizes=p16 + 2)):
        assert call(**bad) == -1, bad
        assert L.igw_codec_last_error()
    if torch.cuda.is_available():
        assert call(n=0) == 0
    else:
        assert call() == -2 and b'no CPU fallback' in L.igw_codec_last_error()
        assert call(n=0) == -2
        with pytest.raises(K.CodecError):
            K.encode_jpeg(torch.zeros((1, 8, 8, 3), dtype=torch.uint8))
    with pytest.raises(ValueError):
        K.encode_jpeg(torch.zeros((1, 8, 8, 2), dtype=torch.uint8))
    with pytest.raises(ValueError):
        K.encode_jpeg(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), quality=0)


def test_codec_code_object_has_no_scratch_no_spills_and_no_scalar_stores(tmp_path):
    from gridworld_amd import codec as K
    lib = K.build()
    tools = [os.path.join(LLVM, t) for t in ('llvm-objcopy', 'clang-offload-bundler', 'llvm-readelf', 'llvm-objdump')]
    fat, co = str(tmp_path / 'fat.bin'), str(tmp_path / 'dev.co')
    subprocess.check_call([tools[0], '--dump-section', '.hip_fatbin=' + fat, lib])
    subprocess.check_call([tools[1], '--type=o', '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--input=' + fat,
                           '--output=' + co, '--unbundle'])
    notes = subprocess.check_output([tools[2], '--notes', co], text=True)
    asm = subprocess.check_output([tools[3], '-d', co], text=True)
    kern = [b for b in notes.split('- .agpr_count:')[1:] if 'igw_jpeg_encode_kernel' in b]
    assert len(kern) == 1
    val = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, kern[0]).group(1))  # noqa: E731
    print('igw_jpeg_encode_kernel: %d VGPRs, %d SGPRs, %d B of LDS' % (val('vgpr_count'), val('sgpr_count'),
                                                                         val('group_segment_fixed_size')))
    assert val('private_segment_fixed_size') == 0
    assert val('vgpr_spill_count') == 0 and val('sgpr_spill_count') == 0
    assert val('vgpr_count') <= 128                          # 256 threads: two workgroups per SIMD quartet and more
    assert val('group_segment_fixed_size') <= 40 * 1024      # four workgroups in a CU's 160 KiB
    assert not _forbidden(asm)
    assert 'ds_or_b32' in asm                                # the codes do go into the window with LDS atomics


def test_step_and_render_build_ids_are_the_ones_before_the_codec():
    from gridworld_amd import build as B, codec as K, render as R
    assert B.source_hash() == STEP_ID
    assert R.source_hash() == RENDER_ID
    theirs = {os.path.basename(s) for s in B.SOURCES + B.HEADERS + R.SOURCES + R.HEADERS}
    assert not theirs & {os.path.basename(s) for s in K.SOURCES + K.HEADERS}


def test_the_codec_argument_of_the_render_calls_is_checked_without_a_device():
    from gridworld_amd import codec as K
    assert K.check_codec(None) is None and K.check_codec('jpeg') == 'jpeg'
    with pytest.raises(ValueError):
        K.check_codec('png')
    with pytest.raises(ValueError):
        K.check_codec('jpeg', outputs=('rgb', 'depth'))
