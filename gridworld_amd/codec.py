"""Frames to JPEG on the device and to Motion-JPEG video: builds and binds libigw_codec.so (include/igw_codec.h).

    import gridworld_amd as G
    buf, sizes = G.encode_jpeg(env.render_pov(), quality=90)     # device tensors, one launch on the current stream
    jpegs = G.jpeg_bytes(buf, sizes)                             # list of bytes: one D2H copy of the used prefixes
    G.codec.write_avi('episode.avi', jpegs, size=(64, 64), fps=20)

The encoder is a third, separate library: its sources and build id are its own, so the step and render libraries'
build ids (and the profiles stamped with them) are untouched by it.  The stream and its integer arithmetic are
DESIGN.md section 9; there is no CPU fallback: without a HIP device encode_jpeg raises.  The container (write_avi /
read_avi) is host code and needs nothing but Python.
"""
import ctypes as C
import os
import struct
import sys

import numpy as np

from . import build as _build

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc', 'codec')
LIB = os.path.join(HERE, 'libigw_codec.so')
SOURCES = [os.path.join(CSRC, 'igw_jpeg.hip')]
HEADERS = [os.path.join(HERE, '..', 'include', 'igw_codec.h')]
VERSION = 1
MAX_SIDE = 1024
HEADER_BYTES = 623
_vp, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64
# every symbol include/igw_codec.h declares: (result, arguments)
SIGNATURES = {
    'igw_codec_version': (C.c_int, []),
    'igw_codec_build_id': (C.c_char_p, []),
    'igw_codec_last_error': (C.c_char_p, []),
    'igw_jpeg_bound': (_i64, [_i32, _i32]),
    'igw_jpeg_encode': (C.c_int, [_vp, _i64, _i32, _i32, _i32, _i32, _vp, _i64, _vp, _vp]),
}
EXPORTS = list(SIGNATURES)
# the library as build.py builds it: the step library's FLAGS, an id of its own (igw_codec_build_id())
LIBRARY = _build.Library(LIB, SOURCES, HEADERS, 'igw-codec-build-id:', 'IGW_CODEC_BUILD_ID', deps=[__file__])
source_hash, built_id, is_stale = LIBRARY.source_hash, LIBRARY.built_id, LIBRARY.is_stale


class CodecError(RuntimeError):
    pass


def build(force=False, verbose=False):
    return LIBRARY.build(force, verbose=verbose)


BINDING = _build.Binding(LIBRARY, SIGNATURES, CodecError, 'igw_codec_last_error', 'igw_codec_build_id',
                         'gridworld_amd.codec', 'igw_jpeg_encode')
load, check, build_id = BINDING.load, BINDING.check, BINDING.build_id


def jpeg_bound(width, height):
    """A stride that holds the stream of any width x height frame (igw_jpeg_bound)."""
    b = load().igw_jpeg_bound(int(width), int(height))
    if b <= 0:
        raise ValueError(f'size must be within 1..{MAX_SIDE} each way, got {(width, height)}')
    return int(b)


def default_stride(width, height):
    """The slot encode_jpeg allocates per frame when it is not told: the header plus half the padded frame's RGB
    bytes, a multiple of 16.  Rendered frames need a fraction of it; a frame that needs more (noise at a high quality)
    is encoded again with the room it asked for."""
    wp, hp = (int(width) + 7) // 8 * 8, (int(height) + 7) // 8 * 8
    return min(jpeg_bound(width, height), (HEADER_BYTES + 2 + wp * hp * 3 // 2 + 15) // 16 * 16)


def encode_into(frames, n, width, height, channels, quality, out, stride, sizes, stream):
    """One igw_jpeg_encode call on raw pointers (ints)."""
    rc = load().igw_jpeg_encode(frames, int(n), int(width), int(height), int(channels), int(quality), out, int(stride),
                                sizes, stream)
    if rc:
        check(rc)


def encode_jpeg(frames, quality=90, out=None, stride=None, check_sizes=True):
    """JPEG streams of uint8 frames [n, H, W, 3 or 4] (a device tensor, e.g. what render_pov / render_views return; a
    fourth channel is ignored), one launch on the current stream.  Returns (buf uint8 [n, stride], sizes int32 [n]),
    device tensors: stream i is buf[i, :sizes[i]] (jpeg_bytes copies them out).

      quality      1..100: the Annex K tables scaled by the IJG rule
      out          (buf, sizes) to write into: contiguous tensors of those shapes on the frames' device; nothing is
                   allocated then, so the call can be captured in a graph (with check_sizes=False)
      stride       bytes per slot when `out` is None (default: default_stride)
      check_sizes  True: the sizes are read back (one small synchronising copy) and a frame whose stream did not fit is
                   dealt with: without `out` everything is encoded again into slots of the largest size asked for,
                   with `out` CodecError is raised.  False: nothing is read back; sizes[i] < 0 marks a stream that
                   needs -sizes[i] bytes, and its slot holds only the first `stride` of them.
    """
    import torch
    if not torch.is_tensor(frames) or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] not in (3, 4):
        raise ValueError('frames must be a uint8 tensor [n, H, W, 3 or 4]')
    n, H, W, ch = (int(s) for s in frames.shape)
    if not (1 <= W <= MAX_SIDE and 1 <= H <= MAX_SIDE):
        raise ValueError(f'frames must be within 1..{MAX_SIDE} each way, got {W} x {H}')
    if not 1 <= int(quality) <= 100:
        raise ValueError(f'quality must be in 1..100, got {quality}')
    if frames.device.type != 'cuda':
        raise CodecError('encode_jpeg needs frames on a HIP device (the codec has no CPU fallback)')
    dev = frames.device
    frames = frames.contiguous()
    given = out is not None
    if given:
        buf, sizes = out
        if (not torch.is_tensor(buf) or buf.dtype != torch.uint8 or buf.dim() != 2 or buf.shape[0] != n
                or not buf.is_contiguous() or buf.device != dev or buf.shape[1] < HEADER_BYTES + 2):
            raise ValueError(f'out[0] must be a contiguous uint8 tensor [{n}, stride >= {HEADER_BYTES + 2}] on {dev}')
        if (not torch.is_tensor(sizes) or sizes.dtype != torch.int32 or tuple(sizes.shape) != (n,)
                or not sizes.is_contiguous() or sizes.device != dev):
            raise ValueError(f'out[1] must be a contiguous int32 tensor [{n}] on {dev}')
    else:
        stride = default_stride(W, H) if stride is None else int(stride)
        if stride < HEADER_BYTES + 2:
            raise ValueError(f'stride must be >= {HEADER_BYTES + 2}, got {stride}')
        buf = torch.empty((n, stride), dtype=torch.uint8, device=dev)
        sizes = torch.empty((n,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        encode_into(frames.data_ptr(), n, W, H, ch, quality, buf.data_ptr(), buf.shape[1], sizes.data_ptr(), stream)
        if check_sizes and n:
            need = -int(sizes.min())
            if need > 0:
                if given:
                    raise CodecError(f'a stream needs {need} bytes but out has {buf.shape[1]} per frame '
                                     f'(jpeg_bound gives a stride that always fits)')
                buf = torch.empty((n, (need + 15) // 16 * 16), dtype=torch.uint8, device=dev)
                encode_into(frames.data_ptr(), n, W, H, ch, quality, buf.data_ptr(), buf.shape[1], sizes.data_ptr(),
                            stream)
    return buf, sizes


def check_codec(codec, outputs=None):
    """The `codec` argument of the render calls: None (raw frames) or 'jpeg' (ValueError otherwise, and with
    `outputs`: only the colour frame has a codec)."""
    if codec is None:
        return None
    if codec != 'jpeg':
        raise ValueError(f"codec must be None or 'jpeg', got {codec!r}")
    if outputs is None:
        return codec
    raise ValueError("codec='jpeg' encodes the colour frame: it cannot be combined with outputs=")


def encoded(codec, outputs, quality, out, draw):
    """The "draw, then encode" step of a render call that takes `codec`: None without a codec (the caller draws what
    it was asked for); with one, (buf, sizes) of the raw frames `draw()` returns, encoded by a second launch on the
    current stream into `out`, the (buf, sizes) pair to write into, or into fresh tensors that are grown to fit."""
    if not check_codec(codec, outputs):
        return None
    return encode_jpeg(draw(), quality, out=out, check_sizes=out is None)


def jpeg_bytes(buf, sizes):
    """The streams of encode_jpeg as a list of bytes: one device-side gather of the used prefixes and one copy to the
    host.  A negative size (a stream that did not fit) raises CodecError."""
    import torch
    n = int(sizes.shape[0])
    if n == 0:
        return []
    sz = sizes.to(torch.int64)
    if int(sz.min()) < 0:
        raise CodecError('a stream did not fit its slot (sizes < 0): encode it again with a larger stride')
    ends = torch.cumsum(sz, 0)
    cols = torch.arange(buf.shape[1], device=buf.device)
    packed = buf[cols[None, :] < sz[:, None]].cpu().numpy().tobytes()      # row-major: stream after stream
    ends = [0] + ends.cpu().tolist()
    return [packed[ends[i]:ends[i + 1]] for i in range(n)]


# ---- Motion-JPEG in AVI ---------------------------------------------------------------------------------------------
AVI_LIMIT = (1 << 31) - 1          # a RIFF chunk of 2 GiB or more needs OpenDML, which is not written here
AVIF_HASINDEX, AVIIF_KEYFRAME = 0x10, 0x10


def _chunk(fcc, data):
    return fcc + struct.pack('<I', len(data)) + data + (b'\0' if len(data) & 1 else b'')


def avi_size(lengths):
    """The size of the file write_avi writes for frames of these lengths."""
    movi = sum(8 + n + (n & 1) for n in lengths)
    return 12 + (12 + 64 + 12 + 64 + 48) + (12 + movi) + (8 + 16 * len(lengths))


def write_avi(path, jpeg_frames, size, fps=20):
    """Writes JPEG streams as a Motion-JPEG AVI: RIFF 'AVI ' { LIST hdrl { avih, LIST strl { strh vids/MJPG, strf
    BITMAPINFOHEADER } }, LIST movi { 00dc ... (even-padded) }, idx1 }.  size = (W, H) of the frames; fps is an integer
    or a (rate, scale) pair.  ValueError before anything is written if the file would reach 2 GiB.  Returns the path."""
    frames = list(jpeg_frames)
    W, H = int(size[0]), int(size[1])
    rate, scale = (int(fps[0]), int(fps[1])) if isinstance(fps, (tuple, list)) else (int(fps), 1)
    if rate < 1 or scale < 1 or rate != (fps[0] if isinstance(fps, (tuple, list)) else fps):
        raise ValueError(f'fps must be a positive integer or a (rate, scale) pair of them, got {fps!r}')
    total = avi_size([len(f) for f in frames])
    if total > AVI_LIMIT:
        raise ValueError(f'the video would take {total} bytes; an AVI without OpenDML extensions ends before 2 GiB: '
                         f'write fewer frames per file')
    frames = [bytes(f) for f in frames]
    n, biggest = len(frames), max([len(f) for f in frames], default=0)
    avih = struct.pack('<14I', scale * 1000000 // rate, biggest * rate // scale, 0, AVIF_HASINDEX, n, 0, 1, biggest,
                       W, H, 0, 0, 0, 0)
    strh = b'vids' + b'MJPG' + struct.pack('<IHHIIIIIIIIhhhh', 0, 0, 0, 0, scale, rate, 0, n, biggest, 0xffffffff, 0,
                                           0, 0, W, H)
    strf = struct.pack('<IiiHH4sIiiII', 40, W, H, 1, 24, b'MJPG', W * H * 3, 0, 0, 0, 0)
    strl = b'LIST' + struct.pack('<I', 4 + 8 + len(strh) + 8 + len(strf)) + b'strl' + _chunk(b'strh', strh) \
        + _chunk(b'strf', strf)
    hdrl = b'LIST' + struct.pack('<I', 4 + 8 + len(avih) + len(strl)) + b'hdrl' + _chunk(b'avih', avih) + strl
    movi_size = 4 + sum(8 + len(f) + (len(f) & 1) for f in frames)
    index, off = [], 4          # idx1 offsets count from the 'movi' fourcc
    for f in frames:
        index.append(struct.pack('<4sIII', b'00dc', AVIIF_KEYFRAME, off, len(f)))
        off += 8 + len(f) + (len(f) & 1)
    idx1 = _chunk(b'idx1', b''.join(index))
    assert 12 + len(hdrl) + 8 + movi_size + len(idx1) == total
    with open(path, 'wb') as fh:
        fh.write(b'RIFF' + struct.pack('<I', total - 8) + b'AVI ')
        fh.write(hdrl)
        fh.write(b'LIST' + struct.pack('<I', movi_size) + b'movi')
        for f in frames:
            fh.write(_chunk(b'00dc', f))
        fh.write(idx1)
    return path


def read_avi(path, info=False):
    """The frames of an AVI as write_avi writes it: a list of byte strings, in order (the 00dc chunks of its movi
    list).  info=True returns (frames, dict(size=(W, H), fps=rate / scale, frames=count in avih)) instead."""
    with open(path, 'rb') as fh:
        data = fh.read()
    if len(data) < 12 or data[:4] != b'RIFF' or data[8:12] != b'AVI ':
        raise ValueError(f'{path} is not a RIFF AVI file')
    frames, meta = [], {}

    def walk(lo, hi):
        while lo + 8 <= hi:
            fcc, n = data[lo:lo + 4], struct.unpack_from('<I', data, lo + 4)[0]
            body = lo + 8
            if body + n > hi:
                raise ValueError(f'{path}: chunk {fcc!r} at {lo} runs past its parent')
            if fcc == b'LIST':
                walk(body + 4, body + n)
            elif fcc == b'avih':
                v = struct.unpack_from('<14I', data, body)
                meta.update(frames=v[4], size=(v[8], v[9]))
            elif fcc == b'strh':
                scale, rate = struct.unpack_from('<II', data, body + 20)
                meta['fps'] = rate / scale
            elif fcc[2:] in (b'dc', b'db'):
                frames.append(data[body:body + n])
            lo = body + n + (n & 1)

    walk(12, min(len(data), 8 + struct.unpack_from('<I', data, 4)[0]))
    return (frames, meta) if info else frames


if __name__ == '__main__':
    print(build(force='--force' in sys.argv, verbose=True))
