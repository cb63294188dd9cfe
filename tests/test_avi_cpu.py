"""The Motion-JPEG AVI container of gridworld_amd/codec.py (write_avi / read_avi): pure Python, no device.  A RIFF walker
written here, independent of read_avi, checks the file's structure."""
import os
import struct

import numpy as np
import pytest

import jpeg_model as J
from gridworld_amd import codec as K


def _frames():
    rng = np.random.RandomState(4)
    fs = [J.encode(rng.randint(0, 256, (16, 24, 3)).astype(np.uint8), q) for q in (20, 50, 90, 35, 71)]
    fs.append(fs[0] + b'\0')                      # an odd and an even length are both among them
    assert {len(f) & 1 for f in fs} == {0, 1}
    return fs


def _walk(data, lo, hi, depth=0, out=None):
    """[(depth, fourcc, list type or None, offset of the chunk, size)] of the chunks in data[lo:hi]; checks that every
    chunk lies inside its parent and starts at an even offset."""
    out = [] if out is None else out
    while lo < hi:
        assert lo % 2 == 0 and lo + 8 <= hi
        fcc, n = data[lo:lo + 4], struct.unpack_from('<I', data, lo + 4)[0]
        assert lo + 8 + n <= hi, (fcc, lo, n, hi)
        if fcc in (b'RIFF', b'LIST'):
            out.append((depth, fcc, data[lo + 8:lo + 12], lo, n))
            _walk(data, lo + 12, lo + 8 + n, depth + 1, out)
        else:
            out.append((depth, fcc, None, lo, n))
        lo += 8 + n + (n & 1)
        if n & 1:
            assert data[lo - 1] == 0               # the pad byte
    assert lo == hi or lo == hi + (hi & 1)
    return out


def test_write_then_read_round_trips_the_streams(tmp_path):
    fs = _frames()
    p = str(tmp_path / 'a.avi')
    assert K.write_avi(p, fs, (24, 16), fps=20) == p
    assert K.read_avi(p) == fs
    got, meta = K.read_avi(p, info=True)
    assert got == fs and meta == dict(frames=len(fs), size=(24, 16), fps=20.0)
    assert os.path.getsize(p) == K.avi_size([len(f) for f in fs])
    # no frames at all is still a file that parses
    K.write_avi(p, [], (24, 16), fps=(30000, 1001))
    got, meta = K.read_avi(p, info=True)
    assert got == [] and meta['frames'] == 0 and abs(meta['fps'] - 29.97) < 0.01
    for bad in (0, -5, 29.97, (30, 0)):
        with pytest.raises(ValueError):
            K.write_avi(p, fs, (24, 16), fps=bad)
    with open(p, 'wb') as fh:
        fh.write(b'not an avi at all')
    with pytest.raises(ValueError):
        K.read_avi(p)


def test_the_riff_structure_chunk_by_chunk(tmp_path):
    fs = _frames()
    p = str(tmp_path / 'b.avi')
    K.write_avi(p, fs, (24, 16), fps=25)
    data = open(p, 'rb').read()
    chunks = _walk(data, 0, len(data))
    shape = [(d, f, t) for d, f, t, _, _ in chunks]
    assert shape == [(0, b'RIFF', b'AVI '), (1, b'LIST', b'hdrl'), (2, b'avih', None), (2, b'LIST', b'strl'),
                     (3, b'strh', None), (3, b'strf', None), (1, b'LIST', b'movi')] \
        + [(2, b'00dc', None)] * len(fs) + [(1, b'idx1', None)]
    by = {(f, t): (o, n) for _, f, t, o, n in chunks if f != b'00dc'}
    assert by[(b'RIFF', b'AVI ')] == (0, len(data) - 8)
    # avih: microseconds per frame, flags with HASINDEX, the frame count, one stream, the size
    o, n = by[(b'avih', None)]
    assert n == 56
    avih = struct.unpack_from('<14I', data, o + 8)
    assert avih[0] == 40000 and avih[3] & 0x10 and avih[4] == len(fs) and avih[6] == 1 and avih[8:10] == (24, 16)
    assert avih[7] >= max(len(f) for f in fs)
    # strh: vids / MJPG, scale and rate, the length in frames; strf: a BITMAPINFOHEADER with the MJPG compression
    o, n = by[(b'strh', None)]
    assert n == 56 and data[o + 8:o + 16] == b'vidsMJPG'
    scale, rate, start, length = struct.unpack_from('<4I', data, o + 8 + 20)
    assert (scale, rate, start, length) == (1, 25, 0, len(fs))
    assert struct.unpack_from('<4h', data, o + 8 + 48) == (0, 0, 24, 16)
    o, n = by[(b'strf', None)]
    assert n == 40
    size, w, h, planes, bits, comp = struct.unpack_from('<IiiHH4s', data, o + 8)
    assert (size, w, h, planes, bits, comp) == (40, 24, 16, 1, 24, b'MJPG')
    # movi: the frames in order, each chunk's size the stream's, odd ones padded; idx1: one entry per frame whose
    # offset (from the 'movi' fourcc) and length land on that chunk
    movi = by[(b'LIST', b'movi')][0] + 8
    frames = [(o, n) for _, f, _, o, n in chunks if f == b'00dc']
    assert [data[o + 8:o + 8 + n] for o, n in frames] == fs
    o, n = by[(b'idx1', None)]
    assert n == 16 * len(fs)
    for k, (fo, fn) in enumerate(frames):
        cid, flags, off, length = struct.unpack_from('<4sIII', data, o + 8 + 16 * k)
        assert cid == b'00dc' and flags & 0x10
        assert movi + off == fo and length == fn
        assert data[movi + off:movi + off + 4] == b'00dc'
        assert struct.unpack_from('<I', data, movi + off + 4)[0] == length


def test_the_two_gib_guard_raises_before_anything_is_written(tmp_path):
    class Big(bytes):
        """A frame that claims 300 MiB without holding them."""
        def __len__(self):
            return 300 << 20

    p = str(tmp_path / 'big.avi')
    assert K.avi_size([300 << 20] * 8) > K.AVI_LIMIT
    with pytest.raises(ValueError, match='2 GiB'):
        K.write_avi(p, [Big(b'x')] * 8, (64, 64), fps=20)
    assert not os.path.exists(p)
    # just below the limit the arithmetic lets it pass: the guard is on the file's size, not on the frame count
    assert K.avi_size([1000] * 1000) < K.AVI_LIMIT
