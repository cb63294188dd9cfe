"""The HIP JPEG encoder on the frames of tests/value_cases.py: nearly every AC symbol of both Huffman tables, 26-bit
codes, ZRL chains of one to three, blocks without an EOB, every DC category in both signs, and scans that end, or whose
chunk ends, exactly on the 32,768-bit boundary of the bit window.  tests/test_value_cases_cpu.py pins what the frames
reach; here every stream and size equals the numpy model's (tests/jpeg_model.py) byte for byte, and nothing is written
past a stream's end.  The same frames run through the kernel's source on the host in tests/test_jpeg_kernel_host.py."""
import numpy as np
import pytest

import value_cases as V
from test_gpu_jpeg import GUARD, _encode_guarded

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', [b[0] for b in V.jpeg_batches()], ids=lambda s: s.replace(' ', '-'))
def test_streams_and_sizes_equal_the_model(name):
    import torch
    frames, quality = next((f, q) for what, f, q in V.jpeg_batches() if what == name)
    want = list(V.jpeg_streams(name))
    d = torch.from_numpy(frames.copy()).cuda()                       # (the cases are read-only arrays)
    jpegs, _, sizes = _encode_guarded(d, quality)                      # (checks that nothing lies past sizes[i])
    bad = [k for k in range(len(want)) if jpegs[k] != want[k]]
    print(f'{name}: {len(want)} frames at quality {quality}, {sum(map(len, want))} bytes, {len(bad)} streams differ')
    assert sizes.cpu().tolist() == [len(w) for w in want]
    assert not bad, (name, bad[:8])


@pytest.mark.parametrize('name', list(V.aligned()))
@pytest.mark.parametrize('short', [1, 5])
def test_a_stride_a_few_bytes_short_of_a_window_aligned_stream(name, short):
    """The stream does not fit by `short` bytes -- 1 cuts the EOI, 5 cuts into the last flush, which for the frame
    whose scan ends on the boundary is the flush of the full window: the size comes back negative, the slot holds the
    stream's first `stride` bytes, and nothing is written behind it (the slot is the first row of a guarded buffer)."""
    import torch
    import gridworld_amd as G
    frame, quality = V.aligned()[name]
    want = V.jpeg_streams(name)[0]
    stride = len(want) - short
    d = torch.from_numpy(frame[None].copy()).cuda()
    buf = torch.full((2, stride), GUARD, dtype=torch.uint8, device='cuda')
    sizes = torch.zeros(1, dtype=torch.int32, device='cuda')
    G.encode_jpeg(d, quality, out=(buf[:1], sizes), check_sizes=False)
    b = buf.cpu().numpy()
    assert int(sizes[0]) == -len(want)
    assert b[0].tobytes() == want[:stride] and (b[1] == GUARD).all()
    with pytest.raises(G.codec.CodecError):
        G.jpeg_bytes(buf[:1], sizes)
