"""The host side of a render call, checked without a device: render.launch (which entry is called, with which
pointers) on CPU tensors and a stand-in library that records its calls, and codec.encoded (the codec rule)."""
import ctypes

import pytest
import torch

KINDS = {   # kind -> (the wrapper's arguments in front of the atlas, frames)
    'pov': ((0x1000, 0x2000, 0x3000, 5), 5),
    'views': ((0x1000, 1104, 2, None, 0x2000, 4), 4),
    'episodes': ((0x1000, 40, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 2, 10), 7),
}
OUTPUTS = [None, ('rgb',), ('depth',), ('rgb', 'surface')]
W, H, CH, STREAM = 24, 16, 4, 0x77
CPU = torch.device('cpu')


class Recorder:
    """Stands in for the loaded library: every symbol is a function that records (name, arguments) and returns 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


@pytest.fixture
def lib(monkeypatch):
    from gridworld_amd import render as R
    rec = Recorder()
    monkeypatch.setattr(R.BINDING, 'lib', rec)
    return rec


def _launch(kind, outputs, out=None, dev=CPU):
    from gridworld_amd import render as R
    args, n = KINDS[kind]
    atlas = torch.zeros((16, 16, 4), dtype=torch.uint8)
    return R.launch(kind, args, n, (W, H), CH, outputs, out, atlas, dev, STREAM), atlas


@pytest.mark.parametrize('outputs', OUTPUTS, ids=str)
@pytest.mark.parametrize('kind', list(KINDS))
def test_none_reaches_the_plain_entry_and_every_tuple_the_aux_entry(lib, kind, outputs):
    from gridworld_amd import render as R
    head, n = KINDS[kind]
    res, atlas = _launch(kind, outputs)
    assert len(lib.calls) == 1
    name, args = lib.calls[0]
    frame = (n, W, H, CH) if kind == 'episodes' else (W, H, CH)
    assert len(args) == len(R.SIGNATURES[name][1])
    assert args[:len(head)] == head and args[len(head):len(head) + 2] == (atlas.data_ptr(), 16)
    rgb = args[len(head) + 2]
    assert args[len(head) + 3:len(head) + 3 + len(frame)] == frame and args[-1] == STREAM
    if outputs is None:
        assert name == 'igw_render_' + kind
        assert torch.is_tensor(res) and tuple(res.shape) == (n, H, W, CH) and res.dtype == torch.uint8
        assert rgb == res.data_ptr()
        return
    assert name == 'igw_render_' + kind + '_aux'
    assert isinstance(res, dict) and tuple(res) == outputs
    assert rgb == (res['rgb'].data_ptr() if 'rgb' in outputs else None)      # out is NULL when 'rgb' is absent
    if 'rgb' in outputs:
        assert tuple(res['rgb'].shape) == (n, H, W, CH) and res['rgb'].dtype == torch.uint8
    aux = args[-2]._obj         # what ctypes.byref() refers to
    assert isinstance(aux, R.Aux) and len(R.Aux._fields_) == 3
    for plane, _ in R.Aux._fields_:
        if plane in outputs:    # NULL exactly for the planes not asked for
            assert getattr(aux, plane) == res[plane].data_ptr()
            assert tuple(res[plane].shape) == (n, H, W) and res[plane].dtype == getattr(torch, R.PLANE_DTYPES[plane])
        else:
            assert getattr(aux, plane) is None


@pytest.mark.parametrize('kind', list(KINDS))
def test_given_targets_are_written_in_place(lib, kind):
    n = KINDS[kind][1]
    out = torch.empty((n, H, W, CH), dtype=torch.uint8)
    res, _ = _launch(kind, None, out)
    assert res is out and lib.calls[0][0] == 'igw_render_' + kind
    planes = {'surface': torch.empty((n, H, W), dtype=torch.int16), 'rgb': out}
    res, _ = _launch(kind, ('rgb', 'surface'), planes)
    assert res['rgb'] is out and res['surface'] is planes['surface']
    name, args = lib.calls[1]
    assert name == 'igw_render_' + kind + '_aux' and args[-2]._obj.surface == planes['surface'].data_ptr()
    assert args[-2]._obj.depth is None and args[-2]._obj.label is None


@pytest.mark.parametrize('kind', list(KINDS))
def test_a_wrong_out_raises_before_any_call(lib, kind):
    n = KINDS[kind][1]
    frame = lambda **kw: torch.empty(kw.pop('shape', (n, H, W, CH)), **{'dtype': torch.uint8, **kw})  # noqa: E731
    depth = lambda **kw: torch.empty(kw.pop('shape', (n, H, W)), **{'dtype': torch.float32, **kw})  # noqa: E731
    bad = [(None, frame(shape=(n, W, H, CH))), (None, frame(shape=(n, H, W, 3))), (None, frame(dtype=torch.int8)),
           (None, frame(device='meta')), (None, frame(shape=(n, H, 2 * W, CH))[:, :, ::2]), (None, {'rgb': frame()}),
           (None, 'frames'),
           (('rgb',), frame()), (('rgb',), {'depth': depth()}), (('rgb',), {'rgb': frame(), 'depth': depth()}),
           (('depth',), {}), (('depth',), {'depth': depth(shape=(n + 1, H, W))}),
           (('depth',), {'depth': depth(dtype=torch.float64)}), (('depth',), {'depth': depth(device='meta')}),
           (('rgb', 'surface'), {'rgb': frame(), 'surface': depth()}),
           (('rgb', 'surface'), {'rgb': frame(shape=(n, H, W, 3)), 'surface': depth(dtype=torch.int16)})]
    for outputs, out in bad:
        with pytest.raises(ValueError):
            _launch(kind, outputs, out)
    for size, channels, outputs in (((0, H), CH, None), ((W, 1025), CH, ('depth',)), ((W, H), 2, None),
                                    ((W, H), 5, ('rgb',)), ((W, H), CH, ('rgb', 'rgb')), ((W, H), CH, ('normals',))):
        from gridworld_amd import render as R
        with pytest.raises(ValueError):
            R.launch(kind, KINDS[kind][0], n, size, channels, outputs, None, torch.zeros((16, 16, 4), dtype=torch.uint8),
                     CPU, STREAM)
    assert lib.calls == []


def test_the_aux_signatures_are_the_plain_ones_with_one_pointer_in_front_of_the_stream():
    from gridworld_amd import render as R
    for kind in KINDS:
        res, args = R.SIGNATURES['igw_render_' + kind]
        assert R.SIGNATURES['igw_render_' + kind + '_aux'] == (res, args[:-1] + [ctypes.c_void_p, ctypes.c_void_p])
        assert args[-1] is ctypes.c_void_p
    assert len(R.SIGNATURES) == 9


# ---- the codec rule ---------------------------------------------------------------------------------------------------
def test_encoded_is_none_without_a_codec_and_draws_nothing():
    from gridworld_amd import codec as K
    drawn = []
    assert K.encoded(None, None, 90, None, lambda: drawn.append(1)) is None
    assert K.encoded(None, ('rgb', 'depth'), 90, None, lambda: drawn.append(1)) is None
    assert drawn == []


def test_encoded_refuses_outputs_and_unknown_codecs_before_drawing():
    from gridworld_amd import codec as K
    drawn = []
    for outputs in (('rgb',), ('depth',), ('rgb', 'surface')):
        with pytest.raises(ValueError, match='outputs'):
            K.encoded('jpeg', outputs, 90, None, lambda: drawn.append(1))
    for codec in ('png', 'JPEG', 1):
        with pytest.raises(ValueError, match='codec'):
            K.encoded(codec, None, 90, None, lambda: drawn.append(1))
    assert drawn == []


def test_encoded_hands_the_drawn_frames_to_the_encoder():
    """With a codec the frames `draw()` returns reach encode_jpeg (which, without a device, raises CodecError for CPU
    frames: the codec has no CPU fallback)."""
    from gridworld_amd import codec as K
    drawn = []

    def draw():
        drawn.append(1)
        return torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(K.CodecError):
        K.encoded('jpeg', None, 90, None, draw)
    assert drawn == [1]
