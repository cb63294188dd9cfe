"""The HIP JPEG encoder (libigw_codec.so) against the numpy model of DESIGN.md section 9 (tests/jpeg_model.py): the
streams are equal byte for byte, and so are the sizes -- there is no tolerance.  Small batches: all of these together
are budgeted at a few seconds."""
import numpy as np
import pytest

import jpeg_model as J

pytestmark = pytest.mark.gpu
GUARD = 0xA5


def _same(frames, quality, jpegs, what):
    """Every stream equals the model's."""
    assert len(jpegs) == len(frames)
    bad = [k for k in range(len(frames)) if jpegs[k] != J.encode(frames[k], quality)]
    print(f'{what}: {len(frames)} frames at quality {quality}, {sum(len(j) for j in jpegs)} bytes, '
          f'{len(bad)} streams differ from the model')
    assert not bad, (what, bad[:8])


def _encode_guarded(frames, quality, stride=None):
    """(streams, buf, sizes) of encode_jpeg into a buffer pre-filled with GUARD; checks that nothing past sizes[i] was
    written."""
    import torch
    import gridworld_amd as G
    n, H, W = frames.shape[:3]
    stride = stride or G.codec.jpeg_bound(W, H)
    buf = torch.full((n, stride), GUARD, dtype=torch.uint8, device=frames.device)
    sizes = torch.full((n,), -7, dtype=torch.int32, device=frames.device)
    rb, rs = G.encode_jpeg(frames, quality, out=(buf, sizes))
    assert rb is buf and rs is sizes
    b, s = buf.cpu().numpy(), sizes.cpu().numpy()
    assert (s >= G.codec.HEADER_BYTES + 2).all() and (s <= stride).all()
    for i in range(n):
        assert (b[i, s[i]:] == GUARD).all(), i
    return [b[i, :s[i]].tobytes() for i in range(n)], buf, sizes


def _stepped(n, flying, T=60):
    from gridworld_amd import VecGridWorld, workloads
    kw = dict(action_space='flying') if flying else {}
    env = VecGridWorld(n, device='cuda:0', autoreset=True, size_reward=False, max_steps=40, **kw)
    env.set_tasks(workloads.rt20(n, seed=3).numpy())
    env.reset()
    if flying:
        rng = np.random.RandomState(5)
        for _ in range(T):
            env.step(dict(movement=rng.uniform(-1, 1, (n, 3)).astype(np.float32),
                          camera=rng.uniform(-5, 5, (n, 2)).astype(np.float32),
                          inventory=rng.randint(0, 7, n).astype(np.int32),
                          placement=rng.randint(0, 3, n).astype(np.int32)))
    else:
        acts = env.fill_actions(T, seed=7)
        for t in range(T):
            env.step(acts[t])
    return env


def test_pov_frames_of_stepped_walking_and_flying_batches_equal_the_model():
    import gridworld_amd as G
    for flying in (False, True):
        env = _stepped(256, flying)
        frames = env.render_pov()
        jpegs, _, _ = _encode_guarded(frames, 90, stride=G.codec.default_stride(64, 64))
        _same(frames.cpu().numpy(), 90, jpegs, 'flying pov' if flying else 'walking pov')
        # the render call with codec='jpeg' is the two launches in one call
        buf, sizes = env.render_pov(codec='jpeg', quality=90)
        assert G.jpeg_bytes(buf, sizes) == jpegs
        with pytest.raises(ValueError):
            env.render_pov(codec='jpeg', outputs=('depth',))
        with pytest.raises(ValueError):
            env.render_pov(codec='png')


def test_outside_eye_views_equal_the_model_at_three_qualities():
    import gridworld_amd as G
    env = _stepped(16, False, T=30)
    poses = G.orbit_poses((0, 1, 0), 9, 5, 16)
    frames = env.render_views(poses, size=(96, 40))
    assert tuple(frames.shape) == (16, 40, 96, 3)
    for q in (1, 50, 100):
        jpegs, _, _ = _encode_guarded(frames, q)
        _same(frames.cpu().numpy(), q, jpegs, 'views 96 x 40')
        buf, sizes = env.render_views(poses, size=(96, 40), codec='jpeg', quality=q)
        assert G.jpeg_bytes(buf, sizes) == jpegs
        buf, sizes = G.render_views(env.grid_buf, poses, size=(96, 40), atlas=env._atlas(), codec='jpeg', quality=q)
        assert G.jpeg_bytes(buf, sizes) == jpegs


def test_noise_odd_sizes_four_channels_and_a_many_chunk_frame_equal_the_model():
    import torch
    rng = np.random.RandomState(1)
    cases = [('noise 64 x 64', rng.randint(0, 256, (6, 64, 64, 3)), (1, 50, 100)),
             ('noise 96 x 40', rng.randint(0, 256, (3, 40, 96, 3)), (90,)),
             ('noise 13 x 7 rgba', rng.randint(0, 256, (4, 7, 13, 4)), (75,)),
             ('1 x 1', rng.randint(0, 256, (3, 1, 1, 3)), (90,)),
             ('extremes', np.stack([np.full((16, 24, 3), v, np.int64) for v in (0, 255)]
                                   + [np.tile(np.array(c), (16, 24, 1)) for c in ((255, 0, 0), (0, 0, 255), (0, 255, 0))]),
              (100,)),
             # 136 x 120: 255 MCUs, four chunks, the last one short; noise at quality 100 takes several windows a chunk
             ('noise 136 x 120', rng.randint(0, 256, (2, 120, 136, 3)), (100, 30))]
    yy, xx = np.mgrid[0:200, 0:328]
    cases.append(('smooth 328 x 200 rgba', np.stack([(xx * 3 + yy) % 256, (yy * 2) % 256, (xx + yy * yy // 64) % 256,
                                                     xx % 256], -1)[None], (90,)))
    for what, f, qualities in cases:
        f = np.ascontiguousarray(f.astype(np.uint8))
        d = torch.from_numpy(f).cuda()
        for q in qualities:
            jpegs, _, _ = _encode_guarded(d, q)
            _same(f, q, jpegs, what)


def test_a_small_stride_gives_negative_sizes_writes_nothing_past_it_and_the_wrapper_retries():
    import torch
    import gridworld_amd as G
    rng = np.random.RandomState(2)
    f = rng.randint(0, 256, (5, 64, 64, 3)).astype(np.uint8)
    f[1] = 90                                  # a flat frame: it fits where the noise does not
    f[3] = 200
    d = torch.from_numpy(f).cuda()
    want = [J.encode(x, 95) for x in f]
    stride = 2048
    assert len(want[1]) <= stride < len(want[0])
    # the slots sit inside a larger guarded buffer: frame i's slot is row i's first `stride` bytes of a [n, stride]
    # tensor followed by a guard row
    buf = torch.full((6, stride), GUARD, dtype=torch.uint8, device='cuda')
    sizes = torch.zeros(5, dtype=torch.int32, device='cuda')
    G.encode_jpeg(d, 95, out=(buf[:5], sizes), check_sizes=False)
    b, s = buf.cpu().numpy(), sizes.cpu().numpy()
    for i in range(5):
        if len(want[i]) <= stride:
            assert s[i] == len(want[i]) and b[i, :s[i]].tobytes() == want[i] and (b[i, s[i]:] == GUARD).all()
        else:
            assert s[i] == -len(want[i])
            assert b[i].tobytes() == want[i][:stride]          # the first `stride` bytes, and nothing past the slot
    assert (b[5] == GUARD).all()
    with pytest.raises(G.codec.CodecError):
        G.jpeg_bytes(buf[:5], sizes)
    with pytest.raises(G.codec.CodecError):
        G.encode_jpeg(d, 95, out=(buf[:5], sizes))              # a given buffer is not replaced: the wrapper raises
    # without `out` the wrapper encodes again with the room the streams asked for
    rb, rs = G.encode_jpeg(d, 95, stride=stride)
    assert rb.shape[1] >= max(len(w) for w in want) and G.jpeg_bytes(rb, rs) == want


def test_out_is_reused_in_place_on_a_side_stream_and_in_a_graph_replay():
    import torch
    import gridworld_amd as G
    rng = np.random.RandomState(3)
    a = torch.from_numpy(rng.randint(0, 256, (4, 64, 64, 3)).astype(np.uint8)).cuda()
    b = torch.from_numpy((rng.randint(0, 256, (4, 64, 64, 3)) // 8 * 8).astype(np.uint8)).cuda()
    stride = G.codec.jpeg_bound(64, 64)
    buf = torch.zeros((4, stride), dtype=torch.uint8, device='cuda')
    sizes = torch.zeros(4, dtype=torch.int32, device='cuda')
    ptr = buf.data_ptr()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for src in (a, b):
            rb, rs = G.encode_jpeg(src, 80, out=(buf, sizes), check_sizes=False)
            assert rb is buf and rs is sizes and buf.data_ptr() == ptr
            side.synchronize()
            _same(src.cpu().numpy(), 80, G.jpeg_bytes(buf, sizes), 'side stream')
    # a captured encode: replaying it encodes whatever the frame tensor holds then
    frames = a.clone()
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        G.encode_jpeg(frames, 80, out=(buf, sizes), check_sizes=False)     # warm: the library is loaded
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            G.encode_jpeg(frames, 80, out=(buf, sizes), check_sizes=False)
    torch.cuda.current_stream().wait_stream(side)
    frames.copy_(b)
    buf.zero_()
    graph.replay()
    torch.cuda.synchronize()
    _same(b.cpu().numpy(), 80, G.jpeg_bytes(buf, sizes), 'graph replay')
