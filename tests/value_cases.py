"""The inputs, and their truth, of the value-coverage tests (tests/test_value_cases_cpu.py pins them on the CPU;
tests/test_gpu_obs_values.py, tests/test_gpu_jpeg_codes.py and tests/test_jpeg_kernel_host.py run them).  Nothing in
this file touches a device.

Observation side (igw_render_pov_obs; DESIGN.md section 8, "Training-layout observations"): an atlas whose tiles hold
every byte value, a batch of eyes that look straight down at it, a table of (scale, bias) rows that reach the rounding
ties, subnormals, infinities and signed zeros of the three float types, and expected(): the observation in numpy,
IEEE-754 with gradual underflow and overflow to +-inf, compared as raw bits.

JPEG side (igw_jpeg_encode): frames synthesised from single DCT coefficients so that nearly every
(run, size) symbol of both AC tables is written, checkerboards for every DC category, and frames whose scan ends, or
whose chunk ends, exactly on the 32,768-bit boundary of the encoder's bit window."""
import functools

import numpy as np

import jpeg_model as J
import pov_model as M

# ---- observation side ----------------------------------------------------------------------------------------------
ATLAS_SIDE, ATLAS_SEED = 128, 41
SIZES = ((64, 64), (65, 65))            # 4,096 pixels: lanes of four; 4,225: every pixel alone
MIN_TRIPLES = 2000
CORNERS = [(r, g, b) for r in (0, 255) for g in (0, 255) for b in (0, 255)]


def _tile(rng):
    """uint8 [32, 32, 3], row 0 the bottom texel row: the 256-texel grey ramp in rows 0..7, the eight corners of the
    RGB cube at the start of row 8, seeded pseudo-random texels for the rest."""
    t = rng.randint(0, 256, (32, 32, 3)).astype(np.uint8)
    t[:8] = np.arange(256, dtype=np.uint8).reshape(8, 32, 1)
    t[8, :8] = CORNERS
    return t


@functools.lru_cache(None)
def atlas():
    """uint8 [128, 128, 4] (row 0 = the top image row): the WHITE and GREY ground tiles and the six block tiles each a
    _tile() of their own; the unused upper half stays black."""
    rng = np.random.RandomState(ATLAS_SEED)
    a = np.zeros((ATLAS_SIDE, ATLAS_SIDE, 4), np.uint8)
    a[..., 3] = 255
    for tid in sorted(M.TILES):
        tx, ty = M.TILES[tid]
        tile = _tile(rng)
        for rowb in range(32):
            a[ATLAS_SIDE - 1 - (32 * ty + rowb), 32 * tx:32 * tx + 32, :3] = tile[rowb]
    a.setflags(write=False)
    return a


# (block id, cell x, cell z): one block of each of four colours on the floor level, well apart
BLOCKS = ((1, 2, 2), (3, 8, 2), (4, 2, 8), (6, 8, 8))
OFF = (0.0137, 0.0071, -0.0113)        # eyes off the integer lattice (tests/test_gpu_render.py)


@functools.lru_cache(None)
def scene():
    """(grid int8 [9, 11, 11], poses f64 [12, 5]): every env holds the same grid, four single blocks; the eyes look
    straight down (and three obliquely) at the white ground, the grey ground and the blocks' top faces from several
    heights.  From 0.5 above a surface a 90-degree frame of 64 pixels holds one whole tile at two pixels a texel."""
    grid = np.zeros((9, 11, 11), np.int8)
    for bid, cx, cz in BLOCKS:
        grid[0, cx, cz] = bid
    poses = []
    for x, z, h in ((0, 0, 0.5), (1, -1, 1.0), (-1, 1, 0.75), (8, 0, 0.5), (-8, 8, 1.0)):    # ground: y = -1.5
        poses.append((x, -1.5 + h, z, 0.0, -90.0))
    for (bid, cx, cz), h in zip(BLOCKS, (0.5, 0.5, 0.75, 1.0)):                               # a block's top: y = -0.5
        poses.append((cx - 5.0, -0.5 + h, cz - 5.0, 90.0, -90.0))
    poses += [(0.0, 0.0, 3.0, 20.0, -50.0), (-3.0, 0.5, -3.0, 135.0, -40.0), (7.0, 1.0, 7.0, -40.0, -35.0)]
    p = np.array(poses, np.float64)
    p[:, :3] += OFF
    return grid, p


@functools.lru_cache(None)
def models(size):
    """pov_model's result for every env of scene() with atlas() at size = (W, H)."""
    grid, poses = scene()
    return [M.render(p, grid, atlas(), size[0], size[1], 3) for p in poses]


def predicted(size):
    """(uint8 [n, H, W, 3], share): the frames the model draws, and the share of their pixels outside its boundary
    band."""
    res = models(size)
    return np.stack([r['image'] for r in res]), float(np.mean([M.clean(r).mean() for r in res]))


def luminance(frames):
    """int64 [...] Y of uint8 RGB [..., 3] (obs_model.luminance, in int64)."""
    f = np.asarray(frames).astype(np.int64)
    return (19595 * f[..., 0] + 38470 * f[..., 1] + 7471 * f[..., 2] + 32768) >> 16


def coverage(frames):
    """What a batch of uint8 frames [n, H, W, 3] holds: the values missing from each of R, G, B, the luminances
    missing, and the number of distinct RGB triples."""
    f = np.asarray(frames)[..., :3].reshape(-1, 3)
    missing = [sorted(set(range(256)) - set(np.unique(f[:, c]).tolist())) for c in range(3)]
    lum = sorted(set(range(256)) - set(np.unique(luminance(f)).tolist()))
    packed = f[:, 0].astype(np.int64) << 16 | f[:, 1].astype(np.int64) << 8 | f[:, 2]
    return dict(missing=missing, missing_luminance=lum, triples=len(np.unique(packed)))


def covered(frames):
    c = coverage(frames)
    return not any(c['missing']) and not c['missing_luminance'] and c['triples'] >= MIN_TRIPLES


# (scale, bias, what the row reaches): scale and bias are Python floats; the kernel, torch and numpy all round them to
# float32 first
ROWS = (
    (1 / 255, 0.0, 'the usual normalisation'),
    (2 / 255, -1.0, 'the usual normalisation'),
    (1.0, -128.0, 'the usual normalisation'),
    (1 / 3, -85 / 3, 'an inexact product'),
    (0.1, -12.75, 'an inexact product'),
    (-1.0, 0.0, 'negative values'),
    (1.0, -255.0, 'negative values'),
    (1.0, 2048.0, '128 exact f16 ties'),
    (1.0, 256.0, 'bf16 ties at spacing 2'),
    (257.0, 0.0, '65,535 rounds to f16 inf while 65,278 stays finite; 20 ties'),
    (65504 / 255, 0.0, 'the f16 maximum, no overflow'),
    (2.0 ** -24, 0.0, '255 f16 subnormals'),
    (2.0 ** -25, 0.0, '128 ties among f16 subnormals'),
    (2.0 ** -149, 0.0, '255 f32 subnormals'),
    (2.0 ** -140, -(2.0 ** -133), 'subnormal sums'),
    (3.3e38, 0.0, 'f32 overflows to inf for v >= 2'),
    (-3.3e38, 3.4e38, '-inf'),
    (-1.0, -0.0, 'v = 0 must give -0.0'),
)
DTYPES = ('float16', 'bfloat16', 'float32')
BITS = {'float16': np.uint16, 'bfloat16': np.uint16, 'float32': np.uint32}


def f32_table(scale, bias):
    """float32 [256]: np.float32(v) * np.float32(scale), then + np.float32(bias), each rounded once."""
    with np.errstate(over='ignore', under='ignore'):
        f = np.arange(256, dtype=np.float32) * np.float32(scale)
        return (f + np.float32(bias)).astype(np.float32)


def bf16_bits(f):
    """uint16 bits of float32 `f` rounded to nearest-even to bfloat16 (in uint64: the carry cannot wrap); a NaN is the
    quiet NaN 0x7fc0."""
    b = np.ascontiguousarray(f, np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + np.uint64(0x7fff) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)
    return np.where((b & np.uint64(0x7fffffff)) > np.uint64(0x7f800000), np.uint16(0x7fc0), r)


def table(dtype, scale, bias):
    """The raw bits [256] of the stored value of every byte in `dtype` (a name from DTYPES)."""
    f = f32_table(scale, bias)
    if dtype == 'float32':
        return f.view(np.uint32)
    if dtype == 'float16':
        with np.errstate(over='ignore', under='ignore'):
            return f.astype(np.float16).view(np.uint16)
    return bf16_bits(f)


def planes(frames_u8, gray):
    """uint8 [N, planes, H, W] as obs_model.planes."""
    f = np.asarray(frames_u8)
    if gray:
        return luminance(f)[:, None].astype(np.uint8)
    return np.ascontiguousarray(f[..., :3].transpose(0, 3, 1, 2))


def expected(frames_u8, spec):
    """The raw bits [N, K * planes, H, W] of a FILLED observation of uint8 frames [N, H, W, 3] in the layout `spec`
    (anything with dtype, gray, stack, scale and bias; dtype a torch dtype or its name): uint8 for uint8, uint16 for
    f16 / bf16, uint32 for f32.  Numpy only."""
    name = str(spec.dtype).replace('torch.', '')
    p = planes(frames_u8, spec.gray)
    new = p if name == 'uint8' else table(name, spec.scale, spec.bias)[p]
    return np.ascontiguousarray(np.tile(new, (1, spec.stack, 1, 1)))


def reaches(scale, bias):
    """Counts over the 256 values of a row, from the reference: ties of the f16 and of the bf16 rounding (the f32 value
    lies exactly halfway between two neighbours of the narrower type), subnormals, infinities and the largest finite
    value of f16, subnormals, infinities and negative zeros of f32, negative values and products that were rounded."""
    with np.errstate(all='ignore'):
        f = f32_table(scale, bias)
        b = f.view(np.uint32).astype(np.int64)
        finite = np.isfinite(f)
        d = np.abs(f.astype(np.float64))
        # the spacing of f16 at d: 2^-24 below 2^-14, else 2^(floor(log2 d) - 10); 65,520 is halfway to the 65,536 that
        # f16 does not have
        unit = np.ldexp(1.0, np.maximum(np.frexp(d)[1] - 1, -14) - 10)
        h = f.astype(np.float16)
        hb = h.view(np.uint16)
        product = np.arange(256, dtype=np.float32) * np.float32(scale)
        exact = np.arange(256, dtype=np.float64) * np.float64(np.float32(scale))
        return {'bf16_ties': int((finite & ((b & 0xffff) == 0x8000)).sum()),
                'f16_ties': int((finite & (d <= 65520.0) & (np.mod(d / unit, 1.0) == 0.5)).sum()),
                'f16_subnormals': int((((hb & 0x7c00) == 0) & ((hb & 0x3ff) != 0)).sum()),
                'f16_inf': int(np.isinf(h).sum()),
                'f16_max': int((np.abs(h.astype(np.float64)) == 65504.0).sum()),
                'f32_subnormals': int((((b & 0x7f800000) == 0) & ((b & 0x7fffff) != 0)).sum()),
                'f32_inf': int(np.isposinf(f).sum()),
                'f32_neg_inf': int(np.isneginf(f).sum()),
                'f32_neg_zero': int((b == 0x80000000).sum()),
                'negative': int((f < 0).sum()),
                'inexact_products': int((np.isfinite(product) & (product.astype(np.float64) != exact)).sum())}


# ---- JPEG side -----------------------------------------------------------------------------------------------------
QUALITIES = (100, 98, 95, 90, 75, 50)
FRAME_BLOCKS = 512                       # a synthesised frame: 64 wide, 8 blocks a row, 512 blocks, 64 x 512 pixels
WINDOW_BITS = 32768                      # the encoder's bit window (csrc/codec/igw_jpeg.hip: kWinBits)


def _idct_basis():
    c = np.array([np.sqrt(1 / 8)] + [0.5] * 7)
    return c[:, None] * np.cos((2 * np.arange(8)[None, :] + 1) * np.arange(8)[:, None] * np.pi / 16)   # [u, x]


def _blocks(quality):
    """uint8 [n, 8, 8, 3]: for each component, zigzag position k = 1..63, size s = 1..10 and sign, the block whose
    only coefficient is about 1.25 * 2^(s - 1) * q_k at k: the float inverse DCT, + 128, chroma through the inverse
    colour transform; a block with a pixel outside 0..255 is dropped."""
    B = _idct_basis()
    tabs = J.quant_tables(quality)
    out = []
    for comp in range(3):
        q = tabs[0 if comp == 0 else 1]
        for k in range(1, 64):
            v, u = divmod(int(J.ZIGZAG[k]), 8)
            wave = np.outer(B[v], B[u])                                 # [y, x]
            for s in range(1, 11):
                for sign in (1, -1):
                    plane = 128.0 + sign * 1.25 * 2 ** (s - 1) * float(q[8 * v + u]) * wave
                    y, cb, cr = (plane if comp == c else np.full((8, 8), 128.0) for c in range(3))
                    rgb = np.stack([y + 1.402 * (cr - 128), y - 0.344136 * (cb - 128) - 0.714136 * (cr - 128),
                                    y + 1.772 * (cb - 128)], -1)
                    rgb = np.round(rgb)
                    if rgb.min() >= 0 and rgb.max() <= 255:
                        out.append(rgb.astype(np.uint8))
    return np.stack(out)


@functools.lru_cache(None)
def synthesised(quality):
    """uint8 [n, 512, 64, 3]: the blocks of _blocks(quality) tiled 8 a row into frames of FRAME_BLOCKS blocks; the
    last frame is filled up with flat grey blocks."""
    b = _blocks(quality)
    n = -(-len(b) // FRAME_BLOCKS)
    full = np.full((n * FRAME_BLOCKS, 8, 8, 3), 128, np.uint8)
    full[:len(b)] = b
    f = full.reshape(n, FRAME_BLOCKS // 8, 8, 8, 8, 3).transpose(0, 1, 3, 2, 4, 5).reshape(n, FRAME_BLOCKS, 64, 3)
    f = np.ascontiguousarray(f)
    f.setflags(write=False)
    return f


CHECKER_PAIRS = (((0, 0, 0), (255, 255, 255)), ((0, 0, 255), (255, 255, 0)), ((255, 0, 0), (0, 255, 255)))
# DC levels (the quantised DC at quality 100, an eighth of the block's level-shifted sum) of the staircase's blocks:
# up to and back from 2^(c - 1) for c = 1..10, then 8 -> -1016 -> 8 for the two differences of category 11
STAIRS = [0] + [v for c in range(1, 11) for v in (1 << (c - 1), 0)] + [8, -1016, 8]


def _staircase():
    """uint8 [64, 64, 3]: 23 grey blocks whose Y has the DC levels of STAIRS, then 23 blocks of colours (g, g, b),
    whose Cb is 128 + (b - g + 1 >> 1), with the same levels of Cb; level m is the flat value 128 + (m >> 3) with the
    first 8 * (m & 7) pixels one higher.  The rest of the frame is grey."""
    blocks = np.full((64, 64, 3), 128, np.int64)
    for i, m in enumerate(STAIRS):
        d = np.full(64, m >> 3)
        d[:8 * (m & 7)] += 1
        blocks[i] = (128 + d)[:, None]
        g = np.clip(128 - d, 0, 255)
        blocks[len(STAIRS) + i] = np.stack([g, g, g + 2 * d], -1)
    assert blocks.min() >= 0 and blocks.max() <= 255
    return blocks.reshape(8, 8, 8, 8, 3).transpose(0, 2, 1, 3, 4).reshape(64, 64, 3).astype(np.uint8)


@functools.lru_cache(None)
def dc_frames():
    """uint8 [4, 64, 64, 3] for quality 100: 8 x 8-block checkerboards black / white, blue / yellow and red / cyan (the
    largest DC differences of Y, Cb and Cr), and the staircase, which walks the categories between."""
    yy, xx = np.mgrid[0:64, 0:64]
    odd = ((yy // 8 + xx // 8) % 2).astype(bool)
    f = np.stack([np.where(odd[..., None], np.array(b), np.array(a)) for a, b in CHECKER_PAIRS] + [_staircase()])
    f = f.astype(np.uint8)
    f.setflags(write=False)
    return f


def _seeded(seed):
    f = np.full((304, 512, 3), 128, np.uint8)
    f[:8, :8] = np.random.RandomState(seed).randint(0, 256, (8, 8, 3))
    return f


STRADDLE_SEED = 28                       # the first seed after 22 whose frame has no code boundary at bit 32,768


@functools.lru_cache(None)
def aligned():
    """name -> (frame uint8 [H, W, 3], quality).  'scan-ends-on-window': 2,340 MCUs, the scan is exactly 32,768 bits
    before stuffing -- the last chunk ends on the boundary with no padding.  'chunk-ends-on-window': 32,768 bits after
    chunk 36 of 38 -- the next chunk starts an empty window.  'code-straddles-window': the same kind of frame with
    another seed, a code of which begins before bit 32,768 and ends past it, in the window's slack words."""
    out = {'scan-ends-on-window': (np.full((360, 416, 3), 200, np.uint8), 50),
           'chunk-ends-on-window': (_seeded(22), 60),
           'code-straddles-window': (_seeded(STRADDLE_SEED), 60)}
    for f, _ in out.values():
        f.setflags(write=False)
    return out


def cumulative_bits(frame, quality):
    """int64 [codes]: the scan's length in bits after each code (before padding and stuffing)."""
    return np.cumsum(J.scan_bits(J.coefficients(frame, quality))[1])


def chunk_end_bits(frame, quality):
    """int64 [chunks]: the scan's length in bits after each chunk of 64 MCUs (the scan of the MCUs so far)."""
    coef = J.coefficients(frame, quality).reshape(-1, 3, 64)
    return np.array([int(J.scan_bits(coef[:m])[1].sum()) for m in list(range(64, len(coef), 64)) + [len(coef)]])


def count(coef):
    """What the scan of quantised coefficients [my, mx, 3, 64] (J.coefficients) writes: the set of (table, 'dc' or
    'ac', symbol) written, DC (table, category, sign) triples, the longest code of each table in bits, the number of
    blocks without an EOB, and the set of ZRL chain lengths (ZRLs in front of one coefficient)."""
    symbols, dc_signed, zrl = set(), set(), set()
    longest, no_eob = [0, 0], 0
    q = coef.reshape(-1, 3, 64)[:, :, J.ZIGZAG]
    pred = [0, 0, 0]
    for mcu in q:
        for comp in range(3):
            blk = mcu[comp]
            tab = 0 if comp == 0 else 1
            diff = int(blk[0]) - pred[comp]
            pred[comp] = int(blk[0])
            cat = abs(diff).bit_length()
            symbols.add((tab, 'dc', cat))
            dc_signed.add((tab, cat, (diff > 0) - (diff < 0)))
            longest[tab] = max(longest[tab], J.DC_CODES[tab][cat][1] + cat)
            nz = np.flatnonzero(blk[1:]) + 1
            prev = 0
            for k in nz.tolist():
                run = k - prev - 1
                prev = k
                if run >= 16:
                    symbols.add((tab, 'ac', 0xf0))
                    zrl.add(run >> 4)
                    longest[tab] = max(longest[tab], J.AC_CODES[tab][0xf0][1])
                size = abs(int(blk[k])).bit_length()
                sym = (run & 15) << 4 | size
                symbols.add((tab, 'ac', sym))
                longest[tab] = max(longest[tab], J.AC_CODES[tab][sym][1] + size)
            if prev < 63:
                symbols.add((tab, 'ac', 0))
            else:
                no_eob += 1
    return dict(symbols=symbols, dc_signed=dc_signed, longest=tuple(longest), no_eob=no_eob, zrl=zrl)


def merge(counts):
    out = dict(symbols=set(), dc_signed=set(), longest=(0, 0), no_eob=0, zrl=set())
    for c in counts:
        out['symbols'] |= c['symbols']
        out['dc_signed'] |= c['dc_signed']
        out['zrl'] |= c['zrl']
        out['longest'] = tuple(max(a, b) for a, b in zip(out['longest'], c['longest']))
        out['no_eob'] += c['no_eob']
    return out


def jpeg_batches():
    """[(name, frames uint8 [n, H, W, 3], quality)]: every JPEG frame of this file, as batches of one size and
    quality."""
    out = [(f'synthesised q{q}', synthesised(q), q) for q in QUALITIES]
    out.append(('dc frames', dc_frames(), 100))
    out += [(name, f[None], q) for name, (f, q) in aligned().items()]
    return out


@functools.lru_cache(None)
def jpeg_streams(name):
    """The model's streams (a tuple of bytes) of the batch `name` of jpeg_batches(); computed once a process."""
    for what, frames, q in jpeg_batches():
        if what == name:
            return tuple(J.encode(f, q) for f in frames)
    raise KeyError(name)
