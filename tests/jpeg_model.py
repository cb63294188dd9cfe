"""A numpy model of the baseline JPEG stream of DESIGN.md section 9 ("JPEG frames and MJPEG video"), written from that
section: integer colour conversion, integer 8 x 8 DCT, IJG-scaled Annex K quantisation tables, Annex K Huffman tables,
4:4:4, one scan, no restart markers.  encode(frame, quality) returns the bytes that igw_jpeg_encode must produce for the
frame, every one of them; the GPU tests compare against it and the CPU tests check it against libjpeg (PIL)."""
import numpy as np

# ---- Annex K -------------------------------------------------------------------------------------------------------
LUMA_Q = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                   14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                   49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
CHROMA_Q = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                     47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64)
DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]
AC_LUMA_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14,
    0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09,
    0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a,
    0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65,
    0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88,
    0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9,
    0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
    0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea,
    0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHROMA_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32,
    0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16,
    0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39,
    0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64,
    0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86,
    0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8,
    0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9,
    0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]

# zigzag position k -> natural index 8 * row + column
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13,
                   6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45,
                   38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# ---- section 9: the arithmetic -------------------------------------------------------------------------------------
# C[u][x] = round(8192 c(u) cos((2x + 1) u pi / 16)), c(0) = sqrt(1/8), c(u) = 1/2: written out, as in the section
DCT = np.array([[2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896],
                [4017, 3406, 2276, 799, -799, -2276, -3406, -4017],
                [3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784],
                [3406, -799, -4017, -2276, 2276, 4017, 799, -3406],
                [2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896],
                [2276, -4017, 799, 3406, -3406, -799, 4017, -2276],
                [1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567],
                [799, -2276, 3406, -4017, 4017, -3406, 2276, -799]], np.int64)


def quant_tables(quality):
    """(luma, chroma) int64 [64] in natural order: Annex K scaled by the IJG rule."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError('quality must be in 1..100')
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((t * scale + 50) // 100, 1, 255) for t in (LUMA_Q, CHROMA_Q))


def ycc(rgb):
    """int64 [H, W, 3] Y, Cb, Cr in 0..255 of uint8 RGB."""
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11058 * r - 21710 * g + 32768 * b + 32768 + (128 << 16)) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + 32768 + (128 << 16)) >> 16
    return np.stack([y, np.minimum(cb, 255), np.minimum(cr, 255)], -1)


def coefficients(frame, quality):
    """Quantised coefficients int64 [my, mx, 3, 64] (natural order) of a uint8 [H, W, 3 or 4] frame."""
    f = np.asarray(frame)
    H, W = f.shape[:2]
    Hp, Wp = (H + 7) // 8 * 8, (W + 7) // 8 * 8
    f = f[np.minimum(np.arange(Hp), H - 1)][:, np.minimum(np.arange(Wp), W - 1)]      # replicate the last row / column
    s = ycc(f[..., :3]) - 128
    s = s.reshape(Hp // 8, 8, Wp // 8, 8, 3).transpose(0, 2, 4, 1, 3)                  # [my, mx, comp, y, x]
    t = (np.einsum('ux,...yx->...yu', DCT, s) + (1 << 10)) >> 11                       # rows: t[y][u]
    F = (np.einsum('vy,...yu->...vu', DCT, t) + (1 << 14)) >> 15                       # columns: F[v][u]
    F = F.reshape(F.shape[:3] + (64,))
    ql, qc = quant_tables(quality)
    q = np.stack([ql, qc, qc])[None, None]
    return np.sign(F) * ((np.abs(F) + (q >> 1)) // q)


def _codes(bits, vals):
    """symbol -> (code, length) of a DHT table (the canonical assignment of Annex C)."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


DC_CODES = (_codes(DC_LUMA_BITS, DC_VALS), _codes(DC_CHROMA_BITS, DC_VALS))
AC_CODES = (_codes(AC_LUMA_BITS, AC_LUMA_VALS), _codes(AC_CHROMA_BITS, AC_CHROMA_VALS))


def _magnitude(v):
    """(category, extra bits) of a non-zero value or DC difference (F.1.2.1)."""
    cat = int(abs(v)).bit_length()
    return cat, (v if v >= 0 else v + (1 << cat) - 1)


def header(W, H, quality):
    ql, qc = quant_tables(quality)
    be16 = lambda v: bytes([v >> 8, v & 255])  # noqa: E731
    out = b'\xff\xd8' + b'\xff\xe0' + be16(16) + b'JFIF\0' + bytes([1, 1, 0]) + be16(1) + be16(1) + bytes([0, 0])
    for k, t in enumerate((ql, qc)):
        out += b'\xff\xdb' + be16(67) + bytes([k]) + bytes(int(t[z]) for z in ZIGZAG)
    out += b'\xff\xc0' + be16(17) + bytes([8]) + be16(H) + be16(W) + bytes([3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
    for tc_th, bits, vals in ((0x00, DC_LUMA_BITS, DC_VALS), (0x10, AC_LUMA_BITS, AC_LUMA_VALS),
                              (0x01, DC_CHROMA_BITS, DC_VALS), (0x11, AC_CHROMA_BITS, AC_CHROMA_VALS)):
        out += b'\xff\xc4' + be16(19 + len(vals)) + bytes([tc_th]) + bytes(bits) + bytes(vals)
    out += b'\xff\xda' + be16(12) + bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    return out


def scan_bits(coef):
    """(codes, lengths) of the scan of quantised coefficients [my, mx, 3, 64], in stream order."""
    codes, lens = [], []
    q = coef.reshape(-1, 3, 64)[:, :, ZIGZAG]
    pred = [0, 0, 0]
    for mcu in q.tolist():
        for comp, blk in enumerate(mcu):
            tab = 0 if comp == 0 else 1
            cat, extra = _magnitude(blk[0] - pred[comp]) if blk[0] != pred[comp] else (0, 0)
            pred[comp] = blk[0]
            c, n = DC_CODES[tab][cat]
            codes.append((c << cat) | extra)
            lens.append(n + cat)
            run = 0
            ac = AC_CODES[tab]
            last = max((k for k in range(1, 64) if blk[k]), default=0)
            for k in range(1, last + 1):
                v = blk[k]
                if v == 0:
                    run += 1
                    continue
                while run >= 16:
                    codes.append(ac[0xf0][0])
                    lens.append(ac[0xf0][1])
                    run -= 16
                cat, extra = _magnitude(v)
                c, n = ac[(run << 4) | cat]
                codes.append((c << cat) | extra)
                lens.append(n + cat)
                run = 0
            if last < 63:
                codes.append(ac[0][0])
                lens.append(ac[0][1])
    return np.array(codes, np.uint64), np.array(lens, np.int64)


def pack(codes, lens):
    """The scan's bytes: codes MSB first, the last byte padded with 1s, a 00 after every FF."""
    j = np.arange(32)[None, :]
    n = lens[:, None]
    bits = ((codes[:, None] >> np.maximum(n - 1 - j, 0).astype(np.uint64)) & np.uint64(1)).astype(np.uint8)[j < n]
    bits = np.concatenate([bits, np.ones(-len(bits) % 8, np.uint8)])
    by = np.packbits(bits)
    ff = np.flatnonzero(by == 255)
    return np.insert(by, ff + 1, 0).tobytes()


def encode(frame, quality=90):
    """The JPEG stream (bytes) of one uint8 [H, W, 3 or 4] frame; a fourth channel is ignored."""
    f = np.asarray(frame)
    if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] not in (3, 4):
        raise ValueError(f'a frame is uint8 [H, W, 3 or 4], got {f.dtype} {f.shape}')
    return header(f.shape[1], f.shape[0], quality) + pack(*scan_bits(coefficients(f, quality))) + b'\xff\xd9'


def scan_of(stream):
    """The entropy-coded bytes of a stream: between the SOS header and the EOI."""
    i = stream.index(b'\xff\xda')
    n = (stream[i + 2] << 8) | stream[i + 3]
    return stream[i + 2 + n:-2]
