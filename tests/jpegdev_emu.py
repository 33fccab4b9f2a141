"""The definition of the device JPEG encoder's output (csrc/jpeg_scan.hip, ops.jpeg_scan, output.jpeg_from_scan): a numpy
emulator, integers only, that the kernels equal byte for byte.  Nothing here imports the package.

Format: baseline sequential JFIF, 8 bit, three components, 4:4:4, ONE interleaved scan.  MCU = one 8x8 block each of Y, Cb, Cr, raster
order; H or W not a multiple of 8 is padded by replicating the last row / column (SOF0 carries the true size).  Restart interval Ri =
mcus_per_segment: a segment is Ri consecutive MCUs in raster order (it may span MCU rows), the last one is what is left; every segment starts
with DC predictors 0, its last byte is padded with 1-bits, inside it every FF is followed by a stuffed 00, and segments are separated by
FF D0+(k mod 8).  ``scan`` is that byte string, without the file headers and EOI; ``file`` adds them.

Arithmetic (every constant of it is below):
  * colour: Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16,
    Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16 (arithmetic shift), clamp to 0..255, minus 128;
  * DCT: M[k][n] = rint(8192 a_k cos((2n+1) k pi / 16)), a_0 = sqrt(1/8), a_k = sqrt(2/8): the table DCT_M below.  First over the columns
    T = (M X + 1024) >> 11, then over the rows F = T M^T (|T| <= 1449, |F| < 4.7e7: int32); F carries a scale of 2^15;
  * quantiser: sign(F) ((|F| + Q 2^14) // (Q 2^15)), Q from the Annex K tables scaled by libjpeg's quality rule (``tables``); AC values are
    clamped to +-1023 (the largest size the baseline AC codes have; no 8-bit input reaches it, the clamp keeps the code total);
  * zigzag order, DC difference against the previous MCU of the segment, (run, size) symbols with ZRL and EOB under the four FIXED Annex K
    Huffman tables, amplitude bits in one's-complement form for negatives.
"""
import struct

import numpy as np

KINDS = ("constant", "smooth", "noise", "smooth_noise", "checker")

DCT_M = np.array([
    [2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896],
    [4017, 3406, 2276, 799, -799, -2276, -3406, -4017],
    [3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784],
    [3406, -799, -4017, -2276, 2276, 4017, 799, -3406],
    [2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896],
    [2276, -4017, 799, 3406, -3406, -799, 4017, -2276],
    [1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567],
    [799, -2276, 3406, -4017, 4017, -3406, 2276, -799]], dtype=np.int64)

# zigzag position -> natural (row-major: vertical frequency x 8 + horizontal frequency) index
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# Annex K.1 / K.2, natural order
Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                    + [99] * 32)

# Annex K.3 - K.6: codes per length 1 .. 16, then the symbols in code order
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
    0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])

BLOCK_BYTES = 208          # (11 + 11 + 63 (16 + 10) + 7) // 8: every coefficient with the longest code and the longest amplitude


def dct_matrix():
    """DCT_M from its rule (the CPU test holds the table to it)."""
    k, n = np.arange(8)[:, None], np.arange(8)[None, :]
    a = np.where(k == 0, np.sqrt(1 / 8), np.sqrt(2 / 8))
    return np.rint(8192 * a * np.cos((2 * n + 1) * k * np.pi / 16)).astype(np.int64)


def tables(quality):
    """quality 1 .. 100 -> (luma, chroma) quantisation tables, natural order, int (libjpeg's jpeg_quality_scaling, baseline clamp 1 .. 255)."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError("quality must be in 1 .. 100")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * s + 50) // 100, 1, 255).astype(np.int64) for base in (Q_LUMA, Q_CHROMA))


def _huff(spec):
    """(counts per length, symbols) -> (code[256], length[256]); length 0: no code."""
    counts, syms = spec
    code, length = np.zeros(256, np.uint64), np.zeros(256, np.int64)
    c, k = 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            code[syms[k]], length[syms[k]] = c, l
            c, k = c + 1, k + 1
        c <<= 1
    return code, length


_DC = (_huff(DC_LUMA), _huff(DC_CHROMA))
_AC = (_huff(AC_LUMA), _huff(AC_CHROMA))


def geometry(H, W, mcus_per_segment):
    """-> (MCU rows, MCU columns, segments)."""
    my, mx = (H + 7) // 8, (W + 7) // 8
    return my, mx, (my * mx + mcus_per_segment - 1) // mcus_per_segment


def capacity(H, W, mcus_per_segment):
    """Worst-case bytes of a frame's scan: 3 x 208 bytes per MCU, every byte stuffed, and the markers between the segments."""
    my, mx, nseg = geometry(H, W, mcus_per_segment)
    return my * mx * 3 * BLOCK_BYTES * 2 + 2 * (nseg - 1)


def ycc(img):
    """(H,W,3) uint8 RGB -> (3,H,W) int64 in -128 .. 127."""
    r, g, b = (img[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return np.clip(np.stack([y, cb, cr]), 0, 255) - 128


def coefficients(img, qt):
    """-> (MCUs in raster order, 3, 64) quantised coefficients in zigzag order."""
    H, W, _ = img.shape
    my, mx = (H + 7) // 8, (W + 7) // 8
    pad = np.pad(img, ((0, 8 * my - H), (0, 8 * mx - W), (0, 0)), mode="edge")
    x = ycc(pad).reshape(3, my, 8, mx, 8).transpose(1, 3, 0, 2, 4)                 # (my, mx, 3, row, column)
    t = (np.einsum("kn,abcnx->abckx", DCT_M, x) + 1024) >> 11
    f = np.einsum("abckx,lx->abckl", t, DCT_M)
    assert np.abs(t).max() <= 1449 and np.abs(f).max() < 47000000
    q = np.stack([qt[0], qt[1], qt[1]]).reshape(1, 1, 3, 8, 8)
    v = np.sign(f) * ((np.abs(f) + (q << 14)) // (q << 15))
    v = v.reshape(my * mx, 3, 64)[:, :, ZIGZAG]
    v[:, :, 1:] = np.clip(v[:, :, 1:], -1023, 1023)
    return v


def _size(a):
    """bits of |a| (0 for 0)."""
    a = np.abs(a)
    s = np.zeros(a.shape, np.int64)
    for k in range(12):
        s += a >= (1 << k)
    return s


def _tokens(coef, ri):
    """-> (value uint64, bits int64) per (MCU, component, zigzag position): the code(s) and amplitude of that position, bits 0 where nothing
    is coded; position 64 holds the block's EOB."""
    n = coef.shape[0]
    val, nb = np.zeros((n, 3, 65), np.uint64), np.zeros((n, 3, 65), np.int64)
    first = (np.arange(n) % ri) == 0
    for c in range(3):
        tc = 0 if c == 0 else 1
        dc = coef[:, c, 0]
        prev = np.concatenate([[0], dc[:-1]])
        prev[first] = 0
        d = dc - prev
        s = _size(d)
        amp = np.where(d < 0, d - 1, d) & ((1 << s) - 1)
        code, length = _DC[tc]
        val[:, c, 0] = (code[s] << s.astype(np.uint64)) | amp.astype(np.uint64)
        nb[:, c, 0] = length[s] + s
        code, length = _AC[tc]
        ac = coef[:, c, 1:]
        nz = ac != 0
        pos = np.broadcast_to(np.arange(1, 64), ac.shape)
        last = np.maximum.accumulate(np.where(nz, pos, 0), axis=1)                  # position of the latest non-zero up to here
        before = np.concatenate([np.zeros((n, 1), np.int64), last[:, :-1]], axis=1)
        run = pos - before - 1
        s = _size(ac)
        amp = (np.where(ac < 0, ac - 1, ac) & ((1 << s) - 1)).astype(np.uint64)
        sym = ((run % 16) << 4) | s
        v = (code[sym] << s.astype(np.uint64)) | amp
        b = length[sym] + s
        zrl_code, zrl_len = int(code[0xF0]), int(length[0xF0])
        for z in range(1, 4):                                                       # run <= 62: at most three ZRL in front
            m = nz & (run // 16 == z)
            pre = 0
            for _ in range(z):
                pre = (pre << zrl_len) | zrl_code
            v = np.where(m, (np.uint64(pre) << b.astype(np.uint64)) | v, v)
            b = np.where(m, b + z * zrl_len, b)
        val[:, c, 1:64] = np.where(nz, v, 0)
        nb[:, c, 1:64] = np.where(nz, b, 0)
        eob = last[:, -1] != 63
        val[:, c, 64] = np.where(eob, code[0], 0)
        nb[:, c, 64] = np.where(eob, length[0], 0)
    return val, nb


def segments(img, quality=90, mcus_per_segment=None, qt=None):
    """-> the list of the segments' bytes: padded with 1-bits, stuffed, without markers."""
    H, W, _ = img.shape
    ri = int(mcus_per_segment or (W + 7) // 8)
    qt = tables(quality) if qt is None else qt
    coef = coefficients(np.asarray(img), qt)
    n = coef.shape[0]
    nseg = (n + ri - 1) // ri
    val, nb = _tokens(coef, ri)
    val, nb = val.reshape(n, -1), nb.reshape(n, -1)
    seg_bits = np.add.reduceat(nb.sum(axis=1), np.arange(0, n, ri))
    padn = (-seg_bits) % 8
    # one token row per MCU, and behind each segment's last MCU the padding token
    val = np.concatenate([val, np.zeros((n, 1), np.uint64)], axis=1)
    nb = np.concatenate([nb, np.zeros((n, 1), np.int64)], axis=1)
    lastm = np.minimum(np.arange(nseg) * ri + ri, n) - 1
    val[lastm, -1] = ((1 << padn) - 1).astype(np.uint64)
    nb[lastm, -1] = padn
    val, nb = val.ravel(), nb.ravel()
    keep = nb > 0
    val, nb = val[keep], nb[keep]
    total = int(nb.sum())
    start = np.cumsum(nb) - nb
    tok = np.repeat(np.arange(nb.size), nb)
    j = np.arange(total) - start[tok]
    bits = ((val[tok] >> (nb[tok] - 1 - j).astype(np.uint64)) & np.uint64(1)).astype(np.uint8)
    data = np.packbits(bits).tobytes()
    ends = np.cumsum(seg_bits + padn) // 8
    out, a = [], 0
    for e in ends:
        out.append(data[a:int(e)].replace(b"\xff", b"\xff\x00"))
        a = int(e)
    return out


def scan(img, quality=90, mcus_per_segment=None, qt=None):
    """The entropy-coded scan of the frame with its restart markers: what ops.jpeg_scan returns for it."""
    segs = segments(img, quality, mcus_per_segment, qt)
    parts = []
    for k, s in enumerate(segs):
        if k:
            parts.append(bytes([0xFF, 0xD0 + (k - 1) % 8]))
        parts.append(s)
    return b"".join(parts)


def _marker(code, body):
    return struct.pack(">BBH", 0xFF, code, len(body) + 2) + body


def headers(W, H, qt, ri):
    """SOI, APP0 JFIF, two DQT, SOF0, four DHT, DRI, SOS."""
    out = [b"\xff\xd8", _marker(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")]
    for tq in range(2):
        out.append(_marker(0xDB, bytes([tq]) + bytes(int(v) for v in np.asarray(qt[tq])[ZIGZAG])))
    out.append(_marker(0xC0, struct.pack(">BHHB", 8, H, W, 3) + bytes([1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])))
    for tc_th, spec in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out.append(_marker(0xC4, bytes([tc_th]) + bytes(spec[0]) + bytes(spec[1])))
    out.append(_marker(0xDD, struct.pack(">H", ri)))
    out.append(_marker(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])))
    return b"".join(out)


def file(img, quality=90, mcus_per_segment=None):
    """The bytes of the JFIF file of the frame."""
    H, W, _ = img.shape
    ri = int(mcus_per_segment or (W + 7) // 8)
    qt = tables(quality)
    return headers(W, H, qt, ri) + scan(img, quality, ri, qt) + b"\xff\xd9"


def frame(kind, H, W, seed=0):
    """The test frames: (H,W,3) uint8."""
    rng = np.random.default_rng(1000 * H + W + seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    smooth = np.stack([(255 * xx) // max(W - 1, 1), (255 * yy) // max(H - 1, 1), (255 * (xx + yy)) // max(H + W - 2, 1)], axis=-1)
    if kind == "constant":
        img = np.empty((H, W, 3), np.int64)
        img[:] = (200, 30, 90)
    elif kind == "smooth":
        img = smooth
    elif kind == "noise":
        img = rng.integers(0, 256, (H, W, 3))
    elif kind == "smooth_noise":
        img = np.clip(smooth + rng.integers(-6, 7, (H, W, 3)), 0, 255)
    elif kind == "checker":
        img = np.repeat((((xx + yy) & 1) * 255)[..., None], 3, axis=-1)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(img.astype(np.uint8))
