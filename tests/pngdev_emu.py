"""The DEFINITION of the device PNG encoder's zlib stream (csrc/png_deflate.hip, include/lwg_hip.h 'lwg_png_deflate_u8'), in numpy.
The kernel must equal ``stream()`` byte for byte; where the two disagree, this file is right.

Stream of one (H, W, 3) uint8 frame, ``rows`` rows per segment:

  78 01                                   zlib header
  per segment (rows r0 .. r0 + nr - 1, nr = min(rows, H - r0)); raw = its nr scanlines, each the byte 04 + the 3W Paeth residuals
  (bpp = 3; left / up / upper-left are 0 outside the IMAGE - a segment's first row is filtered against the image row above it),
  n = nr (1 + 3W) <= 65 535:
      dynamic form   BFINAL 0, BTYPE 2, HLIT 0 (257 codes), HDIST 0 (1 code), HCLEN 15 (19 lengths); the code-length code gives the symbols
                     0..15 four bits and 16..18 none (canonical: symbol l has the code l), so the header carries the 257 literal / length
                     code lengths and the one distance code length 0 as plain 4-bit numbers: 17 + 57 + 1 032 = 1 106 bits; then the n
                     literals, the end-of-block symbol, and an empty stored block that ends the segment on a byte: the bits 000, zero bits
                     up to the byte boundary, 00 00 FF FF.  Its size: dyn = ceil((1 106 + sum hist[s] len[s] + 3) / 8) + 4 bytes.
      stored form    taken if and only if dyn > n + 5:  00, n as two little-endian bytes, ~n likewise, the n raw bytes (n + 5 bytes).
  01 00 00 FF FF                          the final (empty, stored) block
  Adler-32 of all raw bytes, big-endian

so a frame takes at most H (1 + 3W) + 5 nseg + 11 bytes (``capacity``).

The literal / length code of a segment (``code_lengths``), integers only:
  * hist = the histogram of the raw bytes, symbol 256 (end of block) with count 1.  The used symbols are those with a count: at least two.
  * Huffman by the two-queue method: leaves ascending by (count, symbol); the two smallest roots are merged, on equal weight a leaf is taken
    before an internal node and an older internal node before a younger one.
  * lengths are limited to 15 as miniz does: num[l] = codes of depth l, depths above 15 counted at 15; while the Kraft total
    sum num[l] 2^(15 - l) exceeds 2^15: one code leaves length 15, one code of the longest non-empty length i < 15 moves to i + 1 and one more
    code is added at i + 1; the total drops by 1.
  * the symbols sorted by (count descending, symbol ascending) receive the lengths in ascending order (num[1] ones, num[2] twos, ...).
  * codes are canonical (RFC 1951 3.2.2) and sent most significant bit first, i.e. bit-reversed into the LSB-first bit stream.
The code is complete by construction (zlib rejects an incomplete literal / length code).
"""
import struct
import zlib

import numpy as np

MAXLEN = 15
HEADER_BITS = 1106
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
MAX_SEGMENT = 65535


# ------------------------------------------------------------------------------------------------ filter
def _paeth_pred(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def paeth_filter(img):
    """(H, W, 3) uint8 -> the raw scanlines (H, 1 + 3W) uint8: filter byte 4 + residuals."""
    img = np.ascontiguousarray(img)
    H, W, C = img.shape
    assert C == 3 and img.dtype == np.uint8
    x = img.reshape(H, 3 * W).astype(np.int32)
    a = np.zeros_like(x)
    b = np.zeros_like(x)
    c = np.zeros_like(x)
    a[:, 3:] = x[:, :-3]
    b[1:] = x[:-1]
    c[1:, 3:] = x[:-1, :-3]
    raw = np.empty((H, 1 + 3 * W), np.uint8)
    raw[:, 0] = 4
    raw[:, 1:] = ((x - _paeth_pred(a, b, c)) & 255).astype(np.uint8)
    return raw


def paeth_unfilter(res):
    """The inverse: residuals (H, 3W) uint8 (no filter bytes) -> the (H, W, 3) uint8 image whose Paeth residuals they are."""
    res = np.asarray(res, np.uint8)
    H, N = res.shape
    assert N % 3 == 0
    W = N // 3
    r = res.reshape(H, W, 3).astype(np.int32)
    img = np.zeros((H + 1, W + 1, 3), np.int32)          # row 0 / column 0: the zeros outside the image
    for y in range(H):
        up = img[y]
        cur = img[y + 1]
        for x in range(W):
            cur[x + 1] = (r[y, x] + _paeth_pred(cur[x], up[x + 1], up[x])) & 255
    return img[1:, 1:].astype(np.uint8)


# ------------------------------------------------------------------------------------------------ code construction
def huffman_depths(hist):
    """Unlimited Huffman depths by the two-queue method; hist: counts per symbol (0 = unused) -> depths (0 = unused)."""
    hist = [int(v) for v in hist]
    leaves = sorted((c, s) for s, c in enumerate(hist) if c > 0)
    m = len(leaves)
    assert m >= 2
    weight = [c for c, _ in leaves] + [0] * (m - 1)
    parent = [0] * (2 * m - 1)
    li, ii, nn = 0, m, m                                # next leaf, next unmerged internal node, next node to create
    for _ in range(m - 1):
        pick = []
        for _k in range(2):
            if li < m and (ii >= nn or weight[li] <= weight[ii]):
                pick.append(li)
                li += 1
            else:
                pick.append(ii)
                ii += 1
        weight[nn] = weight[pick[0]] + weight[pick[1]]
        parent[pick[0]] = parent[pick[1]] = nn
        nn += 1
    depth = [0] * (2 * m - 1)
    for node in range(2 * m - 3, -1, -1):
        depth[node] = depth[parent[node]] + 1
    out = [0] * len(hist)
    for k, (_, s) in enumerate(leaves):
        out[s] = depth[k]
    return out


def limit_counts(depths):
    """num[l] for l = 0..15 after the miniz rule (num[0] unused)."""
    num = [0] * (MAXLEN + 1)
    for d in depths:
        if d:
            num[min(d, MAXLEN)] += 1
    total = sum(num[l] << (MAXLEN - l) for l in range(1, MAXLEN + 1))
    while total > (1 << MAXLEN):
        num[MAXLEN] -= 1
        for i in range(MAXLEN - 1, 0, -1):
            if num[i]:
                num[i] -= 1
                num[i + 1] += 2
                break
        total -= 1
    return num


def code_lengths(hist):
    """hist: 257 counts (hist[256] = 1) -> the 257 code lengths."""
    hist = [int(v) for v in hist]
    num = limit_counts(huffman_depths(hist))
    order = sorted((s for s, c in enumerate(hist) if c > 0), key=lambda s: (-hist[s], s))
    out = [0] * len(hist)
    k = 0
    for l in range(1, MAXLEN + 1):
        for _ in range(num[l]):
            out[order[k]] = l
            k += 1
    assert k == len(order)
    return out


def canonical_codes(lengths):
    """RFC 1951 3.2.2 codes, bit-reversed (the value to OR into an LSB-first bit stream)."""
    bl = [0] * (MAXLEN + 2)
    for l in lengths:
        bl[l] += 1
    bl[0] = 0
    nxt = [0] * (MAXLEN + 2)
    code = 0
    for b in range(1, MAXLEN + 1):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    out = [0] * len(lengths)
    for s, l in enumerate(lengths):
        if l:
            c = nxt[l]
            nxt[l] += 1
            out[s] = int(format(c, "0%db" % l)[::-1], 2)
    return out


# ------------------------------------------------------------------------------------------------ bits
def _put(bits, pos, values, lens):
    """OR values[i] (lens[i] bits, LSB first) into the bit array at pos[i]."""
    values = np.asarray(values, np.int64)
    lens = np.asarray(lens, np.int64)
    pos = np.asarray(pos, np.int64)
    for k in range(int(lens.max()) if lens.size else 0):
        m = lens > k
        bits[pos[m] + k] |= ((values[m] >> k) & 1).astype(np.uint8)


def segment_hist(raw):
    hist = np.bincount(np.frombuffer(bytes(raw), np.uint8), minlength=257)
    hist[256] = 1
    return hist


def dynamic_size(hist, lengths):
    """Bytes of the dynamic form (with the empty stored block behind it)."""
    payload = int(sum(int(h) * l for h, l in zip(hist, lengths)))
    return (HEADER_BITS + payload + 3 + 7) // 8 + 4


def segment_dynamic(raw, lengths=None):
    """The dynamic form of one segment, whatever its size."""
    raw = np.frombuffer(bytes(raw), np.uint8)
    hist = segment_hist(raw)
    if lengths is None:
        lengths = code_lengths(hist)
    codes = canonical_codes(lengths)
    size = dynamic_size(hist, lengths)
    bits = np.zeros(size * 8, np.uint8)
    head_v = [0, 2, 0, 0, 15] + [0 if s >= 16 else 4 for s in CL_ORDER]
    head_l = [1, 2, 5, 5, 4] + [3] * 19
    _put(bits, np.cumsum([0] + head_l[:-1]), head_v, head_l)
    rev4 = [int(format(l, "04b")[::-1], 2) for l in range(16)]
    _put(bits, 74 + 4 * np.arange(258), [rev4[l] for l in lengths] + [rev4[0]], [4] * 258)
    L = np.asarray(lengths, np.int64)
    C = np.asarray(codes, np.int64)
    ll = L[raw]
    pos = HEADER_BITS + np.concatenate([[0], np.cumsum(ll)])
    _put(bits, pos[:-1], C[raw], ll)
    _put(bits, pos[-1:], [codes[256]], [lengths[256]])
    out = np.packbits(bits, bitorder="little")
    out[-2:] = 255
    return out.tobytes()


def segment_stored(raw):
    raw = bytes(raw)
    n = len(raw)
    return b"\x00" + struct.pack("<HH", n, n ^ 0xFFFF) + raw


def segment(raw):
    raw = bytes(raw)
    n = len(raw)
    assert 1 <= n <= MAX_SEGMENT
    hist = segment_hist(raw)
    lengths = code_lengths(hist)
    if dynamic_size(hist, lengths) > n + 5:
        return segment_stored(raw)
    return segment_dynamic(raw, lengths)


def is_stored(seg):
    return (seg[0] & 7) == 0


# ------------------------------------------------------------------------------------------------ streams
def segments_of(H, rows):
    return [(r0, min(rows, H - r0)) for r0 in range(0, H, rows)]


def capacity(H, W, rows):
    return H * (1 + 3 * W) + 5 * len(segments_of(H, rows)) + 11


def segment_list(raw, rows):
    """The segments' bytes, in order."""
    return [segment(raw[r0:r0 + nr].tobytes()) for r0, nr in segments_of(raw.shape[0], rows)]


def stream_of_raw(raw, rows):
    """raw: (H, 1 + 3W) uint8 scanlines (filter bytes included) -> the zlib stream."""
    H = raw.shape[0]
    assert min(rows, H) * raw.shape[1] <= MAX_SEGMENT
    z = bytearray(b"\x78\x01")
    for seg in segment_list(raw, rows):
        z += seg
    z += b"\x01\x00\x00\xff\xff" + struct.pack(">I", zlib.adler32(raw.tobytes()) & 0xFFFFFFFF)
    return bytes(z)


def stream(img, rows=16):
    """(H, W, 3) uint8 -> the zlib stream the device writes for it."""
    return stream_of_raw(paeth_filter(img), rows)


# ------------------------------------------------------------------------------------------------ test frames (shared by the CPU and GPU tests)
KINDS = ("constant", "smooth", "smooth_noise", "noise", "all256")
FIB_COUNTS = (1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584)      # 17 literals, 6 763 bytes; the end-of-block symbol is the other 1


def frame(kind, H, W, rows=16, seed=0):
    """An (H, W, 3) uint8 test frame.  'all256': every segment's residuals hold the 256 values equally often (to within one) - equal weights
    everywhere, so the code rests on the tie rules; 'noise': uniform noise (every segment stored)."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    if kind == "all256":
        res = np.empty((H, 3 * W), np.uint8)
        for r0, nr in segments_of(H, min(rows, H)):
            v = (np.arange(nr * 3 * W) % 256).astype(np.uint8)
            rng.shuffle(v)
            res[r0:r0 + nr] = v.reshape(nr, 3 * W)
        return paeth_unfilter(res)
    yy, xx = np.mgrid[0:H, 0:W] / float(max(H, W))
    smooth = np.stack([np.sin(6 * xx) * np.cos(4 * yy), xx * yy, np.cos(9 * xx + 3 * yy)], -1)
    x = {"constant": np.full_like(smooth, 0.25), "smooth": smooth, "smooth_noise": smooth + 0.02 * rng.standard_normal(smooth.shape),
         "noise": rng.uniform(-1, 1, smooth.shape)}[kind]
    return ((np.clip(x, -1, 1) + 1) / 2.0 * 255).astype(np.uint8)


def fib_residuals(count, fill, seed=0):
    """``count`` residual bytes whose histogram is FIB_COUNTS on the literals 3, 10, 17, ... and the rest ``fill`` - with the end-of-block
    symbol's 1 a Fibonacci chain 18 or 19 deep, which the limit has to cut to 15."""
    assert count >= sum(FIB_COUNTS)
    v = np.concatenate([np.full(c, 7 * i + 3, np.uint8) for i, c in enumerate(FIB_COUNTS)] + [np.full(count - sum(FIB_COUNTS), fill, np.uint8)])
    np.random.default_rng(seed).shuffle(v)
    return v


def fib_frame(H=64, W=160, rows=32, seed=0):
    """(64, 160, 3): segment 0 uniform-noise residuals (stored), segment 1 = the length-limit stream: the 6 763 Fibonacci bytes, every other
    residual the literal 4 (the filter byte's value)."""
    rng = np.random.default_rng(seed)
    res = rng.integers(0, 256, (H, 3 * W), dtype=np.uint8)
    res[rows:2 * rows] = fib_residuals(rows * 3 * W, 4, seed).reshape(rows, 3 * W)
    return paeth_unfilter(res)
