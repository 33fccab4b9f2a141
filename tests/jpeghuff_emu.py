"""The definition of the device JPEG encoder's per-frame Huffman tables (csrc/jpeg_scan.hip lwg_jpeg_scan_opt_u8 / lwg_jpeg420_scan_opt_u8,
lwg_jpeg_hist_u8 / lwg_jpeg420_hist_u8, lwg_jpeg_huff_tables; ops.jpeg_scan(huffman="optimized")): a numpy emulator, integers
only, that the kernels equal bit for bit.  It imports tests/jpegdev_emu.py and tests/jpeg420_emu.py - the definitions of the two fixed-table
formats - for everything up to the quantised coefficients and for the bit packing, padding, stuffing and restart markers; nothing here imports
the package.

What is new: a frame is coded with four Huffman tables built from ITS OWN symbol counts, and its four DHT segments carry them.  The quantised
coefficients, and so the decoded pixels, are those of the fixed-table file.
  * ``histogram``: the symbols the scan codes, counted per table in DHT order - DC luminance, AC luminance, DC chrominance, AC chrominance:
    the size category of every DC difference (predictors 0 at every segment start; at 4:2:0 the Y predictor runs through the four Y blocks),
    and per AC run (run << 4) | size, 0xF0 once per ZRL, 0x00 per EOB.
  * ``table``: counts -> (codes per length 1 .. 16, symbols in code order), Annex K.2 as libjpeg 6b codes it (jchuff.c jpeg_gen_optimal_table),
    stated here so that it is defined on ties:
      1. 257 slots: the 256 counts, and slot 256 with count 1 - the reserved symbol that keeps any real code from being all 1-bits.
      2. Merge until it stops: c1 = the slot with the least non-zero count, among equal counts the LARGEST index; c2 the same among the other
         slots; no c2: stop.  count[c1] += count[c2], count[c2] = 0; every symbol of c1's set and of c2's set gets one more bit; c2's set
         joins c1's, which keeps index c1.  Sums are exact (no 32-bit wrap), so any uint32 counts are defined.
      3. Count the codes per length, then limit to 16 bits: for i from the largest length down to 17, while bits[i] > 0: j = the first length
         below i - 1 with bits[j] > 0; bits[i] -= 2, bits[i - 1] += 1, bits[j + 1] += 2, bits[j] -= 1.
      4. Take one code away from the longest non-empty length: the reserved symbol's.
      5. The symbols are the real symbols ordered by (length BEFORE step 3, symbol value), assigned to the limited counts in that order.
      6. All counts zero: the empty table - counts zero, no symbols (no frame produces it).
    Unlike libjpeg, lengths before step 3 above 32 work: they are at most 256.
  * ``capacity``: a DC code may now have 16 bits, so a block is at most (16 + 11 + 63 (16 + 10) + 7) // 8 = 209 bytes; the bound used for
    slots, capacity and bit buffers is the next multiple of 4, BLOCK_BYTES = 212.
  * ``dht`` / ``coder_words``: the two forms the device writes a frame's tables in - 4 x (16 counts + 256 symbol slots, unused ones 0) bytes,
    and the coder's 544 words code | length << 16 (DC luminance[16], DC chrominance[16], AC luminance[256], AC chrominance[256]; 0: no code).
"""
import contextlib

import numpy as np

from tests import jpeg420_emu as emu420
from tests import jpegdev_emu as emu

KINDS = emu.KINDS
BLOCK_BYTES = 212          # 209 = (16 + 11 + 63 (16 + 10) + 7) // 8 rounded up to whole words
frame = emu.frame
quant_tables = emu.tables
_FIXED_DHT_AT = 2 + 18 + 2 * 69 + 19       # SOI, APP0, two DQT and SOF0 in front of the four DHT segments
_FIXED_DHT_BYTES = 2 * (5 + 16 + 12) + 2 * (5 + 16 + 162)


def _format(subsampling):
    if subsampling not in ("444", "420"):
        raise ValueError("subsampling must be '444' or '420', not %r" % (subsampling,))
    return emu if subsampling == "444" else emu420


def _blocks(subsampling):
    return 3 if _format(subsampling) is emu else emu420.BLOCKS


def default_interval(W, subsampling="444"):
    side = 8 if _format(subsampling) is emu else 16
    return (W + side - 1) // side


def capacity(H, W, mcus_per_segment, subsampling="444"):
    """Worst-case bytes of a frame's scan: 212 bytes per block, every byte stuffed, and the markers between the segments."""
    my, mx, nseg = _format(subsampling).geometry(H, W, mcus_per_segment)
    return my * mx * _blocks(subsampling) * BLOCK_BYTES * 2 + 2 * (nseg - 1)


# ---- the symbols ----------------------------------------------------------------------------------------------------------------------------------
def _count(blocks, restart, dc, ac):
    """blocks (n, 64): ONE chain of blocks in coding order whose DC predictor is 0 at every ``restart``-th block; adds its symbols to the
    count arrays ``dc`` and ``ac``."""
    n = blocks.shape[0]
    d = blocks[:, 0] - np.concatenate([[0], blocks[:-1, 0]])
    first = (np.arange(n) % restart) == 0
    d[first] = blocks[first, 0]
    dc += np.bincount(emu._size(d), minlength=256)
    a = blocks[:, 1:]
    nz = a != 0
    pos = np.broadcast_to(np.arange(1, 64), a.shape)
    last = np.maximum.accumulate(np.where(nz, pos, 0), axis=1)
    before = np.concatenate([np.zeros((n, 1), np.int64), last[:, :-1]], axis=1)
    run = pos - before - 1
    ac += np.bincount((((run % 16) << 4) | emu._size(a))[nz], minlength=256)
    ac[0xF0] += int((run // 16)[nz].sum())
    ac[0x00] += int((last[:, -1] != 63).sum())


def histogram(img, quality=90, mcus_per_segment=None, subsampling="444", qt=None):
    """-> (4, 256) int64: how often the scan codes every symbol of DC luminance, AC luminance, DC chrominance, AC chrominance."""
    fmt = _format(subsampling)
    ri = int(mcus_per_segment or default_interval(img.shape[1], subsampling))
    coef = fmt.coefficients(np.asarray(img), quant_tables(quality) if qt is None else qt)
    n = coef.shape[0]
    h = np.zeros((4, 256), np.int64)
    if fmt is emu:
        _count(coef[:, 0], ri, h[0], h[1])
    else:
        _count(coef[:, :4].reshape(4 * n, 64), 4 * ri, h[0], h[1])
    for c in (-2, -1):
        _count(coef[:, c], ri, h[2], h[3])
    return h


# ---- the tables -----------------------------------------------------------------------------------------------------------------------------------
def _least(freq, skip):
    best, at = None, -1
    for i, v in enumerate(freq):
        if v and i != skip and (best is None or v <= best):
            best, at = v, i
    return at


def code_lengths(counts):
    """Steps 1 and 2: -> the 257 lengths before limiting (0: the symbol is not counted); slot 256 is the reserved symbol."""
    freq = [int(v) for v in counts] + [1]
    if len(freq) != 257 or min(freq) < 0:
        raise ValueError("a histogram is 256 counts >= 0")
    size, others = [0] * 257, [-1] * 257
    while True:
        c1 = _least(freq, -1)
        c2 = _least(freq, c1)
        if c2 < 0:
            return size
        freq[c1] += freq[c2]
        freq[c2] = 0
        size[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            size[c1] += 1
        others[c1] = c2
        size[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            size[c2] += 1


def limit_lengths(size):
    """Steps 3 and 4: the 257 lengths -> the codes per length 1 .. 16 of the real symbols."""
    bits = [0] * 258
    for s in size:
        if s:
            bits[s] += 1
    for i in range(257, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    for i in range(16, 0, -1):
        if bits[i]:
            bits[i] -= 1
            break
    assert not any(bits[17:]) and bits[0] == 0
    return bits[1:17]


def table(counts):
    """256 counts -> (codes per length 1 .. 16, symbols in code order)."""
    size = code_lengths(counts)
    symbols = sorted((s for s in range(256) if size[s]), key=lambda s: (size[s], s))
    if not symbols:
        return [0] * 16, []
    bits = limit_lengths(size)
    assert sum(bits) == len(symbols)
    return bits, symbols


def frame_tables(img, quality=90, mcus_per_segment=None, subsampling="444", qt=None):
    """-> the four (counts, symbols) of the frame, in DHT order."""
    return [table(h) for h in histogram(img, quality, mcus_per_segment, subsampling, qt)]


def dht(specs):
    """The four tables -> (4, 272) uint8: per table the 16 counts and 256 symbol slots, unused ones 0."""
    out = np.zeros((4, 272), np.uint8)
    for k, (bits, symbols) in enumerate(specs):
        out[k, :16] = bits
        out[k, 16:16 + len(symbols)] = symbols
    return out


def coder_words(specs):
    """The four tables -> (544,) uint32 code | length << 16 by symbol: DC luminance[16], DC chrominance[16], AC luminance[256], AC
    chrominance[256]; 0 where a symbol has no code.  Symbols >= 16 of a DC table have no place in this form."""
    words = []
    for k, n in ((0, 16), (2, 16), (1, 256), (3, 256)):
        code, length = emu._huff(specs[k])
        words.append((code.astype(np.uint32) | (length.astype(np.uint32) << np.uint32(16)))[:n])
    return np.concatenate(words)


# ---- the scan and the file ------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _coding_with(specs):
    """The two fixed-table emulators code with ``specs`` inside this block (their token rule reads the module's tables): everything behind the
    tables - amplitudes, ZRL / EOB, bit order, padding, stuffing - is theirs."""
    saved = emu._DC, emu._AC
    emu._DC = (emu._huff(specs[0]), emu._huff(specs[2]))
    emu._AC = (emu._huff(specs[1]), emu._huff(specs[3]))
    try:
        yield
    finally:
        emu._DC, emu._AC = saved


def scan(img, quality=90, mcus_per_segment=None, subsampling="444", qt=None, specs=None):
    """The entropy-coded scan of the frame under its own tables, with its restart markers: what ops.jpeg_scan(huffman="optimized") returns."""
    fmt = _format(subsampling)
    ri = int(mcus_per_segment or default_interval(img.shape[1], subsampling))
    qt = quant_tables(quality) if qt is None else qt
    specs = frame_tables(img, quality, ri, subsampling, qt) if specs is None else specs
    with _coding_with(specs):
        return fmt.scan(img, quality, ri, qt)


def headers(W, H, qt, ri, specs, subsampling="444"):
    """The fixed-table headers with the four DHT segments replaced by the frame's own."""
    h = _format(subsampling).headers(W, H, qt, ri)
    a, b = _FIXED_DHT_AT, _FIXED_DHT_AT + _FIXED_DHT_BYTES
    assert h[a:a + 2] == b"\xff\xc4" and h[b:b + 2] == b"\xff\xdd"
    own = b"".join(emu._marker(0xC4, bytes([tc_th]) + bytes(bits) + bytes(symbols))
                   for tc_th, (bits, symbols) in zip((0x00, 0x10, 0x01, 0x11), specs))
    return h[:a] + own + h[b:]


def file(img, quality=90, mcus_per_segment=None, subsampling="444"):
    """The bytes of the JFIF file of the frame."""
    H, W, _ = img.shape
    ri = int(mcus_per_segment or default_interval(W, subsampling))
    qt = quant_tables(quality)
    specs = frame_tables(img, quality, ri, subsampling, qt)
    return headers(W, H, qt, ri, specs, subsampling) + scan(img, quality, ri, subsampling, qt, specs) + b"\xff\xd9"
