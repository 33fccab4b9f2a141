"""The definition of the device JPEG encoder's 4:2:0 output (csrc/jpeg_scan.hip lwg_jpeg420_scan_u8, ops.jpeg_scan(subsampling="420"),
output.jpeg_from_scan(subsampling="420")): a numpy emulator, integers only, that the kernels equal byte for byte.  It imports
tests/jpegdev_emu.py - the definition of the 4:4:4 output - for every table and rule the two formats share; nothing here imports the package.

Format: baseline sequential JFIF, 8 bit, three components, ONE interleaved scan; SOF0 gives Y the sampling factors 2 x 2 (0x22) and Cb, Cr
1 x 1.  MCU = 16 x 16 pixels, raster order, ceil(W / 16) x ceil(H / 16) of them; H or W not a multiple of 16 is padded by replicating the last
row / column (SOF0 carries the true size).  An MCU holds six 8 x 8 blocks in this order: Y top-left, Y top-right, Y bottom-left, Y bottom-right,
Cb, Cr.  What differs from jpegdev_emu besides that:
  * colour: per pixel jpegdev_emu.ycc's three integer formulas, clamped to 0 .. 255; a chroma sample is (a + b + c + d + 2) >> 2 of the four
    CLAMPED values of its 2 x 2 pixel square (the rule of half-size cells in csrc/lwg_fuse_geom.h); then minus 128;
  * DC prediction: one predictor per component, following block order - the Y predictor runs through the four Y blocks of an MCU and on into
    the next MCU; all three are 0 at the start of every segment;
  * restart interval Ri = mcus_per_segment counted in 16 x 16 MCUs (default: one MCU row, ceil(W / 16));
  * capacity: nmcu x 6 x 208 x 2 + 2 (nseg - 1).
DCT, quantiser (+-1023 AC clamp), zigzag, the four fixed Annex K Huffman tables, ZRL / EOB, one's-complement amplitudes, 1-bit padding of a
segment's last byte, FF 00 stuffing and FF D0+(k mod 8) between segments are jpegdev_emu's, unchanged.
"""
import numpy as np

from tests import jpegdev_emu as emu

KINDS = emu.KINDS
BLOCKS = 6                 # blocks of an MCU
BLOCK_BYTES = emu.BLOCK_BYTES
tables = emu.tables
frame = emu.frame


def geometry(H, W, mcus_per_segment):
    """-> (MCU rows, MCU columns, segments)."""
    my, mx = (H + 15) // 16, (W + 15) // 16
    return my, mx, (my * mx + mcus_per_segment - 1) // mcus_per_segment


def capacity(H, W, mcus_per_segment):
    """Worst-case bytes of a frame's scan: 6 x 208 bytes per MCU, every byte stuffed, and the markers between the segments."""
    my, mx, nseg = geometry(H, W, mcus_per_segment)
    return my * mx * BLOCKS * BLOCK_BYTES * 2 + 2 * (nseg - 1)


def planes(img):
    """(H,W,3) uint8 RGB, H and W even -> (Y (H,W), Cb (H/2,W/2), Cr (H/2,W/2)) int64 in -128 .. 127."""
    full = emu.ycc(img) + 128                                                         # the clamped 0 .. 255 values
    H, W = full.shape[1:]
    sq = full[1:].reshape(2, H // 2, 2, W // 2, 2)
    c = (sq[:, :, 0, :, 0] + sq[:, :, 0, :, 1] + sq[:, :, 1, :, 0] + sq[:, :, 1, :, 1] + 2) >> 2
    return full[0] - 128, c[0] - 128, c[1] - 128


def coefficients(img, qt):
    """-> (MCUs in raster order, 6, 64) quantised coefficients in zigzag order; blocks Y00 Y01 Y10 Y11 Cb Cr."""
    H, W, _ = img.shape
    my, mx = (H + 15) // 16, (W + 15) // 16
    pad = np.pad(img, ((0, 16 * my - H), (0, 16 * mx - W), (0, 0)), mode="edge")
    y, cb, cr = planes(pad)
    yb = y.reshape(my, 2, 8, mx, 2, 8).transpose(0, 3, 1, 4, 2, 5).reshape(my, mx, 4, 8, 8)     # (my, mx, 2 by + bx, row, column)
    cc = [c.reshape(my, 8, mx, 8).transpose(0, 2, 1, 3)[:, :, None] for c in (cb, cr)]
    x = np.concatenate([yb] + cc, axis=2)                                                       # (my, mx, 6, row, column)
    t = (np.einsum("kn,abcnx->abckx", emu.DCT_M, x) + 1024) >> 11
    f = np.einsum("abckx,lx->abckl", t, emu.DCT_M)
    assert np.abs(t).max() <= 1449 and np.abs(f).max() < 47000000
    q = np.stack([qt[0]] * 4 + [qt[1]] * 2).reshape(1, 1, BLOCKS, 8, 8)
    v = np.sign(f) * ((np.abs(f) + (q << 14)) // (q << 15))
    v = v.reshape(my * mx, BLOCKS, 64)[:, :, emu.ZIGZAG]
    v[:, :, 1:] = np.clip(v[:, :, 1:], -1023, 1023)
    return v


def _tokens(coef, ri):
    """-> (value uint64, bits int64) per (MCU, block, zigzag position), position 64 the block's EOB: jpegdev_emu's tokens, called once for the
    Y blocks as ONE chain of 4 n blocks whose predictor restarts every 4 ri (component 0 of that call: luminance tables) and once for the
    chroma blocks (components 1 and 2: chrominance tables, predictor along the MCUs)."""
    n = coef.shape[0]
    chain = np.zeros((4 * n, 3, 64), np.int64)
    chain[:, 0] = coef[:, :4].reshape(4 * n, 64)
    yv, yb = emu._tokens(chain, 4 * ri)
    mcus = np.zeros((n, 3, 64), np.int64)
    mcus[:, 1:] = coef[:, 4:]
    cv, cb = emu._tokens(mcus, ri)
    val = np.concatenate([yv[:, 0].reshape(n, 4, 65), cv[:, 1:]], axis=1)
    nb = np.concatenate([yb[:, 0].reshape(n, 4, 65), cb[:, 1:]], axis=1)
    return val, nb


def segments(img, quality=90, mcus_per_segment=None, qt=None):
    """-> the list of the segments' bytes: padded with 1-bits, stuffed, without markers."""
    H, W, _ = img.shape
    ri = int(mcus_per_segment or (W + 15) // 16)
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
    """The entropy-coded scan of the frame with its restart markers: what ops.jpeg_scan(subsampling="420") returns for it."""
    parts = []
    for k, s in enumerate(segments(img, quality, mcus_per_segment, qt)):
        if k:
            parts.append(bytes([0xFF, 0xD0 + (k - 1) % 8]))
        parts.append(s)
    return b"".join(parts)


_SOF0 = 2 + 18 + 2 * 69    # SOI, APP0 and the two DQT segments in front of it


def headers(W, H, qt, ri):
    """jpegdev_emu.headers with ONE byte changed: the sampling factors of component 1 in SOF0, 0x22."""
    h = bytearray(emu.headers(W, H, qt, ri))
    at = _SOF0 + 11                                        # FF C0, length, precision, H, W, 3 components, component 1's id
    assert bytes(h[_SOF0:_SOF0 + 2]) == b"\xff\xc0" and h[at - 1] == 1 and h[at] == 0x11
    h[at] = 0x22
    return bytes(h)


def file(img, quality=90, mcus_per_segment=None):
    """The bytes of the JFIF file of the frame."""
    H, W, _ = img.shape
    ri = int(mcus_per_segment or (W + 15) // 16)
    qt = tables(quality)
    return headers(W, H, qt, ri) + scan(img, quality, ri, qt) + b"\xff\xd9"
