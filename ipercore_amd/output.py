"""Output stage of ``Imitator.inference`` (reference models/imitator.py:368-372 + cv_utils.save_cv2_img,
tools/utils/filesio/cv_utils.py:100-116), re-designed for a producer that emits hundreds of frames per second.

The reference converts and writes one frame at a time on the inference thread (``.cpu().numpy()``, fp32 3 MB
D2H, ``cv2.imwrite``): at the rates of the MI355X path that serialises everything behind one host core.  Here:

* the fp32 -> uint8 conversion (same numerics: ``uint8((x + 1) / 2.0 * 255)``, truncation) runs on the device
  (``lwg_frames_to_u8``), so the copy is 0.75 MB/frame;
* the D2H copy goes through a ring of pinned host buffers on a side stream, ordered after the producing kernels by
  an event, never blocking the compute stream;
* PNG encoding + file writes run on a pool of host threads (zlib releases the GIL); ``close()`` joins them.

``FrameWriter(encoder="device")`` (opt-in; ``opt.png_encoder`` of the runners) moves the encoder to the device as well: ``lwg_png_deflate_u8``
writes each frame's zlib stream (Paeth-filtered scanlines, one literal-only dynamic-Huffman block per 16 rows, include/lwg_hip.h), the streams
and their lengths take the pinned-copy path, and a host thread only adds the chunk framing and the CRC-32 (``png_from_stream``) and writes.
The files are larger or smaller than the host encoder's depending on content (no matches: at least one bit per byte); they decode to the same
pixels.

``FrameWriter(encoder="jpeg" | "mjpeg")`` (opt-in; ``opt.output_format`` of the runners) writes lossy frames instead: ``lwg_jpeg_scan_u8`` codes each
frame's baseline JPEG scan on the device (4:4:4, fixed Annex K Huffman tables, restart segments; include/lwg_hip.h), only the CODED bytes cross
PCIe (the lengths first, then - from the helper thread that waits for them - the used prefix of every frame's buffer), and a host thread puts
the constant headers in front (``jpeg_from_scan``).  ``"jpeg"`` writes ``"{prefix}{t:0>8}.jpg"`` files, ``"mjpeg"`` ONE Motion-JPEG AVI file
(``MjpegAviWriter``: the container is ``struct.pack`` on the host, no codec library).  ``subsampling="420"`` (opt-in; ``opt.jpeg_subsampling``)
codes 16 x 16 MCUs with the chroma at half resolution instead (``lwg_jpeg420_scan_u8``): about half the bytes and the format players expect, at
the price of chroma detail - nearly all of it on noise-like frames.  ``huffman="optimized"`` (opt-in; ``opt.jpeg_huffman``) codes every frame
with Huffman tables built on the device from its own symbol counts (``lwg_jpeg_scan_opt_u8``, ``lwg_jpeg420_scan_opt_u8``): the same decoded
pixels in fewer bytes, for two more launches per batch; the tables cross PCIe with the lengths and the worker writes them into the frame's DHT.

``FrameWriter(fuse=FuseSpec(panel, ...))`` (opt-in; ``opt.fuse_output`` of the runners) hands the encoders the reference's comparison canvas
instead of the bare frame: ``lwg_fuse_canvas_u8`` composes [source panel | pad | reference frame | pad | frame ...] (fuse_src_ref_multi_outputs,
tools/utils/multimedia/video.py:451-505) from the fp32 frames in the launch that would have converted them; everything behind that one step is
the same writer.  ``RefFrames`` feeds the reference frames (an array, or image paths decoded a bounded number of batches ahead).

File names are the reference's: ``"{prefix}{t:0>8}.png"`` (imitator.py:369).  Pixels on disk are RGB, exactly what
``cv2.imwrite`` stores for the BGR array the reference hands it.
"""
import functools
import os
import queue
import struct
import threading
import zlib

import numpy as np
import torch


_PNG_SIG = b"\x89PNG\r\n\x1a\n"


def _png_chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def png_bytes(hwc_u8, compress_level=1):
    """(H,W,3) uint8 RGB -> the bytes of an 8-bit truecolour PNG: every scanline with filter type 0, ONE zlib stream (zlib releases the
    GIL, so the writer threads run in parallel).  Twice as fast as PIL's encoder at the same level on noise-like frames (25 vs 50 ms
    per 512x512 frame and thread), 4x on smooth ones: no per-row filter search, no Image object."""
    a = np.ascontiguousarray(hwc_u8)
    h, w, c = a.shape
    assert c == 3 and a.dtype == np.uint8
    raw = np.empty((h, 1 + 3 * w), dtype=np.uint8)
    raw[:, 0] = 0
    raw[:, 1:] = a.reshape(h, 3 * w)
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)
    return _PNG_SIG + _png_chunk(b"IHDR", ihdr) + _png_chunk(b"IDAT", zlib.compress(raw, compress_level)) + _png_chunk(b"IEND", b"")


def png_from_stream(stream, w, h):
    """The zlib stream of an (h, w) 8-bit truecolour image's scanlines (``ops.png_deflate``: bytes, or a uint8 array) -> the bytes of the
    PNG file: signature, IHDR, ONE IDAT with that stream, IEND.  The host's share of the device encoder: a CRC-32 and the framing."""
    ihdr = struct.pack(">IIBBBBB", int(w), int(h), 8, 2, 0, 0, 0)
    return _PNG_SIG + _png_chunk(b"IHDR", ihdr) + _png_chunk(b"IDAT", bytes(stream)) + _png_chunk(b"IEND", b"")


def encode_png(path, hwc_u8, compress_level=1):
    with open(path, "wb") as fp:
        fp.write(png_bytes(hwc_u8, compress_level))
    return path


# ---- JPEG: the tables and the file around a device-coded scan (include/lwg_hip.h lwg_jpeg_scan_u8) ---------------------------------------------
# Annex K.1 / K.2 quantisation tables, natural (row-major) order
_JPEG_Q_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
_JPEG_Q_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
_JPEG_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
# Annex K.3 - K.6 Huffman tables as a DHT segment carries them: (class << 4 | id, codes per length 1 .. 16, symbols); the kernels hold the same
# lists (csrc/lwg_jpeg_code.h)
_JPEG_DHT = (
    (0x00, (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12))),
    (0x10, (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d), bytes.fromhex(
        "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a"
        "535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7"
        "c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")),
    (0x01, (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12))),
    (0x11, (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77), bytes.fromhex(
        "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748494a"
        "535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7"
        "c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")),
)


@functools.lru_cache(maxsize=None)
def jpeg_tables(quality):
    """quality 1 .. 100 -> (luminance, chrominance) quantisation tables, 64 ints each in natural order: the Annex K tables scaled by libjpeg's
    rule (``jpeg_quality_scaling``), clamped to the baseline range 1 .. 255."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError("jpeg quality must be in 1 .. 100, not %r" % (quality,))
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(tuple(min(255, max(1, (b * s + 50) // 100)) for b in base) for base in (_JPEG_Q_LUMA, _JPEG_Q_CHROMA))


def _jpeg_marker(code, body):
    return struct.pack(">BBH", 0xFF, code, len(body) + 2) + body


JPEG_SUBSAMPLINGS = ("444", "420")     # the device encoder's chroma formats; "444" is the default everywhere
_JPEG_Y_SAMPLING = {"444": 0x11, "420": 0x22}


def jpeg_check_subsampling(subsampling):
    if subsampling not in JPEG_SUBSAMPLINGS:
        raise ValueError("jpeg subsampling must be '444' or '420', not %r" % (subsampling,))
    return subsampling


JPEG_HUFFMAN = ("fixed", "optimized")  # the device encoder's Huffman tables: Annex K's, or per-frame ones; "fixed" is the default everywhere
_JPEG_TC_TH = (0x00, 0x10, 0x01, 0x11)  # the order of a frame's tables: DC luminance, AC luminance, DC chrominance, AC chrominance


def jpeg_check_huffman(huffman):
    if huffman not in JPEG_HUFFMAN:
        raise ValueError("jpeg huffman must be 'fixed' or 'optimized', not %r" % (huffman,))
    return huffman


@functools.lru_cache(maxsize=64)
def _jpeg_header_parts(w, h, quality, ri, subsampling):
    """-> (the bytes in front of the four DHT segments, the fixed DHT segments, the bytes behind them)."""
    if not (0 < w <= 65535 and 0 < h <= 65535 and 0 < ri <= 65535):
        raise ValueError("jpeg: sizes and the restart interval are 16-bit fields")
    y_sampling = _JPEG_Y_SAMPLING[jpeg_check_subsampling(subsampling)]
    out = [b"\xff\xd8", _jpeg_marker(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")]
    for tq, table in enumerate(jpeg_tables(quality)):
        out.append(_jpeg_marker(0xDB, bytes([tq]) + bytes(table[k] for k in _JPEG_ZIGZAG)))
    out.append(_jpeg_marker(0xC0, struct.pack(">BHHB", 8, h, w, 3) + bytes([1, y_sampling, 0, 2, 0x11, 1, 3, 0x11, 1])))
    dht = b"".join(_jpeg_marker(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals)) for tc_th, bits, vals in _JPEG_DHT)
    back = _jpeg_marker(0xDD, struct.pack(">H", ri)) + _jpeg_marker(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return b"".join(out), dht, back


def jpeg_headers(w, h, quality, mcus_per_segment, subsampling="444", tables=None):
    """Everything in front of the scan - SOI, APP0 JFIF, two DQT, SOF0 (8 bit, h x w, three components; Y 1x1, with ``subsampling="420"``
    2x2), four DHT, DRI, SOS: constant per (w, h, quality, restart interval, subsampling), built once.  ``tables``: the frame's own Huffman
    tables as ``ops.jpeg_scan(huffman="optimized")`` returns them - (4, 272) uint8, per table 16 counts and 256 symbol slots - go into the
    four DHT segments instead of the Annex K ones."""
    front, dht, back = _jpeg_header_parts(int(w), int(h), quality, int(mcus_per_segment), subsampling)
    if tables is not None:
        t = np.asarray(tables)
        if t.dtype != np.uint8 or t.shape != (4, 272):
            raise ValueError("jpeg: a frame's tables are (4, 272) uint8")
        dht = b"".join(_jpeg_marker(0xC4, bytes([tc_th]) + row[:16 + int(row[:16].sum(dtype=np.int64))].tobytes()) for tc_th, row in zip(_JPEG_TC_TH, t))
    return front + dht + back


def jpeg_from_scan(scan, w, h, quality, mcus_per_segment, subsampling="444", tables=None):
    """The entropy-coded scan of a (h, w) frame (``ops.jpeg_scan`` with the same ``subsampling``: bytes, or a uint8 array) -> the bytes of the
    JFIF file: the headers, the scan, EOI.  The host's share of the device encoder: one concatenation.  ``tables``: as for ``jpeg_headers``."""
    return jpeg_headers(int(w), int(h), int(quality), int(mcus_per_segment), subsampling, tables) + bytes(scan) + b"\xff\xd9"


class MjpegAviWriter(object):
    """ONE RIFF AVI file of JPEG frames (Motion-JPEG): ``hdrl`` (``avih``, one ``strl``: ``strh`` vids / MJPG, ``strf`` BITMAPINFOHEADER), a
    ``movi`` list of ``00dc`` chunks - each a complete JFIF frame, padded to even length - and ``idx1``.  ``add(index, data)`` may be called
    from any thread in any order: one writer thread with a reorder buffer writes the frames in index order (0, 1, ...).  ``close()`` writes the
    index, patches the sizes and frame counts and returns ``[path]``.  AVI 1.0 sizes are 32 bits: an error is raised before the file would
    exceed ``MAX_BYTES`` (OpenDML is not written)."""

    MAX_BYTES = 2 ** 31 - 1
    _HDRL = 4 + (8 + 56) + (12 + (8 + 56) + (8 + 40))          # bytes of the hdrl list's data
    _MOVI = 12 + 8 + _HDRL                                      # file offset of the movi LIST chunk

    def __init__(self, path, w, h, fps=25):
        self.path, self.w, self.h, self.fps = path, int(w), int(h), float(fps)
        if self.w <= 0 or self.h <= 0 or not self.fps > 0:
            raise ValueError("MjpegAviWriter: width, height and fps must be positive")
        self._fp = open(path, "wb")
        self._fp.write(self._header(0, 0, 0, 0))
        self._pos = self._MOVI + 12
        self._index = []               # (offset from the 'movi' fourcc, bytes) per frame
        self._largest = 0
        self._pending = {}
        self._next = 0
        self._closing = False
        self._error = None
        self._cv = threading.Condition()
        self._thread = threading.Thread(target=self._run, daemon=True)
        self._thread.start()

    def _header(self, frames, movi_bytes, riff_bytes, largest):
        usec = int(round(1e6 / self.fps))
        rate, scale = int(round(self.fps * 1000)), 1000
        avih = struct.pack("<14I", usec, 0, 0, 0x10, frames, 0, 1, largest, self.w, self.h, 0, 0, 0, 0)           # 0x10: AVIF_HASINDEX
        strh = struct.pack("<4s4sIHHIIIIIIIIhhhh", b"vids", b"MJPG", 0, 0, 0, 0, scale, rate, 0, frames, largest, 0xFFFFFFFF, 0, 0, 0, self.w, self.h)
        strf = struct.pack("<IiiHH4sIiiII", 40, self.w, self.h, 1, 24, b"MJPG", self.w * self.h * 3, 0, 0, 0, 0)
        strl = b"LIST" + struct.pack("<I", 4 + 8 + len(strh) + 8 + len(strf)) + b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh \
            + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"LIST" + struct.pack("<I", 4 + 8 + len(avih) + len(strl)) + b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + strl
        assert len(hdrl) == 8 + self._HDRL
        return b"RIFF" + struct.pack("<I", riff_bytes) + b"AVI " + hdrl + b"LIST" + struct.pack("<I", movi_bytes) + b"movi"

    def _run(self):
        try:
            while True:
                with self._cv:
                    while self._next not in self._pending and not self._closing:
                        self._cv.wait()
                    if self._next not in self._pending:
                        return
                    data = self._pending.pop(self._next)
                pad = len(data) & 1
                # what the file would come to with this frame, its index entry and the index chunk's header
                if self._pos + 8 + len(data) + pad + 8 + 16 * (len(self._index) + 1) > self.MAX_BYTES:
                    raise RuntimeError("MjpegAviWriter: %s would exceed %d bytes with frame %d (AVI 1.0 sizes are 32 bits; OpenDML is not written)"
                                       % (self.path, self.MAX_BYTES, self._next))
                self._fp.write(b"00dc" + struct.pack("<I", len(data)) + data + b"\x00" * pad)
                self._index.append((self._pos - (self._MOVI + 8), len(data)))
                self._largest = max(self._largest, len(data))
                self._pos += 8 + len(data) + pad
                with self._cv:
                    self._next += 1
        except Exception as e:
            with self._cv:
                self._error = e
                self._pending.clear()

    def add(self, index, data):
        """Frame ``index`` (0-based, every index once) = the bytes of a complete JPEG file."""
        with self._cv:
            if self._error is not None:
                raise self._error
            if self._closing:
                raise RuntimeError("MjpegAviWriter: closed")
            if index < self._next or index in self._pending:
                raise ValueError("MjpegAviWriter: frame %d was already added" % index)
            self._pending[int(index)] = bytes(data)
            self._cv.notify_all()

    def close(self):
        with self._cv:
            self._closing = True
            self._cv.notify_all()
        self._thread.join()
        try:
            if self._error is not None:
                raise self._error
            if self._pending:
                raise RuntimeError("MjpegAviWriter: frame %d is missing (%d later frames were added)" % (self._next, len(self._pending)))
            n = len(self._index)
            self._fp.write(b"idx1" + struct.pack("<I", 16 * n) + b"".join(struct.pack("<4sIII", b"00dc", 0x10, o, s) for o, s in self._index))
            end = self._pos + 8 + 16 * n
            self._fp.seek(0)
            self._fp.write(self._header(n, self._pos - (self._MOVI + 8), end - 8, self._largest))
        finally:
            self._fp.close()
        return [self.path]


class FuseSpec(object):
    """What ``FrameWriter(fuse=...)`` composes around every frame: the source panel (``ops.fuse_source_panel``: (S,Wp,3) uint8 on the device),
    ``pad`` columns of ``pad_val`` between the regions, and whether a reference frame stands between the panel and the outputs (``with_ref``:
    every ``submit`` then needs ``ref``) - fuse_src_ref_multi_outputs' ``pad`` / ``pad_val`` and, without the reference, fuse_source_output."""

    def __init__(self, panel, pad=10, pad_val=0, with_ref=True):
        self.panel, self.pad, self.pad_val, self.with_ref = panel, int(pad), int(pad_val), bool(with_ref)
        if self.pad < 0 or not 0 <= self.pad_val <= 255:
            raise ValueError("FuseSpec: pad >= 0 and 0 <= pad_val <= 255")


class RefFrames(object):
    """The reference frames of a fused video, batch by batch, as pinned host tensors: ``get(k)`` -> (n_k,S,S,3) uint8 RGB of batch k of
    ``batches`` = [(first frame, frames), ...], in order, each once.  ``ref_imgs``: a (n,S,S,3) uint8 array / tensor (a device tensor is
    sliced and returned as it is), or n image paths - decoded by PIL on ``THREADS`` threads into a ring of pinned buffers, ``AHEAD`` batches in
    front of the consumer; a file that is not S x S is resized as ``imitator.load_images`` resizes (PIL bilinear: close to, not identical
    with, cv2.resize).  ``done(k, event)``: batch k's buffer may be decoded into again once ``event`` (its upload) has passed."""

    AHEAD = 2
    THREADS = 4

    def __init__(self, ref_imgs, n_frames, S, batches):
        self.S, self.batches = int(S), [(int(s), int(n)) for s, n in batches]
        self._paths = self._array = self._pool = None
        if isinstance(ref_imgs, (list, tuple)) and all(isinstance(p, (str, os.PathLike)) for p in ref_imgs):
            n = len(ref_imgs)
            self._paths = [os.fspath(p) for p in ref_imgs]
        else:
            a = ref_imgs if torch.is_tensor(ref_imgs) else torch.from_numpy(np.ascontiguousarray(ref_imgs))
            if a.dtype != torch.uint8 or a.dim() != 4 or tuple(a.shape[1:]) != (self.S, self.S, 3):
                raise ValueError("ref_imgs: a (n,%d,%d,3) uint8 RGB array or a list of image paths" % (self.S, self.S))
            n = a.shape[0]
            self._array = a
        if n != int(n_frames):
            raise ValueError("ref_imgs holds %d frames for %d target frames (the reference asserts the same)" % (n, int(n_frames)))
        if self._paths is not None and self.batches:
            from concurrent.futures import ThreadPoolExecutor
            self._pool = ThreadPoolExecutor(self.THREADS)
            most = max(nb for _, nb in self.batches)
            self._ring = [torch.empty((most, self.S, self.S, 3), dtype=torch.uint8, pin_memory=torch.cuda.is_available()) for _ in range(self.AHEAD + 1)]
            self._busy = [None] * len(self._ring)          # the upload event of the batch that used the buffer last
            self._futures = {}
            self._scheduled = 0
            self._fill(0)

    def _decode(self, path, dst):
        from PIL import Image
        im = Image.open(path).convert("RGB")
        if im.size != (self.S, self.S):
            im = im.resize((self.S, self.S), Image.BILINEAR)
        dst.copy_(torch.from_numpy(np.array(im)))

    def _fill(self, k):
        """Schedule the decodes of every batch up to k + AHEAD."""
        while self._scheduled < min(len(self.batches), k + self.AHEAD + 1):
            j = self._scheduled
            slot = j % len(self._ring)
            if self._busy[slot] is not None:
                self._busy[slot].synchronize()
                self._busy[slot] = None
            s, n = self.batches[j]
            self._futures[j] = [self._pool.submit(self._decode, self._paths[s + i], self._ring[slot][i]) for i in range(n)]
            self._scheduled += 1

    def get(self, k):
        s, n = self.batches[k]
        if self._array is not None:
            return self._array[s:s + n]
        for f in self._futures.pop(k):
            f.result()
        return self._ring[k % len(self._ring)][:n]

    def done(self, k, event=None):
        if self._pool is not None:
            self._busy[k % len(self._ring)] = event
            self._fill(k + 1)

    def close(self):
        if self._pool is not None:
            self._pool.shutdown(wait=True)


class FrameWriter(object):
    """Asynchronous ``(B,3,S,S)`` fp32 device frames -> PNG files (encoder "host" | "device"), JPEG files ("jpeg") or one Motion-JPEG AVI file
    ("mjpeg": ``"{prefix}{video_name}"``).  ``submit`` returns immediately; ``close`` joins.  ``fuse``: a ``FuseSpec`` - what is encoded is the
    comparison canvas around every frame instead of the frame (device frames only)."""

    DEVICE_WORKERS = 4          # encoder="device": a worker checksums and writes (zlib.crc32 and the file write release the GIL); not sized by the machine
    ROWS_PER_SEGMENT = 16       # encoder="device": scanlines per deflate block (include/lwg_hip.h lwg_png_deflate_u8)
    RING = 4                    # batches between the producer and the files (pinned buffers of the PNG encoders)
    CODED_RING = 8              # encoder="jpeg" | "mjpeg": a batch passes two copies and their helper thread before a worker sees it; with 4 the
                                # producer waits for the per-file form (GPU side 1 069 against 1 165 frames/s, profiles/jpeg_device_ab*.txt)

    def __init__(self, output_dir, prefix="pred_", workers=None, ring=None, compress_level=1, encoder="host", quality=90, fps=25, fuse=None,
                 video_name="video.avi", subsampling="444", huffman="fixed"):
        self.subsampling = jpeg_check_subsampling(subsampling)    # encoder="jpeg" | "mjpeg": the chroma format of the device encoder (the PNG encoders ignore it)
        self.huffman = jpeg_check_huffman(huffman)                # encoder="jpeg" | "mjpeg": "optimized" codes every frame with tables of its own (the PNG encoders ignore it)
        if fuse is not None and not isinstance(fuse, FuseSpec):
            raise TypeError("fuse must be a FuseSpec or None")
        self.fuse, self.video_name = fuse, str(video_name)
        self.ref_uploaded = None                           # fuse: the event behind the last upload of host reference frames (RefFrames.done)
        if encoder not in ("host", "device", "jpeg", "mjpeg"):
            raise ValueError("encoder must be 'host', 'device', 'jpeg' or 'mjpeg', not %r" % (encoder,))
        self.encoder = encoder
        self.coded = encoder in ("jpeg", "mjpeg")          # the device codes JPEG scans; only their used bytes are copied
        self.quality, self.fps = int(quality), fps
        if self.coded:
            jpeg_tables(self.quality)                      # (a quality outside 1 .. 100 raises here)
        self._avi = None                                   # encoder="mjpeg": the MjpegAviWriter, opened by the first submit (it needs the frame size)
        self._t_first = None
        ring = int(ring or (self.CODED_RING if self.coded else self.RING))
        self._slots = threading.Semaphore(ring)            # coded batches in flight (their device buffers are large: capacity is the worst case)
        self._pool, self._pool_lock = [], threading.Lock() # pinned buffers of the coded bytes
        self.output_dir, self.prefix = output_dir, prefix
        os.makedirs(output_dir, exist_ok=True)
        self.compress_level = compress_level
        if encoder != "host":
            self.workers = int(workers or self.DEVICE_WORKERS)
        else:
            self.workers = int(workers or min(32, max(2, (os.cpu_count() or 4) // 2)))     # (64 measured: the launching thread loses the GIL more often - 869 against 1 090 frames/s on the GPU side, 802 against 865 end to end)
        self.ring = ring
        self._free = queue.Queue()         # pinned host buffers whose frames are all encoded
        self._nbuf = 0
        self._jobs = queue.Queue()
        self._cv = threading.Condition()
        self._submitted = 0
        self._errors = []
        self.paths = {}
        self._copy_stream = None
        self._threads = [threading.Thread(target=self._worker, daemon=True) for _ in range(self.workers)]
        for t in self._threads:
            t.start()

    # ---- host side -------------------------------------------------------------------------------------------
    def _worker(self):
        while True:
            job = self._jobs.get()
            if job is None:
                return
            batch, i = job
            try:
                batch["ready"].wait()                      # the D2H copy of this batch has landed
                t = batch["t0"] + i
                if self.coded:
                    if batch["error"] is not None:
                        raise batch["error"]
                    a, n = batch["offs"][i], int(batch["nbytes"][i])
                    tables = None if batch["tables"] is None else batch["tables"].numpy()[i]
                    data = jpeg_from_scan(batch["host"].numpy()[a:a + n], batch["w"], batch["h"], self.quality, batch["ri"], self.subsampling, tables)
                    if self._avi is not None:
                        path = self._avi.path
                        self._avi.add(t - self._t_first, data)
                    else:
                        path = os.path.join(self.output_dir, self.prefix + "{:0>8}.jpg".format(t))
                        with open(path, "wb") as fp:
                            fp.write(data)
                    with self._cv:
                        self.paths[t] = path
                    continue
                path = os.path.join(self.output_dir, self.prefix + "{:0>8}.png".format(t))
                if batch["nbytes"] is None:
                    encode_png(path, batch["host"].numpy()[i], self.compress_level)
                else:                                      # the device encoded: frame, checksum, write
                    n = int(batch["nbytes"][i])
                    with open(path, "wb") as fp:
                        fp.write(png_from_stream(batch["host"].numpy()[i, :n], batch["w"], batch["h"]))
                with self._cv:
                    self.paths[t] = path
            except Exception as e:                         # surfaced by close()
                with self._cv:
                    self._errors.append(e)
            finally:
                with self._cv:
                    batch["left"] -= 1
                    if batch["left"] == 0:
                        if not self.coded:
                            self._free.put(batch["host"])
                        else:
                            if batch["host"] is not None:
                                with self._pool_lock:
                                    self._pool.append(batch["host"])
                            self._slots.release()
                    self._cv.notify_all()

    def _host_buffer(self, shape, pinned):
        """A pinned (B,S,S,3) uint8 buffer (encoder="device": (B, capacity)); blocks while all ``ring`` buffers still hold frames being encoded."""
        while True:
            if self._nbuf < self.ring and self._free.empty():
                self._nbuf += 1
                return torch.empty(shape, dtype=torch.uint8, pin_memory=pinned)
            buf = self._free.get()
            if tuple(buf.shape) == tuple(shape):
                return buf
            self._nbuf -= 1                                # a last, smaller batch: drop the buffer and allocate

    def _wait_copy(self, batch, event):
        if event is not None:
            event.synchronize()
        batch["ready"].set()

    def _wait_coded(self, batch, event, scans):
        """The helper thread of a coded batch: the lengths have landed -> copy the used prefix of every frame's scan buffer, behind each other,
        into one pinned buffer (on the copy stream, never from the producer thread), wait for them, release the device buffer."""
        try:
            event.synchronize()
            n = [int(v) for v in batch["nbytes"]]
            if min(n) < 0 or max(n) > scans.shape[1]:
                raise RuntimeError("jpeg_scan returned lengths outside its buffers: %r" % (n,))
            offs = [0]
            for v in n:
                offs.append(offs[-1] + ((v + 15) & ~15))
            total = max(offs[-1], 16)
            host = None
            with self._pool_lock:
                for k, buf in enumerate(self._pool):
                    if buf.numel() >= total:
                        host = self._pool.pop(k)
                        break
            if host is None:
                host = torch.empty(max(1 << 20, 1 << (total - 1).bit_length()), dtype=torch.uint8, pin_memory=True)
            batch["host"], batch["offs"] = host, offs
            with torch.cuda.device(scans.device), torch.cuda.stream(self._copy_stream):
                for i, v in enumerate(n):
                    if v:
                        host[offs[i]:offs[i] + v].copy_(scans[i, :v], non_blocking=True)
                landed = torch.cuda.Event()
                landed.record(self._copy_stream)
            landed.synchronize()
        except Exception as e:                             # every frame of the batch reports it
            batch["error"] = e
        finally:
            del scans
            batch["ready"].set()

    def _upload(self, host, device):
        """Host frames -> a device tensor through the copy stream (asynchronous when ``host`` is pinned); the current stream waits for it."""
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(device=device)
        cur = torch.cuda.current_stream(device)
        with torch.cuda.stream(self._copy_stream):
            dev = torch.empty(tuple(host.shape), dtype=host.dtype, device=device)
            dev.copy_(host, non_blocking=True)
            self.ref_uploaded = torch.cuda.Event()
            self.ref_uploaded.record(self._copy_stream)
        cur.wait_event(self.ref_uploaded)
        dev.record_stream(cur)
        return dev

    def _to_u8(self, pred, ref=None, more=()):
        """THE conversion step in front of every encoder: device frames (B,3,S,S) fp32 -> (B,H,W,3) uint8 RGB on the device - the frame itself
        (``lwg_frames_to_u8``), or with ``fuse`` the comparison canvas around it (``lwg_fuse_canvas_u8``: H = S, W = Wc)."""
        from . import ops
        if self.fuse is None:
            if ref is not None or len(more):
                raise ValueError("FrameWriter.submit: ref / more need FrameWriter(fuse=...)")
            return ops.frames_to_u8(pred.contiguous())
        if self.fuse.with_ref:
            if ref is None:
                raise ValueError("FrameWriter(fuse=FuseSpec(with_ref=True)).submit needs the batch's reference frames")
            if not torch.is_tensor(ref):
                ref = torch.from_numpy(np.ascontiguousarray(ref))
            if not ref.is_cuda:
                ref = self._upload(ref, pred.device)
        else:
            ref = None
        return ops.fuse_canvas(self.fuse.panel, ref, (pred,) + tuple(more), self.fuse.pad, self.fuse.pad_val)

    def _submit_coded(self, pred, t0, ref, more):
        from . import ops
        B = pred.shape[0]
        self._slots.acquire()                              # blocks while ``ring`` batches are still being copied or written
        try:
            u8 = self._to_u8(pred, ref, more)
            H, W = u8.shape[1], u8.shape[2]
            side = ops.jpeg_mcu_size(self.subsampling)
            ri = min((W + side - 1) // side, ops.jpeg_max_mcus_per_segment(self.subsampling))
            tables = tables_host = None
            if self.huffman == "fixed":
                scans, nbytes = ops.jpeg_scan(u8, self.quality, ri, self.subsampling)
            else:                                          # the frames' tables ride with the lengths in the first, small copy
                scans, nbytes, tables = ops.jpeg_scan(u8, self.quality, ri, self.subsampling, self.huffman)
                tables_host = torch.empty(tuple(tables.shape), dtype=torch.uint8, pin_memory=True)
            nbytes_host = torch.empty(B, dtype=torch.int32, pin_memory=True)
            if self._copy_stream is None:
                self._copy_stream = torch.cuda.Stream(device=pred.device)
            if self.encoder == "mjpeg" and self._avi is None:
                self._t_first = int(t0)
                self._avi = MjpegAviWriter(os.path.join(self.output_dir, self.prefix + self.video_name), W, H, self.fps)
            produced = torch.cuda.Event()
            produced.record(torch.cuda.current_stream(pred.device))
            with torch.cuda.stream(self._copy_stream):
                self._copy_stream.wait_event(produced)
                nbytes_host.copy_(nbytes, non_blocking=True)
                if tables is not None:
                    tables_host.copy_(tables, non_blocking=True)
                event = torch.cuda.Event()
                event.record(self._copy_stream)
            nbytes.record_stream(self._copy_stream)
            scans.record_stream(self._copy_stream)
            if tables is not None:
                tables.record_stream(self._copy_stream)
        except Exception:
            self._slots.release()
            raise
        batch = {"host": None, "offs": None, "t0": int(t0), "left": B, "ready": threading.Event(), "nbytes": nbytes_host, "h": H, "w": W, "ri": ri,
                 "error": None, "tables": tables_host}
        with self._cv:
            self._submitted += B
        threading.Thread(target=self._wait_coded, args=(batch, event, scans), daemon=True).start()
        for i in range(B):
            self._jobs.put((batch, i))

    # ---- producer side ---------------------------------------------------------------------------------------
    def submit(self, pred, t0, ref=None, more=()):
        """pred: (B,3,S,S) fp32 frames t0 .. t0+B-1, on the device (or on the CPU: tests).  With ``fuse``: ref = the batch's (B,S,S,3) uint8
        RGB reference frames (a device tensor, or a host tensor / array, which is uploaded on the copy stream) where the spec has them, and
        ``more`` = up to three further (B,3,S,S) outputs shown behind ``pred``."""
        B = pred.shape[0]
        if self.fuse is not None and not pred.is_cuda:
            raise RuntimeError("FrameWriter(fuse=...) needs device frames: there is no CPU fallback")
        if self.coded:
            if not pred.is_cuda:
                raise RuntimeError("FrameWriter(encoder=%r) needs device frames: there is no CPU fallback" % (self.encoder,))
            if B:
                self._submit_coded(pred, t0, ref, more)
            return
        event = None
        nbytes_host = None
        if self.encoder == "device" and not pred.is_cuda:
            raise RuntimeError("FrameWriter(encoder='device') needs device frames: there is no CPU fallback")
        if pred.is_cuda:
            from . import ops
            u8 = self._to_u8(pred, ref, more)
            H, W = u8.shape[1], u8.shape[2]
            nbytes = None
            if self.encoder == "device":                   # what is copied and handed to the workers is the streams, not the pixels
                u8, nbytes = ops.png_deflate(u8, ops.png_rows_per_segment(H, W, self.ROWS_PER_SEGMENT))
                nbytes_host = torch.empty(B, dtype=torch.int32, pin_memory=True)
            host = self._host_buffer(tuple(u8.shape), True)
            if self._copy_stream is None:
                self._copy_stream = torch.cuda.Stream(device=pred.device)
            produced = torch.cuda.Event()
            produced.record(torch.cuda.current_stream(pred.device))
            with torch.cuda.stream(self._copy_stream):
                self._copy_stream.wait_event(produced)
                host.copy_(u8, non_blocking=True)
                if nbytes is not None:
                    nbytes_host.copy_(nbytes, non_blocking=True)
                event = torch.cuda.Event()
                event.record(self._copy_stream)
            u8.record_stream(self._copy_stream)
            if nbytes is not None:
                nbytes.record_stream(self._copy_stream)
        else:
            H, W = pred.shape[2], pred.shape[3]
            host = self._host_buffer((B, H, W, 3), False)
            x = np.transpose(pred.detach().numpy().astype(np.float32), (0, 2, 3, 1))
            host.copy_(torch.from_numpy(((x + 1) / 2.0 * 255).astype(np.uint8)))
        batch = {"host": host, "t0": int(t0), "left": B, "ready": threading.Event(), "nbytes": nbytes_host, "h": H, "w": W}
        with self._cv:
            self._submitted += B
        threading.Thread(target=self._wait_copy, args=(batch, event), daemon=True).start()
        for i in range(B):
            self._jobs.put((batch, i))

    def close(self):
        """Wait for every submitted frame to be on disk, stop the pool, return the paths in frame order."""
        with self._cv:
            while len(self.paths) + len(self._errors) < self._submitted:
                self._cv.wait(timeout=0.1)
        for _ in self._threads:
            self._jobs.put(None)
        for t in self._threads:
            t.join()
        if self._avi is not None:
            try:
                video = self._avi.close()
            except Exception as e:
                self._errors.append(e)
        if self._errors:
            raise self._errors[0]
        if self._avi is not None:
            return video
        return [self.paths[t] for t in sorted(self.paths)]
