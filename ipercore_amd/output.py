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

File names are the reference's: ``"{prefix}{t:0>8}.png"`` (imitator.py:369).  Pixels on disk are RGB, exactly what
``cv2.imwrite`` stores for the BGR array the reference hands it.
"""
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


class FrameWriter(object):
    """Asynchronous ``(B,3,S,S)`` fp32 device frames -> PNG files.  ``submit`` returns immediately; ``close`` joins."""

    DEVICE_WORKERS = 4          # encoder="device": a worker checksums and writes (zlib.crc32 and the file write release the GIL); not sized by the machine
    ROWS_PER_SEGMENT = 16       # encoder="device": scanlines per deflate block (include/lwg_hip.h lwg_png_deflate_u8)

    def __init__(self, output_dir, prefix="pred_", workers=None, ring=4, compress_level=1, encoder="host"):
        if encoder not in ("host", "device"):
            raise ValueError("encoder must be 'host' or 'device', not %r" % (encoder,))
        self.encoder = encoder
        self.output_dir, self.prefix = output_dir, prefix
        os.makedirs(output_dir, exist_ok=True)
        self.compress_level = compress_level
        if encoder == "device":
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
                        self._free.put(batch["host"])
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

    # ---- producer side ---------------------------------------------------------------------------------------
    def submit(self, pred, t0):
        """pred: (B,3,S,S) fp32 frames t0 .. t0+B-1, on the device (or on the CPU: tests)."""
        B = pred.shape[0]
        event = None
        nbytes_host = None
        if self.encoder == "device" and not pred.is_cuda:
            raise RuntimeError("FrameWriter(encoder='device') needs device frames: there is no CPU fallback")
        if pred.is_cuda:
            from . import ops
            u8 = ops.frames_to_u8(pred.contiguous())
            nbytes = None
            if self.encoder == "device":                   # what is copied and handed to the workers is the streams, not the pixels
                u8, nbytes = ops.png_deflate(u8, self.ROWS_PER_SEGMENT)
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
            host = self._host_buffer((B, pred.shape[2], pred.shape[3], 3), False)
            x = np.transpose(pred.detach().numpy().astype(np.float32), (0, 2, 3, 1))
            host.copy_(torch.from_numpy(((x + 1) / 2.0 * 255).astype(np.uint8)))
        batch = {"host": host, "t0": int(t0), "left": B, "ready": threading.Event(), "nbytes": nbytes_host, "h": pred.shape[2], "w": pred.shape[3]}
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
        if self._errors:
            raise self._errors[0]
        return [self.paths[t] for t in sorted(self.paths)]
