"""The device JPEG encoder without a GPU: tests/jpegdev_emu.py - the definition of the scan - against a real decoder and against
PIL's encoder, the host code around the scan (output.jpeg_tables / jpeg_from_scan / MjpegAviWriter / FrameWriter) and the argument checks of
the C entry points (the library loads without a GPU).

Grid: sizes (1,1) (8,8) (17,23) (24,40) (64,64) (128,128); qualities 50, 90, 100; contents constant, smooth gradient, uniform noise, smooth +
noise, 0/255 checkerboard; restart intervals per size: one MCU row, 1, one that does not divide the row, one that gives more than 8 segments.

Measured on the CPU with Pillow 12.2 (libjpeg-turbo), the emulator at one MCU row per segment against
``save("JPEG", qtables=the same tables, subsampling=0, optimize=False, restart_marker_rows=1)``:
  * quality 100: every frame decodes with PSNR >= 49.89 dB (the floor asserted is 45 dB);
  * worst PSNR deficit against PIL over the whole grid: 3.01 dB, on the ONE-pixel frame (smooth + noise, quality 50: an error of one level more
    in two channels of one pixel); over the frames of 17 x 23 and larger 0.86 dB (64 x 64 smooth, quality 90).  PIL loses by up to 3.4 dB on
    other cells (checkerboard, quality 50);
  * worst file size ratio against PIL: 1.100 (128 x 128 smooth, quality 90; PIL's is larger by up to 15 % on other cells).
The emulator is deterministic; the margins asserted on top - 0.5 dB and 5 % - are for another libjpeg build behind PIL, whose forward DCT may
differ: deficit <= 3.51 dB (<= 1.36 dB from 17 x 23 on), ratio <= 1.155.
"""
import io
import os
import struct
import tempfile

import numpy as np
import pytest

from ipercore_amd import _lib, output
from tests import jpegdev_emu as emu

SIZES = ((1, 1), (8, 8), (17, 23), (24, 40), (64, 64), (128, 128))
QUALITIES = (50, 90, 100)
NEW = ("lwg_jpeg_scan_u8", "lwg_jpeg_scan_capacity", "lwg_jpeg_scan_ws_bytes", "lwg_jpeg_max_mcus_per_segment")
DEFICIT_DB, DEFICIT_DB_17, RATIO = 3.01 + 0.5, 0.86 + 0.5, 1.100 * 1.05


def intervals(H, W):
    """The restart intervals of the grid for an (H, W) frame: one MCU row, 1, the smallest value that does not divide the row, and one that
    cuts the frame into more than 8 segments (where it has more than 8 MCUs)."""
    my, mx = (H + 7) // 8, (W + 7) // 8
    n = my * mx
    ragged = [r for r in range(2, mx) if mx % r][:1]
    return sorted(r for r in {mx, 1, max(1, (n - 1) // 9)} | set(ragged) if r <= 64)


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def decode(data, W, H):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    assert im.size == (W, H) and im.mode == "RGB" and im.format == "JPEG"
    return np.asarray(im)


def riff_frames(data):
    """A walk through a RIFF AVI file -> avih's fields, strh's handler, the 00dc payloads in file order; checks the sizes, idx1 and the padding."""
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI " and struct.unpack("<I", data[4:8])[0] == len(data) - 8
    info = {"frames": []}
    offsets = []

    def walk(a, b, movi):
        while a < b:
            tag, size = data[a:a + 4], struct.unpack("<I", data[a + 4:a + 8])[0]
            body = a + 8
            assert body + size <= b, tag
            if tag == b"LIST":
                kind = data[body:body + 4]
                walk(body + 4, body + size, body if kind == b"movi" else movi)
                if kind == b"movi":
                    info["movi"] = body
            elif tag == b"avih":
                f = struct.unpack("<14I", data[body:body + size])
                info.update(usec=f[0], flags=f[3], total=f[4], streams=f[6], width=f[8], height=f[9])
            elif tag == b"strh":
                info.update(fcc=data[body:body + 4], handler=data[body + 4:body + 8])
                info["scale"], info["rate"], _, info["length"] = struct.unpack("<4I", data[body + 20:body + 36])
            elif tag == b"strf":
                bi = struct.unpack("<IiiHH4s", data[body:body + 20])
                info.update(bi_size=bi[0], bi_w=bi[1], bi_h=bi[2], bi_bits=bi[4], bi_comp=bi[5])
            elif tag == b"00dc":
                assert movi is not None
                info["frames"].append(data[body:body + size])
                offsets.append((a - movi, size))
            elif tag == b"idx1":
                info["idx1"] = [struct.unpack("<4sIII", data[body + 16 * k:body + 16 * k + 16]) for k in range(size // 16)]
            else:
                raise AssertionError("unexpected chunk %r" % tag)
            a = body + size + (size & 1)                   # chunks start on even offsets
        assert a == b or a == b + 1
    walk(12, len(data), None)
    assert [(b"00dc", 0x10, o, s) for o, s in offsets] == info["idx1"]
    for _, _, o, s in info["idx1"]:
        assert o % 2 == 0 and data[info["movi"] + o:info["movi"] + o + 4] == b"00dc"
    assert info["fcc"] == b"vids" and info["handler"] == b"MJPG" and info["bi_comp"] == b"MJPG" and info["flags"] & 0x10 and info["streams"] == 1
    assert info["length"] == info["total"] == len(info["frames"]) and (info["bi_size"], info["bi_w"], info["bi_h"]) == (40, info["width"], info["height"])
    return info


def check_scan(scan, H, W, ri):
    """No FF but FF 00 and the RST markers, which come in the order D0 .. D7 D0 ..; the number of segments."""
    _, _, nseg = emu.geometry(H, W, ri)
    marks, i = [], scan.find(b"\xff")
    while i >= 0:
        assert i + 1 < len(scan), "the scan ends in FF"
        if scan[i + 1] != 0:
            marks.append(scan[i + 1])
        i = scan.find(b"\xff", i + 2)
    assert marks == [0xD0 + k % 8 for k in range(nseg - 1)], (marks, nseg)


# ---- the definition -----------------------------------------------------------------------------------------------------------------------------
def test_tables_are_the_standard_ones():
    """The emulator's constants against their rules, and its Huffman and base quantisation tables against the ones libjpeg writes."""
    from PIL import Image
    assert (emu.dct_matrix() == emu.DCT_M).all()
    assert sorted(emu.ZIGZAG) == list(range(64))
    buf = io.BytesIO()
    Image.fromarray(emu.frame("smooth", 16, 16)).save(buf, "JPEG", quality=50, subsampling=0, optimize=False)
    data = buf.getvalue()
    dht, i = {}, data.find(b"\xff\xc4")
    while i >= 0:
        body = data[i + 4:i + 2 + struct.unpack(">H", data[i + 2:i + 4])[0]]
        while body:
            n = sum(body[1:17])
            dht[body[0]] = (list(body[1:17]), list(body[17:17 + n]))
            body = body[17 + n:]
        i = data.find(b"\xff\xc4", i + 2)
    for key, spec in ((0x00, emu.DC_LUMA), (0x10, emu.AC_LUMA), (0x01, emu.DC_CHROMA), (0x11, emu.AC_CHROMA)):
        assert dht[key] == (list(spec[0]), list(spec[1])), hex(key)
    q = Image.open(io.BytesIO(data)).quantization               # quality 50 is the base tables; natural or zigzag order depending on the Pillow
    for k, base in enumerate((emu.Q_LUMA, emu.Q_CHROMA)):
        assert list(q[k]) in (list(base), list(base[emu.ZIGZAG]))
    for quality in (1, 10, 49, 50, 75, 90, 100):
        assert [list(t) for t in emu.tables(quality)] == [list(t) for t in output.jpeg_tables(quality)]
    assert set(emu.tables(100)[0]) == {1} and emu.tables(1)[0].max() == 255
    for bad in (0, 101):
        with pytest.raises(ValueError):
            output.jpeg_tables(bad)


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("quality", QUALITIES)
def test_emulator_files_decode(quality, H, W):
    for kind in emu.KINDS:
        img = emu.frame(kind, H, W)
        for ri in intervals(H, W):
            scan = emu.scan(img, quality, ri)
            assert 0 < len(scan) <= emu.capacity(H, W, ri)
            check_scan(scan, H, W, ri)
            data = emu.file(img, quality, ri)
            assert data == output.jpeg_from_scan(scan, W, H, quality, ri), "output.jpeg_from_scan differs from the emulator's file"
            assert data == output.jpeg_from_scan(np.frombuffer(scan, np.uint8), W, H, quality, ri)
            p = psnr(decode(data, W, H), img)
            print("%s %d x %d q %d interval %d: %d bytes, %.2f dB" % (kind, H, W, quality, ri, len(data), p))
            if quality == 100:
                assert p >= 45.0, (kind, ri, p)


def test_against_pils_encoder():
    """Equal tables, 4:4:4, fixed Huffman tables, a restart marker per MCU row on both sides."""
    from PIL import Image
    worst = {"deficit": (-99.0, None), "deficit17": (-99.0, None), "ratio": (0.0, None)}
    for H, W in SIZES:
        for quality in QUALITIES:
            qt = emu.tables(quality)
            for kind in emu.KINDS:
                img = emu.frame(kind, H, W)
                mine = emu.file(img, quality, (W + 7) // 8)
                buf = io.BytesIO()
                Image.fromarray(img).save(buf, "JPEG", qtables=[[int(v) for v in t[emu.ZIGZAG]] for t in qt], subsampling=0, optimize=False,
                                          restart_marker_rows=1)
                theirs = buf.getvalue()
                q = Image.open(io.BytesIO(theirs)).quantization
                assert all(list(q[k]) in ([int(v) for v in qt[k]], [int(v) for v in qt[k][emu.ZIGZAG]]) for k in (0, 1))
                deficit = psnr(decode(theirs, W, H), img) - psnr(decode(mine, W, H), img)
                ratio = len(mine) / len(theirs)
                cell = (kind, H, W, quality)
                print("%s %d x %d q %d: deficit %.2f dB, size ratio %.3f" % (cell + (deficit, ratio)))
                worst["deficit"] = max(worst["deficit"], (deficit, cell))
                worst["ratio"] = max(worst["ratio"], (ratio, cell))
                if H >= 17:
                    worst["deficit17"] = max(worst["deficit17"], (deficit, cell))
    print("worst", worst)
    assert worst["deficit"][0] <= DEFICIT_DB, worst
    assert worst["deficit17"][0] <= DEFICIT_DB_17, worst
    assert worst["ratio"][0] <= RATIO, worst


def test_emulator_is_fast_enough_for_a_512_frame():
    import time
    img = emu.frame("noise", 512, 512)
    t = time.perf_counter()
    data = emu.file(img, 100, 64)
    dt = time.perf_counter() - t
    assert decode(data, 512, 512).shape == (512, 512, 3)
    assert dt < 10.0, dt


# ---- the library without a GPU ------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_bound():
    hdr = _lib.header_symbols()
    for name in NEW:
        assert name in hdr and name in _lib._SIGS, name
    assert _lib.lib().lwg_abi_version() == 10
    assert _lib.lib().lwg_jpeg_max_mcus_per_segment() == 64


def test_capacity_is_the_emulators_bound():
    lib = _lib.lib()
    for H, W in SIZES + ((512, 512), (1024, 1024)):
        for ri in intervals(H, W) + [64]:
            cap = emu.capacity(H, W, ri)
            _, _, nseg = emu.geometry(H, W, ri)
            assert lib.lwg_jpeg_scan_capacity(H, W, ri) == cap, (H, W, ri)
            assert lib.lwg_jpeg_scan_ws_bytes(3, H, W, ri) >= 3 * (cap - 2 * (nseg - 1))
    assert emu.capacity(512, 512, 64) == 64 * 64 * 1248 + 2 * 63


def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib.lib()
    good = bytes([1] * 128)
    ok = dict(u8=16, B=1, H=8, W=8, q=good, ri=1, ws=16, scans=16, nbytes=16)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.lwg_jpeg_scan_u8(a["u8"], a["B"], a["H"], a["W"], a["q"], a["ri"], a["ws"], a["scans"], a["nbytes"], None)
    for bad in (dict(u8=None), dict(q=None), dict(ws=None), dict(scans=None), dict(nbytes=None), dict(B=0), dict(B=-3), dict(H=0), dict(W=-1),
                dict(ri=0), dict(ri=-1), dict(ri=65), dict(ri=65536),
                dict(q=bytes([1] * 127 + [0])), dict(q=bytes([0] + [1] * 127)), dict(q=bytes([1] * 64 + [0] + [1] * 63)),
                dict(H=16384, W=16384, ri=64),     # 4 194 304 MCUs x 1 248 bytes: beyond int32
                dict(ws=24)):                      # not 16-byte aligned
        assert call(**bad) == 1, bad
    for H, W, ri in ((0, 8, 1), (8, 0, 1), (8, 8, 0), (8, 8, 65), (8, 8, 65536), (16384, 16384, 64)):
        assert lib.lwg_jpeg_scan_capacity(H, W, ri) == 0
        assert lib.lwg_jpeg_scan_ws_bytes(1, H, W, ri) == 0
    assert lib.lwg_jpeg_scan_ws_bytes(0, 8, 8, 1) == 0


def test_frame_writer_jpeg_has_no_cpu_fallback():
    import torch
    from ipercore_amd import ops
    with tempfile.TemporaryDirectory() as d:
        for enc in ("jpeg", "mjpeg"):
            w = output.FrameWriter(d, encoder=enc)
            try:
                assert w.workers == output.FrameWriter.DEVICE_WORKERS and w.quality == 90
                with pytest.raises(RuntimeError):
                    w.submit(torch.zeros(1, 3, 8, 8), 0)
            finally:
                assert w.close() == []
        with pytest.raises(ValueError):
            output.FrameWriter(d, encoder="jpeg", quality=0)
        with pytest.raises(ValueError):
            output.FrameWriter(d, encoder="jpg")
    with pytest.raises(RuntimeError):
        ops.jpeg_scan(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))


# ---- the container ------------------------------------------------------------------------------------------------------------------------------
def test_mjpeg_avi_writer():
    H, W = 17, 23
    frames = [emu.file(emu.frame(kind, H, W), 90, 3) for kind in emu.KINDS]
    assert any(len(f) & 1 for f in frames) and any(not len(f) & 1 for f in frames)          # both paddings occur
    with tempfile.TemporaryDirectory() as d:
        w = output.MjpegAviWriter(os.path.join(d, "clip.avi"), W, H, 25)
        for k in (3, 0, 4, 2, 1):                                                           # out of order
            w.add(k, frames[k])
        with pytest.raises(ValueError):
            w.add(3, frames[3])
        assert w.close() == [os.path.join(d, "clip.avi")]
        with open(os.path.join(d, "clip.avi"), "rb") as fp:
            info = riff_frames(fp.read())
        assert info["frames"] == frames
        assert (info["width"], info["height"], info["total"], info["usec"], info["scale"], info["rate"]) == (W, H, 5, 40000, 1000, 25000)
        for f, kind in zip(info["frames"], emu.KINDS):
            assert decode(f, W, H).shape == (H, W, 3), kind
        # a missing frame is an error, not a shorter file
        w = output.MjpegAviWriter(os.path.join(d, "gap.avi"), W, H, 25)
        w.add(1, frames[1])
        with pytest.raises(RuntimeError):
            w.close()
        # the size guard: a file that would pass the limit is refused with the frame's number
        w = output.MjpegAviWriter(os.path.join(d, "big.avi"), W, H, 25)
        w.MAX_BYTES = w._pos + 8 + 16 + len(frames[0]) + len(frames[1]) + 64               # room for two frames, not three
        assert output.MjpegAviWriter.MAX_BYTES == 2 ** 31 - 1
        w.add(0, frames[0])
        w.add(1, frames[1])
        w.add(2, frames[2])
        with pytest.raises(RuntimeError, match="would exceed"):
            w.close()
