"""The device JPEG encoder's 4:2:0 format without a GPU: tests/jpeg420_emu.py - the definition of the scan - against a real
decoder, against PIL's encoder and against the 4:4:4 definition, the host code around the scan (output.jpeg_headers / jpeg_from_scan /
FrameWriter / Imitator's option) and the argument checks of the four C entry points (the library loads without a GPU).

Grid: sizes (1,1) (8,8) (16,16) (17,23) (24,40) (33,47) (64,64) (128,128); qualities 50, 90, 100; the five contents of jpegdev_emu.KINDS;
restart intervals per size, in 16 x 16 MCUs: one MCU row, 1, one that does not divide the row, one that gives more than 8 segments.

Measured on the CPU with Pillow 12.2 (libjpeg-turbo), the emulator at one MCU row per segment against
``save("JPEG", qtables=the same tables, subsampling=2, optimize=False, restart_marker_rows=1)``:
  * worst PSNR deficit against PIL over the whole grid: 3.01 dB, on the ONE-pixel frame (smooth + noise, quality 50); over the frames of
    17 x 23 and larger 0.46 dB (24 x 40 smooth, quality 100);
  * worst file size ratio against PIL: 1.105 (24 x 40 checkerboard, quality 50).
The margins asserted on top - 0.5 dB and 5 %, those of tests/test_jpeg_device_cpu.py - are for another libjpeg build behind PIL: deficit
<= 3.51 dB (<= 0.96 dB from 17 x 23 on), ratio <= 1.160.
  * constant and checkerboard frames (constant chroma: nothing for 4:2:0 to remove, and the Y blocks hold the values the 4:4:4 blocks hold):
    the decoded PSNR equals that of the 4:4:4 file of the same frame; the largest gap over the grid is 0.00 dB.  Asserted with a margin of
    0.01 dB: a decoder that interpolates chroma ("fancy upsampling") returns a constant plane unchanged, so only the rounding of a printed
    figure is allowed for.
  * uniform colour noise is where the format is destructive (12.7 dB against 30.0 dB at quality 90, 128 x 128): no floor is asserted on it.
"""
import io
import tempfile

import numpy as np
import pytest

from ipercore_amd import _lib, output
from tests import jpeg420_emu as emu
from tests import jpegdev_emu as emu444
from tests.test_jpeg_device_cpu import decode, psnr

SIZES = ((1, 1), (8, 8), (16, 16), (17, 23), (24, 40), (33, 47), (64, 64), (128, 128))
QUALITIES = (50, 90, 100)
NEW = ("lwg_jpeg420_scan_u8", "lwg_jpeg420_scan_capacity", "lwg_jpeg420_scan_ws_bytes", "lwg_jpeg420_max_mcus_per_segment")
DEFICIT_DB, DEFICIT_DB_17, RATIO = 3.01 + 0.5, 0.46 + 0.5, 1.105 * 1.05
CONSTANT_CHROMA_GAP_DB = 0.01


def intervals(H, W):
    """The restart intervals of the grid for an (H, W) frame, in 16 x 16 MCUs: one MCU row, 1, the smallest value that does not divide the
    row, and one that cuts the frame into more than 8 segments (where it has more than 8 MCUs)."""
    my, mx = (H + 15) // 16, (W + 15) // 16
    n = my * mx
    ragged = [r for r in range(2, mx) if mx % r][:1]
    return sorted(r for r in {mx, 1, max(1, (n - 1) // 9)} | set(ragged) if r <= 64)


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
def test_grid_has_its_intervals():
    assert intervals(128, 128) == [1, 3, 7, 8] and intervals(33, 47) == [1, 2, 3] and intervals(1, 1) == [1]
    assert emu.geometry(128, 128, 7)[2] > 8 and emu.geometry(33, 47, 3) == (3, 3, 3)


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
            assert data == output.jpeg_from_scan(scan, W, H, quality, ri, subsampling="420"), "output.jpeg_from_scan differs from the emulator's file"
            assert data == output.jpeg_from_scan(np.frombuffer(scan, np.uint8), W, H, quality, ri, "420")
            p = psnr(decode(data, W, H), img)
            print("%s %d x %d q %d interval %d: %d bytes, %.2f dB" % (kind, H, W, quality, ri, len(data), p))


def test_headers_differ_from_444_in_one_byte_and_the_default_is_untouched():
    for (W, H, q, ri) in ((1, 1, 50, 1), (23, 17, 90, 2), (512, 512, 90, 32), (65535, 9, 100, 64)):
        base = emu444.headers(W, H, emu444.tables(q), ri)
        assert output.jpeg_headers(W, H, q, ri) == base                      # without the new argument: the default is untouched
        assert output.jpeg_headers(W, H, q, ri, "444") == base and output.jpeg_headers(W, H, q, ri, subsampling="444") == base
        h420 = output.jpeg_headers(W, H, q, ri, "420")
        assert h420 == emu.headers(W, H, emu.tables(q), ri) and len(h420) == len(base)
        diff = [i for i in range(len(base)) if base[i] != h420[i]]
        assert len(diff) == 1 and (base[diff[0]], h420[diff[0]]) == (0x11, 0x22) and base[diff[0] - 11:diff[0] - 9] == b"\xff\xc0"
        assert output.jpeg_from_scan(b"\x00", W, H, q, ri) == base + b"\x00\xff\xd9"
    for bad in ("411", "422", 420, None, ""):
        with pytest.raises(ValueError):
            output.jpeg_headers(8, 8, 90, 1, bad)
        with pytest.raises(ValueError):
            output.jpeg_from_scan(b"", 8, 8, 90, 1, subsampling=bad)


def test_against_pils_encoder():
    """Equal tables, 4:2:0, fixed Huffman tables, a restart marker per MCU row on both sides."""
    from PIL import Image
    worst = {"deficit": (-99.0, None), "deficit17": (-99.0, None), "ratio": (0.0, None)}
    for H, W in SIZES:
        for quality in QUALITIES:
            qt = emu.tables(quality)
            for kind in emu.KINDS:
                img = emu.frame(kind, H, W)
                mine = emu.file(img, quality, (W + 15) // 16)
                buf = io.BytesIO()
                Image.fromarray(img).save(buf, "JPEG", qtables=[[int(v) for v in t[emu444.ZIGZAG]] for t in qt], subsampling=2, optimize=False,
                                          restart_marker_rows=1)
                theirs = buf.getvalue()
                q = Image.open(io.BytesIO(theirs)).quantization
                assert all(list(q[k]) in ([int(v) for v in qt[k]], [int(v) for v in qt[k][emu444.ZIGZAG]]) for k in (0, 1))
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


def test_constant_chroma_costs_nothing():
    """constant and checker have constant chroma: the 4:2:0 file decodes to the PSNR of the 4:4:4 file of the same frame."""
    worst = (-1.0, None)
    for H, W in SIZES:
        for quality in QUALITIES:
            for kind in ("constant", "checker"):
                img = emu.frame(kind, H, W)
                p420 = psnr(decode(emu.file(img, quality), W, H), img)
                p444 = psnr(decode(emu444.file(img, quality), W, H), img)
                print("%s %d x %d q %d: 4:2:0 %.2f dB, 4:4:4 %.2f dB" % (kind, H, W, quality, p420, p444))
                worst = max(worst, (abs(p420 - p444), (kind, H, W, quality)))
    assert worst[0] <= CONSTANT_CHROMA_GAP_DB, worst


def test_420_file_is_smaller_on_an_image_like_frame():
    img = emu.frame("smooth_noise", 128, 128)
    n420, n444 = len(emu.file(img, 90)), len(emu444.file(img, 90))
    print("smooth_noise 128 x 128 q 90: %d bytes against %d (%.2f)" % (n420, n444, n420 / n444))
    assert n420 < n444


def test_emulator_is_fast_enough_for_a_512_frame():
    import time
    img = emu.frame("noise", 512, 512)
    t = time.perf_counter()
    data = emu.file(img, 100, 32)
    dt = time.perf_counter() - t
    assert decode(data, 512, 512).shape == (512, 512, 3)
    assert dt < 10.0, dt


# ---- the library without a GPU ------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_bound():
    hdr = _lib.header_symbols()
    for name in NEW:
        assert name in hdr and name in _lib._SIGS, name
    assert _lib.lib().lwg_abi_version() == 10
    assert _lib.lib().lwg_jpeg420_max_mcus_per_segment() >= 32          # an MCU row of a 512-wide frame is one segment
    from ipercore_amd import ops
    assert ops.jpeg_max_mcus_per_segment("420") == ops.jpeg_max_mcus_per_segment(subsampling="420") == _lib.lib().lwg_jpeg420_max_mcus_per_segment()
    assert ops.jpeg_max_mcus_per_segment() == ops.jpeg_max_mcus_per_segment("444") == 64
    with pytest.raises(ValueError):
        ops.jpeg_max_mcus_per_segment("411")


def test_capacity_is_the_emulators_bound():
    lib = _lib.lib()
    R = lib.lwg_jpeg420_max_mcus_per_segment()
    for H, W in SIZES + ((512, 512), (1024, 1024)):
        for ri in intervals(H, W) + [R]:
            cap = emu.capacity(H, W, ri)
            _, _, nseg = emu.geometry(H, W, ri)
            assert lib.lwg_jpeg420_scan_capacity(H, W, ri) == cap, (H, W, ri)
            assert lib.lwg_jpeg420_scan_ws_bytes(3, H, W, ri) >= 3 * (cap - 2 * (nseg - 1))
    assert emu.capacity(512, 512, 32) == 32 * 32 * 2496 + 2 * 31


def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib.lib()
    R = lib.lwg_jpeg420_max_mcus_per_segment()
    good = bytes([1] * 128)
    ok = dict(u8=16, B=1, H=8, W=8, q=good, ri=1, ws=16, scans=16, nbytes=16)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.lwg_jpeg420_scan_u8(a["u8"], a["B"], a["H"], a["W"], a["q"], a["ri"], a["ws"], a["scans"], a["nbytes"], None)
    for bad in (dict(u8=None), dict(q=None), dict(ws=None), dict(scans=None), dict(nbytes=None), dict(B=0), dict(B=-3), dict(H=0), dict(W=-1),
                dict(H=65536), dict(W=65536), dict(ri=0), dict(ri=-1), dict(ri=R + 1), dict(ri=65536),
                dict(q=bytes([1] * 127 + [0])), dict(q=bytes([0] + [1] * 127)), dict(q=bytes([1] * 64 + [0] + [1] * 63)),
                dict(H=16384, W=16384, ri=R),      # 1 048 576 MCUs x 2 496 bytes: beyond int32
                dict(ws=24)):                      # not 16-byte aligned
        assert call(**bad) == 1, bad
    for H, W, ri in ((0, 8, 1), (8, 0, 1), (8, 8, 0), (8, 8, R + 1), (8, 8, 65536), (16384, 16384, R), (65536, 8, 1)):
        assert lib.lwg_jpeg420_scan_capacity(H, W, ri) == 0
        assert lib.lwg_jpeg420_scan_ws_bytes(1, H, W, ri) == 0
    assert lib.lwg_jpeg420_scan_ws_bytes(0, 8, 8, 1) == 0


def test_bad_subsampling_raises_and_there_is_no_cpu_fallback():
    import torch
    from ipercore_amd import ops
    from ipercore_amd.imitator import Imitator
    with tempfile.TemporaryDirectory() as d:
        for enc in ("jpeg", "mjpeg"):
            w = output.FrameWriter(d, encoder=enc, subsampling="420")
            try:
                assert w.subsampling == "420" and w.workers == output.FrameWriter.DEVICE_WORKERS and w.quality == 90
                with pytest.raises(RuntimeError):
                    w.submit(torch.zeros(1, 3, 8, 8), 0)
            finally:
                assert w.close() == []
        w = output.FrameWriter(d, encoder="jpeg")
        assert w.subsampling == "444" and w.close() == []
        for bad in ("411", "422", 420, None):
            with pytest.raises(ValueError):
                output.FrameWriter(d, encoder="jpeg", subsampling=bad)
    with pytest.raises(RuntimeError):
        ops.jpeg_scan(torch.zeros(1, 16, 16, 3, dtype=torch.uint8), subsampling="420")
    with pytest.raises(ValueError):
        ops.jpeg_scan(torch.zeros(1, 16, 16, 3, dtype=torch.uint8), 90, None, "411")
    for bad in ("411", "4:2:0", 420):
        with pytest.raises(ValueError, match="jpeg_subsampling"):
            Imitator({"jpeg_subsampling": bad}, device=torch.device("cpu"))
