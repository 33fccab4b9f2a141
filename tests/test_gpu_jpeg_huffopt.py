"""The device JPEG encoder's per-frame Huffman tables on the GPU (csrc/jpeg_scan.hip lwg_jpeg_scan_opt_u8 / lwg_jpeg420_scan_opt_u8,
lwg_jpeg_hist_u8 / lwg_jpeg420_hist_u8, lwg_jpeg_huff_tables; ops.jpeg_scan(huffman="optimized"), ops.jpeg_symbol_histogram,
ops.jpeg_huffman_tables, output.FrameWriter(huffman="optimized"), opt.jpeg_huffman): every comparison is BITWISE against
tests/jpeghuff_emu.py, the definition.

  * the table kernel on the adversarial histograms of tests/test_jpeg_huffopt_cpu.py, all in one launch, each in all four table positions, in
    both output forms;
  * the symbol histograms, and scans, lengths and tables, on the grids of tests/test_jpeg_device_cpu.py and tests/test_jpeg420_cpu.py: sizes
    (1,1) .. (128,128), qualities 50 / 90 / 100, the five contents as one batch per launch, per size the restart intervals 1, one MCU row, one
    that does not divide the row and one that gives more than 8 segments;
  * a batch of three frames of different content equals the same frames encoded alone;
  * the largest restart interval on the checkerboard and on noise at quality 100, with a ragged last MCU column: the most LDS, many FF bytes;
  * one 512 x 512 frame per subsampling at the default interval;
  * the entry points on buffers with guard bytes;
  * FrameWriter(encoder="jpeg" | "mjpeg", huffman="optimized") at both subsamplings and Imitator.inference with opt.jpeg_huffman, alone and
    with the fused canvas; with the option absent the file of huffman="fixed"."""
import functools
import os
import tempfile

import numpy as np
import pytest
import torch

from ipercore_amd import _lib, ops, output
from tests import fusecanvas_emu
from tests import jpeg420_emu as emu420
from tests import jpegdev_emu as emu444
from tests import jpeghuff_emu as emu
from tests import test_jpeg420_cpu as grid420
from tests import test_jpeg_device_cpu as grid444
from tests.gpu_checks import DEV
from tests.test_gpu_jpeg420 import _check, _decode, _pred, _read, _run
from tests.test_jpeg_device_cpu import riff_frames
from tests.test_jpeg_huffopt_cpu import adversarial_histograms

pytestmark = pytest.mark.gpu

GRIDS = {"444": grid444, "420": grid420}
FIXED = {"444": emu444, "420": emu420}
SUBS = ("444", "420")


def _grid():
    for sub in SUBS:
        for H, W in GRIDS[sub].SIZES:
            for quality in GRIDS[sub].QUALITIES:
                yield sub, quality, H, W


@functools.lru_cache(maxsize=None)
def _frame(kind, H, W):
    img = emu.frame(kind, H, W)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _want(kind, H, W, quality, ri, sub):
    """-> (histogram, dht form, scan) of the definition."""
    img = _frame(kind, H, W)
    hist = emu.histogram(img, quality, ri, sub)
    specs = [emu.table(h) for h in hist]
    return hist, emu.dht(specs), emu.scan(img, quality, ri, sub, specs=specs)


def _most(sub):
    return ops.jpeg_max_mcus_per_segment(sub)


def _encode(imgs, quality, ri, sub):
    """ops.jpeg_scan(huffman="optimized") on a list of equal-size frames -> (their scans (bytes), their tables (4, 272) uint8)."""
    u8 = torch.from_numpy(np.stack(imgs)).to(DEV)
    scans, nbytes, tables = ops.jpeg_scan(u8, quality, ri, sub, huffman="optimized")
    H, W = imgs[0].shape[:2]
    assert tuple(scans.shape) == (len(imgs), emu.capacity(H, W, ri or min(emu.default_interval(W, sub), _most(sub)), sub)) and scans.dtype == torch.uint8
    assert tuple(nbytes.shape) == (len(imgs),) and nbytes.dtype == torch.int32
    assert tuple(tables.shape) == (len(imgs), 4, 272) and tables.dtype == torch.uint8
    n = nbytes.cpu().numpy()
    assert (n > 0).all() and (n <= scans.shape[1]).all(), n
    return [scans[i, :int(n[i])].cpu().numpy().tobytes() for i in range(len(imgs))], tables.cpu().numpy()


def _check_tables(got, want, what):
    assert got.shape == want.shape == (4, 272)
    if not (got == want).all():
        k = int(np.nonzero((got != want).any(axis=1))[0][0])
        raise AssertionError("%s: table %d differs from the definition: counts %s symbols %s != counts %s symbols %s"
                             % (what, k, got[k, :16].tolist(), got[k, 16:48].tolist(), want[k, :16].tolist(), want[k, 16:48].tolist()))


# ---- the table kernel alone -----------------------------------------------------------------------------------------------------------------------
def test_tables_of_adversarial_histograms():
    """Every histogram in each of the four table positions of a frame (the other three hold the next histograms), all frames in ONE launch."""
    hists = adversarial_histograms()
    names = sorted(hists)
    frames = [[names[(i + k) % len(names)] for k in range(4)] for i in range(len(names))]
    h = np.array([[hists[n] for n in f] for f in frames], dtype=np.uint64)
    assert h.shape == (len(names), 4, 256) and h.max() == 0xFFFFFFFF
    dev = torch.from_numpy(h.astype(np.uint32).view(np.int32)).to(DEV)
    tables, codes = ops.jpeg_huffman_tables(dev)
    assert tuple(tables.shape) == (len(names), 4, 272) and tables.dtype == torch.uint8
    assert tuple(codes.shape) == (len(names), 544) and codes.dtype == torch.int32
    tables, codes = tables.cpu().numpy(), codes.cpu().numpy().view(np.uint32)
    spec = {n: emu.table(hists[n]) for n in names}
    for b, f in enumerate(frames):
        specs = [spec[n] for n in f]
        _check_tables(tables[b], emu.dht(specs), "frame %d %r" % (b, f))
        want = emu.coder_words(specs)
        assert (codes[b] == want).all(), "frame %d %r: code words differ at %s" % (b, f, np.nonzero(codes[b] != want)[0][:8].tolist())
    torch.cuda.synchronize()


def test_tables_entry_point_writes_nothing_outside_its_outputs():
    hists = adversarial_histograms()
    names = ("256 ones", "fibonacci", "empty", "all 2^32 - 1")
    B, G = 2, 64
    h = np.array([[hists[n] for n in names], [hists[n] for n in names[::-1]]], dtype=np.uint64).astype(np.uint32)
    dev = torch.from_numpy(h.view(np.int32)).to(DEV)
    tables = torch.full((G + B * 4 * 272 + G,), 0xA5, device=DEV, dtype=torch.uint8)
    codes = torch.full((G + B * 544 + G,), -77, device=DEV, dtype=torch.int32)
    err = _lib.lib().lwg_jpeg_huff_tables(dev.data_ptr(), B, tables.data_ptr() + G, codes.data_ptr() + 4 * G, torch.cuda.current_stream().cuda_stream)
    assert err == 0
    torch.cuda.synchronize()
    tables, codes = tables.cpu().numpy(), codes.cpu().numpy()
    assert (tables[:G] == 0xA5).all() and (tables[-G:] == 0xA5).all() and (codes[:G] == -77).all() and (codes[-G:] == -77).all()
    for b, f in enumerate((names, names[::-1])):
        specs = [emu.table(hists[n]) for n in f]
        _check_tables(tables[G + b * 1088:G + (b + 1) * 1088].reshape(4, 272), emu.dht(specs), "frame %d" % b)
        assert (codes[G + b * 544:G + (b + 1) * 544].view(np.uint32) == emu.coder_words(specs)).all()


# ---- the grids ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub,quality,H,W", list(_grid()))
def test_histogram_equals_the_definition(sub, quality, H, W):
    u8 = torch.from_numpy(np.stack([_frame(kind, H, W) for kind in emu.KINDS])).to(DEV)
    for ri in GRIDS[sub].intervals(H, W):
        got = ops.jpeg_symbol_histogram(u8, quality, ri, sub)
        assert tuple(got.shape) == (len(emu.KINDS), 4, 256) and got.dtype == torch.int32
        got = got.cpu().numpy()
        for b, kind in enumerate(emu.KINDS):
            want = _want(kind, H, W, quality, ri, sub)[0]
            assert (got[b] == want).all(), "%s %s %d x %d quality %d interval %d: table %d differs" % (
                sub, kind, H, W, quality, ri, int(np.nonzero((got[b] != want).any(axis=1))[0][0]))


@pytest.mark.parametrize("sub,quality,H,W", list(_grid()))
def test_scan_and_tables_equal_the_definition(sub, quality, H, W):
    imgs = [_frame(kind, H, W) for kind in emu.KINDS]
    for ri in GRIDS[sub].intervals(H, W):
        scans, tables = _encode(imgs, quality, ri, sub)
        for b, kind in enumerate(emu.KINDS):
            what = "%s %s %d x %d quality %d interval %d" % (sub, kind, H, W, quality, ri)
            _, dht, scan = _want(kind, H, W, quality, ri, sub)
            _check_tables(tables[b], dht, what)
            _check(scans[b], scan, what)


@pytest.mark.parametrize("sub", SUBS)
def test_batch_equals_frames_alone(sub):
    kinds = ("smooth", "noise", "checker")
    imgs = [_frame(k, 17, 23) for k in kinds]
    alone = [_encode([im], 90, 2, sub) for im in imgs]
    scans, tables = _encode(imgs, 90, 2, sub)
    for b, k in enumerate(kinds):
        assert alone[b][0][0] == scans[b] and (alone[b][1][0] == tables[b]).all(), "frame '%s' in a batch differs from the frame alone" % k
        _check(scans[b], _want(k, 17, 23, 90, 2, sub)[2], k)
    assert len({t.tobytes() for t in tables}) == 3


@pytest.mark.parametrize("sub", SUBS)
def test_largest_segment_on_the_checkerboard_and_on_noise(sub):
    """The most MCUs a segment takes, quantiser 1, half an MCU missing on the right: the most LDS a launch uses, many FF bytes; segments span
    MCU rows and the last one is partial."""
    ri, side = _most(sub), ops.jpeg_mcu_size(sub)
    cols = (ri + 20 + 2) // 3
    H, W = 2 * side + side // 2, side * cols - side // 2
    assert FIXED[sub].geometry(H, W, ri) == (3, cols, 2) and W % 4 == 0
    for kind in ("checker", "noise"):
        img = _frame(kind, H, W)
        (got,), tables = _encode([img], 100, ri, sub)
        _, dht, want = _want(kind, H, W, 100, ri, sub)
        assert kind != "noise" or want.count(b"\xff\x00") > 40      # (the checkerboard's own tables leave it few FF bytes: 3 and 0)
        _check_tables(tables[0], dht, kind)
        _check(got, want, "%s %s at %d MCUs" % (sub, kind, ri))


@pytest.mark.parametrize("sub", SUBS)
def test_large_frame_bitwise(sub):
    S = 512
    img = _frame("smooth_noise", S, S)
    ri = min(emu.default_interval(S, sub), _most(sub))
    (got,), tables = _encode([img], 90, None, sub)
    hist = emu.histogram(img, 90, ri, sub)
    specs = [emu.table(h) for h in hist]
    assert (ops.jpeg_symbol_histogram(torch.from_numpy(np.array(img[None])).to(DEV), 90, None, sub).cpu().numpy()[0] == hist).all()
    _check_tables(tables[0], emu.dht(specs), "smooth_noise %d" % S)
    _check(got, emu.scan(img, 90, ri, sub, specs=specs), "smooth_noise %d" % S)
    own = output.jpeg_from_scan(got, S, S, 90, ri, sub, tables[0])
    fixed = FIXED[sub].file(img, 90, ri)
    assert len(own) < len(fixed) and (_decode(own) == _decode(fixed)).all()


@pytest.mark.parametrize("sub", SUBS)
def test_nothing_is_written_behind_nbytes_or_outside_the_tables(sub):
    H, W, ri, B, G = 17, 23, 2, 3, 256
    kinds = ("constant", "smooth_noise", "checker")
    lib = _lib.lib()
    prefix = "lwg_jpeg" if sub == "444" else "lwg_jpeg420"
    cap = getattr(lib, prefix + "_scan_opt_capacity")(H, W, ri)
    assert cap == emu.capacity(H, W, ri, sub)
    u8 = torch.from_numpy(np.stack([_frame(k, H, W) for k in kinds])).to(DEV)
    buf = torch.full((G + B * cap + G,), 0xA5, device=DEV, dtype=torch.uint8)
    nb = torch.full((4 + B + 4,), -77, device=DEV, dtype=torch.int32)
    tb = torch.full((G + B * 1088 + G,), 0x5A, device=DEV, dtype=torch.uint8)
    ws = torch.empty(getattr(lib, prefix + "_scan_opt_ws_bytes")(B, H, W, ri), device=DEV, dtype=torch.uint8)
    qt = output.jpeg_tables(100)
    err = getattr(lib, prefix + "_scan_opt_u8")(u8.data_ptr(), B, H, W, bytes(qt[0]) + bytes(qt[1]), ri, ws.data_ptr(), buf.data_ptr() + G,
                                                nb.data_ptr() + 16, tb.data_ptr() + G, torch.cuda.current_stream().cuda_stream)
    assert err == 0
    torch.cuda.synchronize()
    buf, nb, tb = buf.cpu().numpy(), nb.cpu().numpy(), tb.cpu().numpy()
    assert (buf[:G] == 0xA5).all() and (buf[G + B * cap:] == 0xA5).all(), "guard bytes around the scans were written"
    assert (nb[:4] == -77).all() and (nb[4 + B:] == -77).all(), "guard elements around nbytes were written"
    assert (tb[:G] == 0x5A).all() and (tb[G + B * 1088:] == 0x5A).all(), "guard bytes around the tables were written"
    for b, k in enumerate(kinds):
        n = int(nb[4 + b])
        assert 0 < n <= cap
        row = buf[G + b * cap:G + (b + 1) * cap]
        assert (row[n:] == 0xA5).all(), "frame %d: bytes behind nbytes were written" % b
        _, dht, want = _want(k, H, W, 100, ri, sub)
        _check(row[:n].tobytes(), want, k)
        _check_tables(tb[G + b * 1088:G + (b + 1) * 1088].reshape(4, 272), dht, k)


# ---- the writer and the runner --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", SUBS)
def test_frame_writer_jpeg_and_mjpeg(sub):
    pred = _pred()
    u8 = ops.frames_to_u8(pred).cpu().numpy()
    ri = emu.default_interval(128, sub)
    want = [emu.file(u8[t], 90, ri, sub) for t in range(5)]
    fixed = [FIXED[sub].file(u8[t], 90, ri) for t in range(5)]
    with tempfile.TemporaryDirectory() as d:
        paths = {}
        for enc in ("jpeg", "mjpeg"):
            w = output.FrameWriter(os.path.join(d, enc), prefix="pred_", encoder=enc, fps=30, subsampling=sub, huffman="optimized")
            w.submit(pred[:3], 0)
            w.submit(pred[3:], 3)
            paths[enc] = w.close()
        assert [os.path.basename(p) for p in paths["jpeg"]] == ["pred_{:0>8}.jpg".format(t) for t in range(5)]
        files = [_read(p) for p in paths["jpeg"]]
        for t in range(5):
            assert files[t] == want[t], "file %d differs from the emulator's" % t
            assert len(files[t]) < len(fixed[t]) and (_decode(files[t]) == _decode(fixed[t])).all()
        assert paths["mjpeg"] == [os.path.join(d, "mjpeg", "pred_video.avi")] and os.listdir(os.path.join(d, "mjpeg")) == ["pred_video.avi"]
        info = riff_frames(_read(paths["mjpeg"][0]))
        assert info["frames"] == files and (info["width"], info["height"], info["total"], info["usec"]) == (128, 128, 5, 33333)


def test_imitator_inference_honours_jpeg_huffman():
    from tests.test_gpu_fuse_video import _clip
    case, u8, _, pan, refs = _clip()                     # S = 128, five frames in batches of three; u8: ops.frames_to_u8's bytes
    want = [emu.file(u8[t], 90, 16) for t in range(5)]
    canvas = fusecanvas_emu.canvas(pan, refs, [u8], 10, 0)
    Wc = canvas.shape[2]
    want_fused = [emu.file(c, 90, min((Wc + 7) // 8, _most("444"))) for c in canvas]
    with tempfile.TemporaryDirectory() as d:
        opt = type(case.opt)(case.opt)
        opt.update(output_format="jpeg", jpeg_huffman="optimized")
        im, jpg = _run(case, opt, os.path.join(d, "jpeg"))
        assert im.jpeg_huffman == "optimized"
        assert [os.path.basename(p) for p in jpg] == ["pred_{:0>8}.jpg".format(t) for t in range(5)]
        assert [_read(p) for p in jpg] == want
        opt["fuse_output"] = "src_ref_out"
        im, jpg = _run(case, opt, os.path.join(d, "fused"), ref_imgs=refs)
        assert [_read(p) for p in jpg] == want
        info = riff_frames(_read(im.fused_video_path))
        assert (info["width"], info["height"], info["total"]) == (Wc, 128, 5)
        for t in range(5):
            assert info["frames"][t] == want_fused[t], t
        # "png" ignores the option
        opt = type(case.opt)(case.opt)
        opt["jpeg_huffman"] = "optimized"
        _, png = _run(case, opt, os.path.join(d, "png"))
        assert [os.path.basename(p) for p in png] == ["pred_{:0>8}.png".format(t) for t in range(5)]
        # the option absent: the file of huffman = "fixed" given explicitly, which is the fixed-table emulator's
        opt = type(case.opt)(case.opt)
        opt["output_format"] = "jpeg"
        im, absent = _run(case, opt, os.path.join(d, "absent"))
        assert im.jpeg_huffman == "fixed"
        opt["jpeg_huffman"] = "fixed"
        _, given = _run(case, opt, os.path.join(d, "given"))
        assert [_read(p) for p in absent] == [_read(p) for p in given] == [emu444.file(u8[t], 90, 16) for t in range(5)]
        w = output.FrameWriter(os.path.join(d, "writer"), prefix="pred_", encoder="jpeg", huffman="fixed")
        w.submit(torch.from_numpy(np.stack(im.inference(case.tgt_smpls, cam_strategy="smooth"))).to(DEV), 0)
        assert [_read(p) for p in w.close()] == [_read(p) for p in absent]
    with pytest.raises(ValueError):
        opt["jpeg_huffman"] = "optimised"
        _run(case, opt, "")
