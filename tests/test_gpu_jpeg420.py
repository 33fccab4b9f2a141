"""The device JPEG encoder's 4:2:0 format on the GPU (csrc/jpeg_scan.hip lwg_jpeg420_scan_u8, ops.jpeg_scan(subsampling="420"),
output.FrameWriter(subsampling="420"), opt.jpeg_subsampling): every comparison of a scan is BITWISE against
tests/jpeg420_emu.py, the definition, lengths included.

  * the grid of tests/test_jpeg420_cpu.py: sizes (1,1) .. (128,128), qualities 50 / 90 / 100, the five contents as one batch per launch, and
    per size the restart intervals one MCU row, 1, one that does not divide the row, and one that gives more than 8 segments;
  * a batch of three frames of different content equals the same frames encoded alone;
  * one 512 x 512 frame at the default segment (32 MCUs: an MCU row);
  * the largest restart interval the entry point accepts, on a frame whose last MCU column is ragged, on the 0/255 checkerboard and on
    noise at quality 100: the most LDS, the longest codes, many FF bytes;
  * the entry point on buffers with guard bytes: nothing behind nbytes[b] is written, in a frame's row or behind the last one;
  * FrameWriter(encoder="jpeg" | "mjpeg", subsampling="420"): today's file names, files equal to the emulator's, the AVI's chunks are those
    files; Imitator.inference with opt.jpeg_subsampling = "420" at S = 128, alone and with the fused canvas (340 pixels wide: a ragged
    right MCU column), and with the option absent the file of subsampling="444" given explicitly."""
import functools
import io
import os
import tempfile

import numpy as np
import pytest
import torch

from ipercore_amd import _lib, ops, output
from tests import fusecanvas_emu
from tests import jpeg420_emu as emu
from tests.gpu_checks import DEV
from tests.test_jpeg420_cpu import QUALITIES, SIZES, intervals
from tests.test_jpeg_device_cpu import riff_frames

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _frame(kind, H, W):
    img = emu.frame(kind, H, W)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _want(kind, H, W, quality, ri):
    return emu.scan(_frame(kind, H, W), quality, ri)


def _decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    assert im.mode == "RGB"
    return np.asarray(im)


def _most():
    return ops.jpeg_max_mcus_per_segment("420")


def _encode(imgs, quality, ri):
    """ops.jpeg_scan(subsampling="420") on a list of equal-size frames -> the list of their scans (bytes)."""
    u8 = torch.from_numpy(np.stack(imgs)).to(DEV)
    scans, nbytes = ops.jpeg_scan(u8, quality, ri, subsampling="420")
    H, W = imgs[0].shape[:2]
    assert tuple(scans.shape) == (len(imgs), emu.capacity(H, W, ri or min((W + 15) // 16, _most()))) and scans.dtype == torch.uint8
    assert tuple(nbytes.shape) == (len(imgs),) and nbytes.dtype == torch.int32
    n = nbytes.cpu().numpy()
    assert (n > 0).all() and (n <= scans.shape[1]).all(), n
    return [scans[i, :int(n[i])].cpu().numpy().tobytes() for i in range(len(imgs))]


def _check(got, want, what):
    if got != want:
        at = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
        raise AssertionError("%s: scan of %d bytes (definition %d) differs from the definition at byte %d: %s != %s"
                             % (what, len(got), len(want), at, got[at:at + 8].hex(), want[at:at + 8].hex()))


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("quality", QUALITIES)
def test_scan_equals_the_definition(quality, H, W):
    for ri in intervals(H, W):
        imgs = [_frame(kind, H, W) for kind in emu.KINDS]
        for kind, got in zip(emu.KINDS, _encode(imgs, quality, ri)):
            _check(got, _want(kind, H, W, quality, ri), "%s %d x %d quality %d interval %d" % (kind, H, W, quality, ri))


def test_batch_equals_frames_alone():
    kinds = ("smooth", "noise", "checker")
    imgs = [_frame(k, 17, 23) for k in kinds]
    alone = [_encode([im], 90, 2)[0] for im in imgs]
    for k, a, b in zip(kinds, alone, _encode(imgs, 90, 2)):
        assert a == b, "frame '%s' in a batch differs from the frame alone" % k
        _check(b, _want(k, 17, 23, 90, 2), k)


def test_large_frame_bitwise():
    S = 512
    img = _frame("smooth_noise", S, S)
    (got,) = _encode([img], 90, None)
    assert _most() >= 32
    _check(got, emu.scan(img, 90, 32), "smooth_noise %d" % S)
    assert _decode(output.jpeg_from_scan(got, S, S, 90, 32, "420")).shape == (S, S, 3)


def test_largest_segment_on_the_checkerboard_and_on_noise():
    """The most MCUs a segment takes, every pixel 0 or 255, quantiser 1: the largest coefficients, the longest codes, many FF bytes - the most
    LDS a launch uses.  3 x ceil((R + 20) / 3) MCUs with half an MCU missing on the right: segments span MCU rows, the last one is partial."""
    ri = _most()
    cols = (ri + 20 + 2) // 3
    H, W = 40, 16 * cols - 8
    assert emu.geometry(H, W, ri) == (3, cols, 2) and W % 4 == 0
    img = _frame("checker", H, W)
    (got,) = _encode([img], 100, ri)
    want = emu.scan(img, 100, ri)
    assert want.count(b"\xff\x00") > 100
    _check(got, want, "checker at %d MCUs" % ri)
    noise = _frame("noise", H, W)
    want = emu.scan(noise, 100, ri)
    assert want.count(b"\xff\x00") > 100
    _check(_encode([noise], 100, ri)[0], want, "noise at %d MCUs" % ri)


def test_nothing_is_written_behind_nbytes():
    """The C entry point on buffers with guard bytes in front and behind, every output byte preset: a frame's row keeps its preset behind nbytes[b]."""
    H, W, ri, B, G = 17, 23, 2, 3, 256
    kinds = ("constant", "smooth_noise", "checker")
    imgs = [_frame(k, H, W) for k in kinds]
    lib = _lib.lib()
    cap = lib.lwg_jpeg420_scan_capacity(H, W, ri)
    assert cap == emu.capacity(H, W, ri)
    u8 = torch.from_numpy(np.stack(imgs)).to(DEV)
    buf = torch.full((G + B * cap + G,), 0xA5, device=DEV, dtype=torch.uint8)
    nb = torch.full((4 + B + 4,), -77, device=DEV, dtype=torch.int32)
    ws = torch.empty(lib.lwg_jpeg420_scan_ws_bytes(B, H, W, ri), device=DEV, dtype=torch.uint8)
    qt = output.jpeg_tables(100)
    err = lib.lwg_jpeg420_scan_u8(u8.data_ptr(), B, H, W, bytes(qt[0]) + bytes(qt[1]), ri, ws.data_ptr(), buf.data_ptr() + G, nb.data_ptr() + 16,
                                  torch.cuda.current_stream().cuda_stream)
    assert err == 0
    torch.cuda.synchronize()
    buf, nb = buf.cpu().numpy(), nb.cpu().numpy()
    assert (buf[:G] == 0xA5).all() and (buf[G + B * cap:] == 0xA5).all(), "guard bytes around the scans were written"
    assert (nb[:4] == -77).all() and (nb[4 + B:] == -77).all(), "guard elements around nbytes were written"
    for b, k in enumerate(kinds):
        n = int(nb[4 + b])
        assert 0 < n <= cap
        row = buf[G + b * cap:G + (b + 1) * cap]
        assert (row[n:] == 0xA5).all(), "frame %d: bytes behind nbytes were written" % b
        _check(row[:n].tobytes(), _want(k, H, W, 100, ri), k)


def _pred(n=5, S=128):
    g = torch.Generator().manual_seed(5)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, S), torch.linspace(-1, 1, S), indexing="ij")
    base = torch.stack([torch.sin(3 * xx) * yy, xx * yy, torch.cos(4 * xx + yy)])
    return (base[None] + 0.05 * torch.randn(n, 3, S, S, generator=g)).clamp(-1, 1).to(DEV)


def test_frame_writer_jpeg_and_mjpeg():
    pred = _pred()
    u8 = ops.frames_to_u8(pred).cpu().numpy()
    want = [emu.file(u8[t], 90, 8) for t in range(5)]
    with tempfile.TemporaryDirectory() as d:
        paths = {}
        for enc in ("jpeg", "mjpeg"):
            w = output.FrameWriter(os.path.join(d, enc), prefix="pred_", encoder=enc, fps=30, subsampling="420")
            w.submit(pred[:3], 0)
            w.submit(pred[3:], 3)
            paths[enc] = w.close()
        assert [os.path.basename(p) for p in paths["jpeg"]] == ["pred_{:0>8}.jpg".format(t) for t in range(5)]
        files = []
        for t, p in enumerate(paths["jpeg"]):
            with open(p, "rb") as fp:
                files.append(fp.read())
            assert files[t] == want[t], "file %d differs from the emulator's" % t
            assert _decode(files[t]).shape == (128, 128, 3)
        assert paths["mjpeg"] == [os.path.join(d, "mjpeg", "pred_video.avi")] and os.listdir(os.path.join(d, "mjpeg")) == ["pred_video.avi"]
        with open(paths["mjpeg"][0], "rb") as fp:
            info = riff_frames(fp.read())
        assert info["frames"] == files and (info["width"], info["height"], info["total"], info["usec"]) == (128, 128, 5, 33333)


def _run(case, opt, out, **kw):
    from tests import parity_utils as pu
    im = pu.make_imitator(type(case)(case, opt=opt), frame_batch=3)
    paths = im.inference(case.tgt_smpls, cam_strategy="smooth", output_dir=out, prefix="pred_", **kw)
    return im, paths


def _read(path):
    with open(path, "rb") as fp:
        return fp.read()


def test_imitator_inference_honours_jpeg_subsampling():
    from tests.test_gpu_fuse_video import _clip
    case, u8, _, pan, refs = _clip()                     # S = 128, five frames in batches of three; u8: ops.frames_to_u8's bytes
    want = [emu.file(u8[t], 90, 8) for t in range(5)]
    canvas = fusecanvas_emu.canvas(pan, refs, [u8], 10, 0)
    Wc = canvas.shape[2]
    assert Wc == 340 and Wc % 16 != 0
    want_fused = [emu.file(c, 90, min((Wc + 15) // 16, _most())) for c in canvas]
    with tempfile.TemporaryDirectory() as d:
        opt = type(case.opt)(case.opt)
        opt.update(output_format="jpeg", jpeg_subsampling="420")
        im, jpg = _run(case, opt, os.path.join(d, "jpeg"))
        assert im.jpeg_subsampling == "420"
        assert [os.path.basename(p) for p in jpg] == ["pred_{:0>8}.jpg".format(t) for t in range(5)]
        for t, p in enumerate(jpg):
            assert _read(p) == want[t], p
            assert _decode(want[t]).shape == (128, 128, 3)
        opt["fuse_output"] = "src_ref_out"
        im, jpg = _run(case, opt, os.path.join(d, "fused"), ref_imgs=refs)
        assert [_read(p) for p in jpg] == want
        assert im.fused_video_path == os.path.join(d, "fused", "pred_fused.avi")
        info = riff_frames(_read(im.fused_video_path))
        assert (info["width"], info["height"], info["total"]) == (Wc, 128, 5)
        for t in range(5):
            assert info["frames"][t] == want_fused[t], t
        assert _decode(info["frames"][0]).shape == (128, Wc, 3)
        # "png" ignores the option
        opt = type(case.opt)(case.opt)
        opt["jpeg_subsampling"] = "420"
        _, png = _run(case, opt, os.path.join(d, "png"))
        assert [os.path.basename(p) for p in png] == ["pred_{:0>8}.png".format(t) for t in range(5)]
        # the option absent: the file of subsampling = "444" given explicitly
        opt = type(case.opt)(case.opt)
        opt["output_format"] = "mjpeg"
        im, absent = _run(case, opt, os.path.join(d, "absent"))
        assert im.jpeg_subsampling == "444"
        opt["jpeg_subsampling"] = "444"
        _, given = _run(case, opt, os.path.join(d, "given"))
        assert _read(absent[0]) == _read(given[0])
        w = output.FrameWriter(os.path.join(d, "writer"), prefix="pred_", encoder="mjpeg", subsampling="444")
        w.submit(torch.from_numpy(np.stack(im.inference(case.tgt_smpls, cam_strategy="smooth"))).to(DEV), 0)
        assert _read(w.close()[0]) == _read(absent[0])
    with pytest.raises(ValueError):
        opt["jpeg_subsampling"] = "411"
        _run(case, opt, "")
