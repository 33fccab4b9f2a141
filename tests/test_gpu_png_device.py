"""The device PNG encoder on the GPU (csrc/png_deflate.hip, ops.png_deflate, output.FrameWriter(encoder="device")): every
comparison of a stream is BITWISE against tests/pngdev_emu.py, the definition, and every stream is decoded back to the input pixels.

  * sizes (H, W, rows): (5, 5, 16) one short segment; (20, 20, 8) segments of 8, 8 and 4 rows; (37, 53, 16) ragged, odd row length;
    (128, 128, 16); (64, 160, 32) whose second segment is the Fibonacci length-limit stream (tests/pngdev_emu.fib_frame) behind a noise segment;
    contents: constant, smooth, smooth + noise, uniform noise (every segment stored), all 256 residual values equally often;
  * a batch of three frames of different classes equals the same frames encoded alone, frame for frame;
  * one 512 x 512 and one 1024 x 1024 frame at 16 rows (the largest LDS footprint the engine uses), both compared bitwise: the emulator
    takes well under a second for either;
  * the largest segment the entry point accepts (65 533 raw bytes, 140 KB of LDS), dynamic and stored;
  * the entry point called on buffers with guard bytes: nothing behind nbytes[b] is written, in a frame's row or behind the last one;
  * FrameWriter(encoder="device") against encoder="host": same file names, same decoded pixels; Imitator.inference with
    opt.png_encoder = "device" at S = 128 writes files that decode to the frames the host path writes."""
import functools
import io
import os
import tempfile
import zlib

import numpy as np
import pytest
import torch

from ipercore_amd import _lib, ops, output
from tests import pngdev_emu as emu
from tests.gpu_checks import DEV

pytestmark = pytest.mark.gpu

SIZES = ((5, 5, 16), (20, 20, 8), (37, 53, 16), (128, 128, 16))


@functools.lru_cache(maxsize=None)
def _frame(kind, H, W, rows):
    img = emu.fib_frame() if kind == "fib" else emu.frame(kind, H, W, rows)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _want(kind, H, W, rows):
    return emu.stream(_frame(kind, H, W, rows), rows)


def _decode_png(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def _encode(imgs, rows):
    """ops.png_deflate on a list of equal-size frames -> the list of their streams (bytes)."""
    u8 = torch.from_numpy(np.stack(imgs)).to(DEV)
    streams, nbytes = ops.png_deflate(u8, rows)
    H, W = imgs[0].shape[:2]
    assert tuple(streams.shape) == (len(imgs), emu.capacity(H, W, min(rows, H))) and streams.dtype == torch.uint8
    assert tuple(nbytes.shape) == (len(imgs),) and nbytes.dtype == torch.int32
    s, n = streams.cpu().numpy(), nbytes.cpu().numpy()
    assert (n > 0).all() and (n <= s.shape[1]).all(), n
    return [s[i, :n[i]].tobytes() for i in range(len(imgs))]


def _check(got, img, want, rows):
    H, W, _ = img.shape
    print("frame %d x %d rows %d: %d bytes (definition %d, capacity %d)" % (H, W, rows, len(got), len(want), emu.capacity(H, W, min(rows, H))))
    assert len(got) == len(want), "nbytes differs from the definition"
    if got != want:
        at = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError("stream differs from the definition at byte %d of %d: %s != %s" % (at, len(want), got[at:at + 8].hex(), want[at:at + 8].hex()))
    assert zlib.decompress(got) == emu.paeth_filter(img).tobytes()
    assert np.array_equal(_decode_png(output.png_from_stream(got, W, H)), img)


@pytest.mark.parametrize("H,W,rows", SIZES)
@pytest.mark.parametrize("kind", emu.KINDS)
def test_stream_equals_the_definition(kind, H, W, rows):
    img = _frame(kind, H, W, rows)
    (got,) = _encode([img], rows)
    _check(got, img, _want(kind, H, W, rows), rows)


def test_length_limit_segment_behind_a_stored_one():
    img = _frame("fib", 64, 160, 32)
    raw = emu.paeth_filter(img)
    h1 = emu.segment_hist(raw[32:].tobytes())
    assert max(emu.huffman_depths(h1)) > 15 and max(emu.code_lengths(h1)) == 15         # the case is what it claims to be
    (got,) = _encode([img], 32)
    _check(got, img, _want("fib", 64, 160, 32), 32)


def test_batch_equals_frames_alone():
    kinds = ("smooth", "noise", "all256")
    imgs = [_frame(k, 37, 53, 16) for k in kinds]
    alone = [_encode([im], 16)[0] for im in imgs]
    batch = _encode(imgs, 16)
    for k, im, a, b in zip(kinds, imgs, alone, batch):
        assert a == b, "frame '%s' in a batch differs from the frame alone" % k
        _check(b, im, _want(k, 37, 53, 16), 16)


@pytest.mark.parametrize("S", [512, 1024])
def test_large_frame_bitwise(S):
    img = _frame("smooth_noise", S, S, 16)
    (got,) = _encode([img], 16)
    _check(got, img, _want("smooth_noise", S, S, 16), 16)


def test_largest_segment():
    """1 x 21 844 pixels in one row per segment: 65 533 raw bytes, the most LDS a launch can ask for; a smooth row (dynamic) and a noise row (stored)."""
    W = 21844
    rng = np.random.default_rng(11)
    img = np.empty((2, W, 3), np.uint8)
    img[0] = (np.arange(W)[:, None] // 97 + np.array([0, 40, 90])) % 256
    img[1] = rng.integers(0, 256, (W, 3), dtype=np.uint8)
    segs = emu.segment_list(emu.paeth_filter(img), 1)
    assert not emu.is_stored(segs[0]) and emu.is_stored(segs[1])
    (got,) = _encode([img], 1)
    _check(got, img, emu.stream(img, 1), 1)


def test_nothing_is_written_behind_nbytes():
    """The C entry point on buffers with guard bytes in front and behind, every output byte preset: a frame's row keeps its preset behind nbytes[b]."""
    H, W, rows, B, G = 37, 53, 16, 3, 256
    kinds = ("constant", "smooth_noise", "noise")
    imgs = [_frame(k, H, W, rows) for k in kinds]
    lib = _lib.lib()
    cap = lib.lwg_png_stream_capacity(H, W, rows)
    assert cap == emu.capacity(H, W, rows)
    u8 = torch.from_numpy(np.stack(imgs)).to(DEV)
    buf = torch.full((G + B * cap + G,), 0xA5, device=DEV, dtype=torch.uint8)
    nb = torch.full((4 + B + 4,), -77, device=DEV, dtype=torch.int32)
    ws = torch.empty(lib.lwg_png_deflate_ws_bytes(B, H, W, rows), device=DEV, dtype=torch.uint8)
    err = lib.lwg_png_deflate_u8(u8.data_ptr(), B, H, W, rows, ws.data_ptr(), buf.data_ptr() + G, nb.data_ptr() + 16, torch.cuda.current_stream().cuda_stream)
    assert err == 0
    torch.cuda.synchronize()
    buf, nb = buf.cpu().numpy(), nb.cpu().numpy()
    assert (buf[:G] == 0xA5).all() and (buf[G + B * cap:] == 0xA5).all(), "guard bytes around the streams were written"
    assert (nb[:4] == -77).all() and (nb[4 + B:] == -77).all(), "guard elements around nbytes were written"
    for b, k in enumerate(kinds):
        n = int(nb[4 + b])
        assert 0 < n <= cap
        row = buf[G + b * cap:G + (b + 1) * cap]
        assert (row[n:] == 0xA5).all(), "frame %d: bytes behind nbytes were written" % b
        _check(row[:n].tobytes(), imgs[b], _want(k, H, W, rows), rows)
    assert int(nb[4 + 2]) == cap                                           # the noise frame fills its row exactly


def test_frame_writer_device_equals_host():
    from PIL import Image
    g = torch.Generator().manual_seed(5)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, 128), torch.linspace(-1, 1, 128), indexing="ij")
    base = torch.stack([torch.sin(3 * xx) * yy, xx * yy, torch.cos(4 * xx + yy)])
    pred = (base[None] + 0.05 * torch.randn(5, 3, 128, 128, generator=g)).clamp(-1, 1).to(DEV)
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for enc in ("host", "device"):
            w = output.FrameWriter(os.path.join(d, enc), prefix="pred_", encoder=enc)
            w.submit(pred[:3], 0)
            w.submit(pred[3:], 3)
            paths = w.close()
            out[enc] = ([os.path.basename(p) for p in paths], [np.asarray(Image.open(p).convert("RGB")) for p in paths], [os.path.getsize(p) for p in paths])
    assert out["host"][0] == out["device"][0] == ["pred_{:0>8}.png".format(t) for t in range(5)]
    want = ops.frames_to_u8(pred).cpu().numpy()
    for t in range(5):
        assert np.array_equal(out["device"][1][t], want[t]) and np.array_equal(out["host"][1][t], want[t]), t
    print("file bytes host", out["host"][2], "device", out["device"][2])


def test_imitator_inference_with_the_device_encoder():
    from PIL import Image
    from tests import parity_utils as pu
    case = pu.build_case(image_size=128, num_filters=[64, 64, 128], n_res=2, bg_filters=[64, 64, 128], n_frames=5, ns=2)
    im = pu.make_imitator(case, frame_batch=3)
    assert im.png_encoder == "host"
    with tempfile.TemporaryDirectory() as d:
        host = im.inference(case.tgt_smpls, cam_strategy="smooth", output_dir=os.path.join(d, "host"), prefix="pred_")
        case.opt["png_encoder"] = "device"              # (an AttrDict: the mapping is what the runner reads)
        im2 = pu.make_imitator(case, frame_batch=3)
        assert im2.png_encoder == "device"
        dev = im2.inference(case.tgt_smpls, cam_strategy="smooth", output_dir=os.path.join(d, "device"), prefix="pred_")
        assert [os.path.basename(p) for p in dev] == [os.path.basename(p) for p in host] == ["pred_{:0>8}.png".format(t) for t in range(5)]
        for ph, pd in zip(host, dev):
            assert np.array_equal(np.asarray(Image.open(pd).convert("RGB")), np.asarray(Image.open(ph).convert("RGB"))), pd
            with open(pd, "rb") as fp:
                data = fp.read()
            i = data.index(b"IDAT")
            assert data[i + 4:i + 6] == b"\x78\x01" and data.count(b"IDAT") >= 1
