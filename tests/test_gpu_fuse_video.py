"""The fused source | reference | output video on the device: lwg_fuse_sources_u8 and lwg_fuse_canvas_u8 bitwise against
tests/fusecanvas_emu.py, output.FrameWriter(fuse=...) through all four encoders, and Imitator / Viewer with opt.fuse_output.

Canvas grid: S in (4, 8, 20, 36) x ns in (1, 2, 8) x pad in (0, 1, 2, 3, 10) x reference yes / no x n_out in (1, 2, 4) x B in (1, 3) x pad_val
in (0, 255); every region is filled with bytes that encode (region, column, row, channel), so a misplaced byte names where it came from.
3 Wc % 4 != 0 for most of the grid (S = 4, ns = 1, pad = 1, one output, no reference: rows of 27 bytes), so region seams and row starts fall at
every byte alignment.  Outside the grid: odd S (ns = 1: one pixel per item, a batch that ends in a partial word) and output tensors that are
4- but not 16-byte aligned."""
import functools
import os
import tempfile

import numpy as np
import pytest
import torch

from ipercore_amd import _lib, ops, output
from tests import fusecanvas_emu as emu
from tests import jpegdev_emu
from tests.gpu_checks import DEV
from tests.test_fuse_video_cpu import CANVAS_NS, CANVAS_S, N_OUTS, PADS, PANEL_S, as_source, panel_ok
from tests.test_jpeg_device_cpu import riff_frames

pytestmark = pytest.mark.gpu


def _sources(ns, S, seed=0):
    r = np.random.RandomState(seed + 31 * ns + S)
    return as_source(r.randint(0, 256, size=(ns, S, S, 3)).astype(np.uint8))


def _coded(region, n, S, W):
    """(n,S,W,3) uint8 whose bytes encode (region, frame, row, column, channel)."""
    b, y, x, c = np.meshgrid(np.arange(n), np.arange(S), np.arange(W), np.arange(3), indexing="ij")
    return ((37 * region + 101 * b + 11 * y + 3 * x + 5 * c + 1) % 251).astype(np.uint8)


def _as_pred(u8):
    """(B,S,S,3) uint8 -> (B,3,S,S) fp32 that lwg_frames_to_u8 turns back into exactly these bytes (level + 1/2 before the truncation)."""
    x = (u8.astype(np.float32) + np.float32(0.5)) / np.float32(127.5) - np.float32(1)
    pred = np.ascontiguousarray(x.transpose(0, 3, 1, 2))
    assert np.array_equal(emu.frames_u8(pred), u8)
    return pred


# ---- the source panel ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", PANEL_S)
def test_panel_equals_the_definition(S):
    for ns in range(1, 10):
        src = _sources(ns, S)
        if not panel_ok(ns, S):
            with pytest.raises(ValueError):
                ops.fuse_source_panel(torch.from_numpy(src).to(DEV))
            continue
        got = ops.fuse_source_panel(torch.from_numpy(src).to(DEV))
        want = emu.panel(src)
        assert tuple(got.shape) == want.shape and got.dtype == torch.uint8
        assert np.array_equal(got.cpu().numpy(), want), "ns = %d" % ns
        assert np.array_equal(ops.fuse_source_panel(torch.from_numpy(src[None]).to(DEV)).cpu().numpy(), want)          # src_info["img"]'s shape


def _ties():
    """fp32 inputs whose (x + 1) * 127.5 is EXACTLY k + 1/2 in fp32 arithmetic, found by a walk over the neighbours of (k + 1/2) / 127.5 - 1."""
    out = []
    for k in range(255):
        x = np.float32((k + 0.5) / 127.5 - 1)
        lo = hi = x
        for _ in range(64):
            for cand in (lo, hi):
                if (cand + np.float32(1)) * np.float32(127.5) == np.float32(k + 0.5):
                    out.append(cand)
                    break
            else:
                lo, hi = np.nextafter(lo, np.float32(-2)), np.nextafter(hi, np.float32(2))
                continue
            break
    return np.array(out, dtype=np.float32)


def test_panel_values_levels_ties_and_out_of_range():
    levels = (np.arange(256, dtype=np.float32) / 255.0 * 2 - 1).astype(np.float32)
    ties = _ties()
    assert ties.size >= 64 and np.float32(0) in ties                  # 127.5 -> 128, ties to even
    odd = np.array([1.5, -1.5, np.nan, np.inf, -np.inf, 1.0, -1.0, 3e38, -3e38], dtype=np.float32)
    vals = np.concatenate([levels, ties, odd])
    S = 32
    r = np.random.RandomState(4)
    src = vals[r.randint(0, vals.size, size=(4, 3, S, S))]
    src[0, 0].reshape(-1)[:vals.size] = vals                          # every value at least once, unmixed in the ns = 1 panel
    want_levels = emu.src_u8(vals)
    assert np.array_equal(want_levels[:256], np.arange(256)) and want_levels[256 + ties.size:].tolist() == [255, 0, 0, 255, 0, 255, 0, 255, 0]
    even = want_levels[256:256 + ties.size]
    assert (even % 2 == 0).all()
    for ns in (1, 2, 4):
        got = ops.fuse_source_panel(torch.from_numpy(src[:ns]).to(DEV)).cpu().numpy()
        assert np.array_equal(got, emu.panel(src[:ns])), "ns = %d" % ns
        if ns == 1:
            assert np.array_equal(got[..., 0].reshape(-1)[:vals.size], want_levels)


# ---- the canvas ---------------------------------------------------------------------------------------------------------------------------------
def _canvas_inputs(S, ns, B=3, n_out=4):
    Wp = emu.layout(ns, S)[0]
    panel = _coded(0, 1, S, Wp)[0]
    refs = _coded(2, B, S, S)
    outs = [_coded(3 + k, B, S, S) for k in range(n_out)]
    return panel, refs, outs


@pytest.mark.parametrize("S", CANVAS_S)
def test_canvas_equals_the_definition_on_the_grid(S):
    ragged = 0
    for ns in CANVAS_NS:
        if not panel_ok(ns, S):
            continue
        panel, refs, outs = _canvas_inputs(S, ns)
        panel_d, refs_d = torch.from_numpy(panel).to(DEV), torch.from_numpy(refs).to(DEV)
        preds_d = [torch.from_numpy(_as_pred(o)).to(DEV) for o in outs]
        for pad in PADS:
            for ref in (True, False):
                for n_out in N_OUTS:
                    for B in (1, 3):
                        for pad_val in (0, 255):
                            got = ops.fuse_canvas(panel_d, refs_d[:B] if ref else None, [p[:B] for p in preds_d[:n_out]], pad, pad_val)
                            want = emu.canvas(panel, refs[:B] if ref else None, [o[:B] for o in outs[:n_out]], pad, pad_val)
                            assert tuple(got.shape) == want.shape
                            g = got.cpu().numpy()
                            if not np.array_equal(g, want):
                                bad = np.argwhere(g != want)[0]
                                raise AssertionError("S %d ns %d pad %d ref %s n_out %d B %d pad_val %d: first wrong byte at (b, y, x, c) = %s: %d, want %d"
                                                     % (S, ns, pad, ref, n_out, B, pad_val, bad.tolist(), g[tuple(bad)], want[tuple(bad)]))
                            ragged += (3 * want.shape[2]) % 4 != 0
    assert ragged > 0
    if S == 4:
        assert emu.canvas_width(4, 4, 1, False, 1) * 3 == 27


WILD = np.array([3.0, -3.0, 1.0000001, -1.0000001, 1e10, -1e10, np.nan, np.inf, -np.inf, 0.999, 1.004, 1.01, -1.01, 255.0, 300.7], dtype=np.float32)


@pytest.mark.parametrize("S,off", ((20, 0), (36, 0), (20, 1), (5, 0), (7, 3)))
def test_out_regions_are_frames_to_u8_for_any_value(S, off):
    """In range and far out of it (the conversion of 300.7 wraps, NaN and the infinities go where the instruction puts them): the bytes of
    lwg_frames_to_u8 on the same tensors.  off: floats between a 16-byte boundary and the tensor (the one-pixel-per-item path, as odd S)."""
    B, n_out, pad = 2, 2, 3
    r = np.random.RandomState(S + off)
    preds = []
    for k in range(n_out):
        x = r.uniform(-1.2, 1.2, size=(B, 3, S, S)).astype(np.float32)
        idx = r.randint(0, x.size, size=x.size // 4)
        x.reshape(-1)[idx] = WILD[r.randint(0, WILD.size, size=idx.size)]
        buf = torch.zeros(x.size + 8, dtype=torch.float32, device=DEV)
        t = buf[off:off + x.size].view(B, 3, S, S)
        t.copy_(torch.from_numpy(x))
        assert t.data_ptr() % 16 == (4 * off) % 16
        preds.append(t)
    Wp = S
    panel = _coded(0, 1, S, Wp)[0]
    refs = _coded(2, B, S, S)
    got = ops.fuse_canvas(torch.from_numpy(panel).to(DEV), torch.from_numpy(refs).to(DEV), preds, pad, 7).cpu().numpy()
    u8 = [ops.frames_to_u8(p).cpu().numpy() for p in preds]
    assert np.array_equal(got, emu.canvas(panel, refs, u8, pad, 7))
    x0 = Wp + 2 * (S + pad) + pad
    assert np.array_equal(got[:, :, x0:x0 + S], u8[1])


def test_a_frame_in_a_batch_is_the_frame_alone():
    S, ns, B = 20, 2, 5
    panel, refs, outs = _canvas_inputs(S, ns, B=B, n_out=2)
    panel_d, refs_d = torch.from_numpy(panel).to(DEV), torch.from_numpy(refs).to(DEV)
    preds_d = [torch.from_numpy(_as_pred(o)).to(DEV) for o in outs]
    whole = ops.fuse_canvas(panel_d, refs_d, preds_d, 1, 9)
    assert (3 * whole.shape[2]) % 4 != 0
    for b in range(B):
        alone = ops.fuse_canvas(panel_d, refs_d[b:b + 1], [p[b:b + 1] for p in preds_d], 1, 9)
        assert torch.equal(alone[0], whole[b]), b


@pytest.mark.parametrize("S,ns,pad,ref,n_out,B", ((4, 1, 1, False, 1, 1), (5, 1, 1, True, 1, 1), (7, 1, 2, False, 2, 3), (20, 2, 3, True, 4, 3), (36, 8, 10, True, 1, 2)))
def test_nothing_is_written_outside_the_canvas(S, ns, pad, ref, n_out, B):
    import ctypes
    panel, refs, outs = _canvas_inputs(S, ns, B=B, n_out=n_out)
    Wp = panel.shape[1]
    want = emu.canvas(panel, refs if ref else None, outs, pad, 200)
    N, G = want.size, 64
    panel_d, refs_d = torch.from_numpy(panel).to(DEV), torch.from_numpy(refs).to(DEV)
    preds_d = [torch.from_numpy(_as_pred(o)).to(DEV) for o in outs]
    buf = torch.full((G + N + G,), 0xA5, dtype=torch.uint8, device=DEV)
    ptrs = (ctypes.c_void_p * n_out)(*[p.data_ptr() for p in preds_d])
    err = _lib.lib().lwg_fuse_canvas_u8(panel_d.data_ptr(), Wp, refs_d.data_ptr() if ref else None, ptrs, n_out, B, S, pad, 200, buf.data_ptr() + G, ops._stream())
    assert err == 0
    h = buf.cpu().numpy()
    assert (h[:G] == 0xA5).all() and (h[G + N:] == 0xA5).all(), "bytes outside the canvas were written"
    assert np.array_equal(h[G:G + N], want.reshape(-1))
    if S in (5, 7):
        assert N % 4 != 0 or S == 7                                   # (S = 5: 165 bytes - the batch ends in a partial word)


# ---- the writer ---------------------------------------------------------------------------------------------------------------------------------
def _pred(n=5, S=64, seed=5):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, S), torch.linspace(-1, 1, S), indexing="ij")
    base = torch.stack([torch.sin(3 * xx) * yy, xx * yy, torch.cos(4 * xx + yy)])
    return (base[None] + 0.05 * torch.randn(n, 3, S, S, generator=g)).clamp(-1, 1).to(DEV)


def _jpeg(canvas_hwc, quality=90):
    H, W = canvas_hwc.shape[:2]
    ri = min((W + 7) // 8, 64)
    return output.jpeg_from_scan(jpegdev_emu.scan(canvas_hwc, quality, ri), W, H, quality, ri)


def test_frame_writer_fuse_through_every_encoder():
    from PIL import Image
    S, n = 64, 5
    src = _sources(2, S)
    pred, pred2 = _pred(n, S), _pred(n, S, seed=6)
    refs = np.random.RandomState(8).randint(0, 256, size=(n, S, S, 3)).astype(np.uint8)
    panel_d = ops.fuse_source_panel(torch.from_numpy(src).to(DEV))
    u8, u8b = ops.frames_to_u8(pred).cpu().numpy(), ops.frames_to_u8(pred2).cpu().numpy()
    want = emu.canvas(emu.panel(src), refs, [u8], 10, 0)
    Wc = want.shape[2]
    assert Wc == 32 + 2 * 74
    files = [_jpeg(want[t]) for t in range(n)]
    refs_d = torch.from_numpy(refs).to(DEV)
    with tempfile.TemporaryDirectory() as d:
        paths = {}
        for enc in ("host", "device", "jpeg", "mjpeg"):
            w = output.FrameWriter(os.path.join(d, enc), prefix="pred_", encoder=enc, fps=30, fuse=output.FuseSpec(panel_d), video_name="fused.avi")
            w.submit(pred[:3], 0, ref=refs_d[:3])
            w.submit(pred[3:], 3, ref=refs[3:])                       # host frames: uploaded on the writer's copy stream
            paths[enc] = w.close()
        for enc in ("host", "device"):
            assert [os.path.basename(p) for p in paths[enc]] == ["pred_{:0>8}.png".format(t) for t in range(n)]
            for t, p in enumerate(paths[enc]):
                im = Image.open(p)
                assert im.size == (Wc, S) and np.array_equal(np.asarray(im.convert("RGB")), want[t]), p
        for t, p in enumerate(paths["jpeg"]):
            with open(p, "rb") as fp:
                assert fp.read() == files[t], p
        assert paths["mjpeg"] == [os.path.join(d, "mjpeg", "pred_fused.avi")]
        with open(paths["mjpeg"][0], "rb") as fp:
            info = riff_frames(fp.read())
        assert info["frames"] == files and (info["width"], info["height"], info["total"], info["usec"]) == (Wc, S, n, 33333)
        # no reference, a second output behind the first, other pads
        w = output.FrameWriter(os.path.join(d, "two"), encoder="mjpeg", fuse=output.FuseSpec(panel_d, pad=3, pad_val=255, with_ref=False))
        w.submit(pred, 0, more=(pred2,))
        with open(w.close()[0], "rb") as fp:
            info = riff_frames(fp.read())
        want2 = emu.canvas(emu.panel(src), None, [u8, u8b], 3, 255)
        assert info["frames"] == [_jpeg(want2[t]) for t in range(n)] and info["width"] == 32 + 2 * 67
        w = output.FrameWriter(os.path.join(d, "bad"), encoder="mjpeg", fuse=output.FuseSpec(panel_d))
        try:
            with pytest.raises(ValueError):
                w.submit(pred, 0)                                     # the spec shows a reference frame and none was given
        finally:
            assert w.close() == []


def test_png_rows_per_segment_follows_the_canvas_width():
    assert ops.png_rows_per_segment(512, 512) == 16 and ops.png_rows_per_segment(1024, 1024) == 16 and ops.png_rows_per_segment(512, 1556) == 8
    S = 16
    panel_d = torch.from_numpy(_coded(0, 1, S, S)[0]).to(DEV)
    wide = ops.fuse_canvas(panel_d, None, [_pred(1, S)] * 4, 1400, 3)  # a canvas 5 680 wide: 2 rows per segment
    assert wide.shape[2] == 5680 and ops.png_rows_per_segment(S, wide.shape[2]) == 2
    with pytest.raises(ValueError):
        ops.png_deflate(wide, 4)
    from PIL import Image
    with tempfile.TemporaryDirectory() as d:
        w = output.FrameWriter(d, encoder="device", fuse=output.FuseSpec(panel_d, pad=1400, pad_val=3, with_ref=False))
        w.submit(_pred(1, S), 0, more=(_pred(1, S),) * 3)
        path, = w.close()
        assert np.array_equal(np.asarray(Image.open(path).convert("RGB")), wide[0].cpu().numpy())


# ---- the runners --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _clip():
    """The synthetic model at S = 128, five frames in batches of three: the case, its frames as uint8 and the files of a run WITHOUT the option."""
    from tests import parity_utils as pu
    case = pu.build_case(image_size=128, num_filters=[64, 64, 128], n_res=2, bg_filters=[64, 64, 128], n_frames=5, ns=2)
    im = pu.make_imitator(case, frame_batch=3)
    assert (im.fuse_output, im.fuse_pad, im.fuse_pad_val, im.fused_video_path) == ("none", 10, 0, None)
    frames = np.stack(im.inference(case.tgt_smpls, cam_strategy="smooth"))
    u8 = ops.frames_to_u8(torch.from_numpy(frames).to(DEV)).cpu().numpy()
    d = tempfile.mkdtemp()
    try:
        paths = im.inference(case.tgt_smpls, cam_strategy="smooth", output_dir=d, prefix="pred_")
        assert sorted(os.listdir(d)) == ["pred_{:0>8}.png".format(t) for t in range(5)] and im.fused_video_path is None     # no fused file appears
        base = []
        for p in paths:
            with open(p, "rb") as fp:
                base.append((os.path.basename(p), fp.read()))
            os.remove(p)
    finally:
        os.rmdir(d)
    with pytest.raises(ValueError):
        im.inference(case.tgt_smpls, cam_strategy="smooth", output_dir="", ref_imgs=np.zeros((5, 128, 128, 3), np.uint8))
    pan = emu.panel(np.asarray(case.src_img, dtype=np.float32)[0])
    assert np.array_equal(ops.fuse_source_panel(im.src_info["img"]).cpu().numpy(), pan)
    refs = np.random.RandomState(12).randint(0, 256, size=(5, 128, 128, 3)).astype(np.uint8)
    return case, u8, base, pan, refs


def _files(paths):
    out = []
    for p in paths:
        with open(p, "rb") as fp:
            out.append((os.path.basename(p), fp.read()))
    return out


def test_imitator_writes_the_fused_video_next_to_its_usual_output():
    from PIL import Image
    from tests import parity_utils as pu
    case, u8, base, pan, refs = _clip()
    want = [_jpeg(c) for c in emu.canvas(pan, refs, [u8], 10, 0)]
    opt = type(case.opt)(case.opt)
    opt["fuse_output"] = "src_ref_out"
    case2 = type(case)(case, opt=opt)
    im = pu.make_imitator(case2, frame_batch=3)
    with tempfile.TemporaryDirectory() as d:
        for kind in ("array", "tensor", "paths"):
            out = os.path.join(d, kind)
            if kind == "paths":
                os.makedirs(os.path.join(d, "refs"))
                given = []
                for t in range(5):
                    given.append(os.path.join(d, "refs", "%04d.png" % t))
                    Image.fromarray(refs[t], mode="RGB").save(given[t])
            else:
                given = refs if kind == "array" else torch.from_numpy(refs).to(DEV)
            paths = im.inference(case.tgt_smpls, cam_strategy="smooth", output_dir=out, prefix="pred_", ref_imgs=given)
            assert _files(paths) == base, kind                        # the ordinary output: the same files, byte for byte
            assert im.fused_video_path == os.path.join(out, "pred_fused.avi")
            assert sorted(os.listdir(out)) == [n for n, _ in base] + ["pred_fused.avi"]
            with open(im.fused_video_path, "rb") as fp:
                info = riff_frames(fp.read())
            assert (info["width"], info["height"], info["total"], info["usec"]) == (64 + 2 * 138, 128, 5, 40000)
            for t in range(5):
                assert info["frames"][t] == want[t], (kind, t)
        with pytest.raises(ValueError):
            im.inference(case.tgt_smpls, cam_strategy="smooth", output_dir=os.path.join(d, "none"), prefix="pred_")          # no ref_imgs
        with pytest.raises(ValueError):
            im.inference(case.tgt_smpls, cam_strategy="smooth", output_dir=os.path.join(d, "four"), prefix="pred_", ref_imgs=refs[:4])
        with pytest.raises(ValueError):
            im.inference(case.tgt_smpls, cam_strategy="smooth", ref_imgs=refs)                                              # nowhere to write
    with pytest.raises(ValueError):
        opt["fuse_output"] = "ref_out"
        pu.make_imitator(case2, frame_batch=3)


def test_viewer_honours_src_out():
    from ipercore_amd.imitator import Viewer
    case, u8, base, pan, _ = _clip()
    opt = type(case.opt)(case.opt)
    opt.update(fuse_output="src_out", fuse_pad=3, fuse_pad_val=255, output_format="mjpeg", output_fps=30)
    vw = Viewer(opt, device=torch.device(DEV), frame_batch=2)
    vw.generator.load_state_dict({k: torch.tensor(v) for k, v in case.state.items()}, strict=True)
    vw.generator.to(vw.device)
    vw.set_source(case.src_smpl, case.uv_img, case.bg_img, src_img=case.src_img)
    with tempfile.TemporaryDirectory() as d:
        paths = vw.inference(case.tgt_smpls, cam_strategy="smooth", output_dir=d)
        assert paths == [os.path.join(d, "pred_video.avi")] and vw.fused_video_path == os.path.join(d, "pred_fused.avi")
        with open(paths[0], "rb") as fp:
            plain = riff_frames(fp.read())
        with open(vw.fused_video_path, "rb") as fp:
            info = riff_frames(fp.read())
    assert plain["frames"] == [_jpeg(u8[t]) for t in range(5)]
    assert info["frames"] == [_jpeg(c) for c in emu.canvas(pan, None, [u8], 3, 255)]
    assert (info["width"], info["total"], info["usec"]) == (64 + 131, 5, 33333)
    opt["fuse_output"] = "src_ref_out"
    vw2 = Viewer(opt, device=torch.device(DEV), frame_batch=2)
    vw2.src_info = vw.src_info
    with tempfile.TemporaryDirectory() as d:
        with pytest.raises(ValueError):
            vw2.inference(case.tgt_smpls, cam_strategy="smooth", output_dir=d)
