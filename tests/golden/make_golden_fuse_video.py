#!/usr/bin/env python3
"""Generate tests/golden/golden_fuse_video_v1.npz: the source panel and the canvas rows of the REFERENCE's own
tools/utils/multimedia/video.py - ``fuse_source``, ``merge``, ``merge_src_out``, ``merge_multi_outs`` - loaded from the reference checkout in
the authoring container and run on seeded 16 x 16 PNG files: the panel for ns = 1 .. 9, the three row forms for ns in (1, 2, 8) with pad 10
(pad_val 0) and pad 3 (pad_val 255).

    python tests/golden/make_golden_fuse_video.py

video.py imports cv2 and tqdm, which are not installed here: stand-in modules are put into sys.modules first.  ``cv2.imread`` goes through PIL
and flips to BGR; ``cv2.resize`` is OpenCV's INTER_LINEAR for uint8 restated from its algorithm (half-pixel centres, 11-bit coefficients, the
horizontal pass in int, the vertical ``((b0 (r0 >> 4)) >> 16) + ((b1 (r1 >> 4)) >> 16) + 2) >> 2``).  So what the file pins is the LAYOUT - which
source lands where at which size, the order of the regions - by the reference's own concatenations; the resize is the stand-in's, and parity
with OpenCV's binary is not pinned.

Stored (arrays only, everything in the reference's BGR except ``src`` / ``ref`` / ``outs``, which are the RGB pixels of the PNG files):
src (9,16,16,3), ref (16,16,3), outs (3,16,16,3); panel_ns{1..9}; row_{merge|src_out|multi}_ns{1,2,8}_pad{10,3} (multi: the three outs)."""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("LWG_REFERENCE", "/root/reference")
S = 16
PADS = ((10, 0), (3, 255))
ROW_NS = (1, 2, 8)


def resize_linear_u8(img, dsize):
    """OpenCV's resize(INTER_LINEAR) for 8-bit images, restated: dsize = (width, height)."""
    img = np.asarray(img)
    sh, sw = img.shape[:2]
    dw, dh = int(dsize[0]), int(dsize[1])

    def taps(dn, sn):
        scale = sn / dn
        d = np.arange(dn)
        f = ((d + 0.5) * scale - 0.5).astype(np.float32)
        s0 = np.floor(f).astype(np.int64)
        f = f - s0
        f = np.where(s0 < 0, 0.0, f)
        s0 = np.maximum(s0, 0)
        f = np.where(s0 >= sn - 1, 0.0, f)
        s0 = np.minimum(s0, sn - 1)
        s1 = np.minimum(s0 + 1, sn - 1)
        a1 = np.rint(f.astype(np.float32) * 2048).astype(np.int64)
        a0 = np.rint((1.0 - f).astype(np.float32) * 2048).astype(np.int64)
        return s0, s1, a0, a1
    x0, x1, ax0, ax1 = taps(dw, sw)
    y0, y1, ay0, ay1 = taps(dh, sh)
    src = img.astype(np.int64)
    rows = src[:, x0] * ax0[None, :, None] + src[:, x1] * ax1[None, :, None]                # (sh, dw, 3): the horizontal pass
    r0, r1 = rows[y0], rows[y1]
    out = (((ay0[:, None, None] * (r0 >> 4)) >> 16) + ((ay1[:, None, None] * (r1 >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def stand_in_modules():
    from PIL import Image
    cv2 = types.ModuleType("cv2")
    cv2.INTER_LINEAR = 1

    def imread(path, *a):
        return np.ascontiguousarray(np.asarray(Image.open(path).convert("RGB"))[:, :, ::-1])

    def resize(img, dsize, *a, **kw):
        return resize_linear_u8(img, dsize)
    cv2.imread, cv2.resize = imread, resize
    sys.modules["cv2"] = cv2
    try:
        import tqdm  # noqa: F401
    except ImportError:
        tq = types.ModuleType("tqdm")
        tq.tqdm = lambda it, *a, **kw: it
        sys.modules["tqdm"] = tq


def images(seed=20):
    """Nine sources, one reference frame, three outputs: a gradient per image (so a swapped or mirrored cell shows) plus seeded noise."""
    r = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:S, 0:S]
    out = []
    for k in range(13):
        base = np.stack([(yy * 13 + k * 17) % 256, (xx * 11 + k * 29) % 256, ((yy + xx) * 7 + k * 41) % 256], axis=-1)
        out.append(((base + r.randint(0, 48, size=(S, S, 3))) % 256).astype(np.uint8))
    return np.stack(out[:9]), out[9], np.stack(out[10:])


def main():
    from PIL import Image
    stand_in_modules()
    spec = importlib.util.spec_from_file_location("ref_video", os.path.join(REF, "iPERCore/tools/utils/multimedia/video.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    src, refimg, outs = images()
    res = {"src": src, "ref": refimg, "outs": outs}
    with tempfile.TemporaryDirectory() as d:
        def save(name, a):
            p = os.path.join(d, name + ".png")
            Image.fromarray(a, mode="RGB").save(p)
            return p
        src_paths = [save("src%d" % k, src[k]) for k in range(9)]
        ref_path = save("ref", refimg)
        out_paths = [save("out%d" % k, outs[k]) for k in range(3)]
        for ns in range(1, 10):
            res["panel_ns%d" % ns] = ref.fuse_source(src_paths[:ns], S)
        for ns in ROW_NS:
            fused = res["panel_ns%d" % ns]
            for pad, pad_val in PADS:
                pad_region = np.zeros((S, pad, 3), dtype=np.uint8) + np.uint8(pad_val)      # (fuse_src_ref_multi_outputs builds it so)
                tag = "_ns%d_pad%d" % (ns, pad)
                res["row_merge" + tag] = ref.merge(fused, ref_path, out_paths[0], pad_region)
                res["row_src_out" + tag] = ref.merge_src_out(fused, out_paths[0], pad_region)
                res["row_multi" + tag] = ref.merge_multi_outs(fused, ref_path, out_paths, pad_region)
    for k, v in res.items():
        assert v.dtype == np.uint8, (k, v.dtype)
    dst = os.path.join(HERE, "golden_fuse_video_v1.npz")
    np.savez_compressed(dst, **res)
    print("wrote", dst, os.path.getsize(dst), "bytes;", {k: v.shape for k, v in res.items()})


if __name__ == "__main__":
    main()
