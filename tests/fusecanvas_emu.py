"""The comparison canvas of the output stage in numpy - the DEFINITION that csrc/lwg_fuse_geom.h, lwg_fuse_sources_u8 and lwg_fuse_canvas_u8
equal byte for byte.  It restates fuse_source / merge_multi_outs / merge_src_out of the reference
(tools/utils/multimedia/video.py:173-213, 297-357) with explicit index arithmetic per pixel - no concatenation - so that it is a second,
independent statement of the layout; tests/golden/golden_fuse_video_v1.npz (the reference's own concatenations) pins it.  RGB throughout.

  layout(ns, S)                 -> (Wp, [(source or -1, top, left, size), ...])
  src_u8(x)                     -> the 8-bit level of a source pixel: clamp(rint((x + 1) * 127.5), 0, 255), fp32, ties to even, NaN -> 0
  panel(src (ns,3,S,S) fp32)    -> (S,Wp,3) uint8
  row_map(Wp, S, pad, has_ref, n_out) -> per byte of a canvas row (region, offset in the region's row); regions PANEL, PAD, REF, OUT0 + k
  canvas(panel, refs, outs_u8, pad, pad_val) -> (B,S,Wc,3) uint8 from the panel, (B,S,S,3) uint8 refs or None, and the outs as (B,S,S,3) uint8
  frames_u8(pred (B,3,S,S))     -> (B,S,S,3) uint8: lwg_frames_to_u8's in-range arithmetic, uint8((x + 1) / 2.0 * 255)
"""
import numpy as np

PANEL, PAD, REF, OUT0 = 0, 1, 2, 3


def layout(ns, S):
    """The cells of fuse_source AS ITS CODE RUNS: ns = 7 is padded to eight paths and then handed to fuse_four_images (sources 0..3);
    ns >= 8 goes to fuse_eight_images, which hands paths [0:4] and [4:8] to fuse_two_images - and that reads two of each: sources 0, 1, 4, 5,
    one column of quarter-size cells.  ValueError for sizes the halving / quartering does not divide."""
    ns, S = int(ns), int(S)
    if ns < 1 or S < 1:
        raise ValueError("ns >= 1 and S >= 1")
    if ns == 1:
        return S, [(0, 0, 0, S)]
    if ns <= 7:
        if S % 2:
            raise ValueError("2..7 sources need an even size")
        s = S // 2
        if ns == 2:
            return s, [(0, 0, 0, s), (1, s, 0, s)]
        return S, [(0, 0, 0, s), (1, s, 0, s), (2, 0, s, s), (3 if ns > 3 else -1, s, s, s)]
    if S % 4:
        raise ValueError("8 and more sources need S % 4 == 0")
    q = S // 4
    return q, [(0, 0, 0, q), (1, q, 0, q), (4, 2 * q, 0, q), (5, 3 * q, 0, q)]


def src_u8(x):
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.rint((x + np.float32(1)) * np.float32(127.5)).astype(np.float32)
    t = np.where(np.isnan(t), np.float32(0), t)
    return np.clip(t, 0, 255).astype(np.uint8)


def panel(src):
    """Every panel pixel from its cell: factor f = S / size in {1, 2, 4}; the pixel is (a + b + c + d + 2) >> 2 over source rows and columns
    f i + f/2 - 1 and f i + f/2 (cv2.resize INTER_LINEAR of uint8 at these factors; f = 1: the pixel itself)."""
    src = np.asarray(src, dtype=np.float32)
    ns, C, S, S2 = src.shape
    assert C == 3 and S == S2
    Wp, cells = layout(ns, S)
    u = src_u8(src).astype(np.int32)                                  # (ns,3,S,S)
    out = np.zeros((S, Wp, 3), dtype=np.uint8)
    hits = np.zeros((S, Wp), dtype=np.int32)
    for k, top, left, size in cells:
        f = S // size
        assert f * size == S and f in (1, 2, 4)
        i = np.arange(size)
        lo = f * i + (f // 2 - 1 if f > 1 else 0)
        hi = lo + (1 if f > 1 else 0)
        hits[top:top + size, left:left + size] += 1
        if k < 0:
            continue
        for ch in range(3):
            p = u[k, ch]
            v = (p[lo[:, None], lo[None, :]] + p[lo[:, None], hi[None, :]] + p[hi[:, None], lo[None, :]] + p[hi[:, None], hi[None, :]] + 2) >> 2
            out[top + i[:, None], left + i[None, :], ch] = v
    assert (hits == 1).all(), "the cells tile the panel"
    return out


def canvas_width(Wp, S, pad, has_ref, n_out):
    return Wp + (int(bool(has_ref)) + n_out) * (S + pad)


def row_map(Wp, S, pad, has_ref, n_out):
    """(region, offset) of each of the 3 Wc bytes of a canvas row, pixel by pixel."""
    Wc = canvas_width(Wp, S, pad, has_ref, n_out)
    xb = np.arange(3 * Wc)
    px, ch = xb // 3, xb % 3
    region = np.empty(3 * Wc, dtype=np.int32)
    off = np.empty(3 * Wc, dtype=np.int32)
    in_panel = px < Wp
    region[in_panel], off[in_panel] = PANEL, xb[in_panel]
    r = px - Wp
    slot, q = r // (S + pad), r % (S + pad)
    in_pad = ~in_panel & (q < pad)
    region[in_pad], off[in_pad] = PAD, (3 * q + ch)[in_pad]
    img = ~in_panel & (q >= pad)
    if has_ref:                                                       # slot 0 is the reference frame, out k is slot k + 1
        region[img] = np.where(slot == 0, REF, OUT0 + slot - 1)[img]
    else:
        region[img] = (OUT0 + slot)[img]
    off[img] = (3 * (q - pad) + ch)[img]
    return region, off


def canvas(panel_u8, refs, outs_u8, pad=10, pad_val=0):
    panel_u8 = np.asarray(panel_u8)
    outs_u8 = [np.asarray(o) for o in outs_u8]
    B, S = outs_u8[0].shape[0], outs_u8[0].shape[1]
    Wp = panel_u8.shape[1]
    assert panel_u8.shape == (S, Wp, 3) and all(o.shape == (B, S, S, 3) and o.dtype == np.uint8 for o in outs_u8) and 1 <= len(outs_u8) <= 4
    assert refs is None or np.asarray(refs).shape == (B, S, S, 3)
    region, off = row_map(Wp, S, pad, refs is not None, len(outs_u8))
    Wc = region.size // 3
    out = np.empty((B, S, 3 * Wc), dtype=np.uint8)
    written = np.zeros(3 * Wc, dtype=np.int32)
    m = region == PANEL
    out[:, :, m] = panel_u8.reshape(S, 3 * Wp)[None][:, :, off[m]]
    written[m] += 1
    m = region == PAD
    out[:, :, m] = pad_val
    written[m] += 1
    if refs is not None:
        m = region == REF
        out[:, :, m] = np.asarray(refs).reshape(B, S, 3 * S)[:, :, off[m]]
        written[m] += 1
    for k, o in enumerate(outs_u8):
        m = region == OUT0 + k
        out[:, :, m] = o.reshape(B, S, 3 * S)[:, :, off[m]]
        written[m] += 1
    assert (written == 1).all()
    return out.reshape(B, S, Wc, 3)


def frames_u8(pred):
    x = np.transpose(np.asarray(pred, dtype=np.float32), (0, 2, 3, 1))
    return ((x + 1) / 2.0 * 255).astype(np.uint8)
