"""Flow families, operands and references for the attention-warp kernels (csrc/lwb_attn.hip, csrc/lwb_attn_x.hip, csrc/bf16_ops.hip).
CPU only (torch and numpy): tests/test_attn_flows_cpu.py checks this module itself, tests/test_gpu_lwb_attention_flows.py and the
fuse tests feed its fields to the kernels.

A flow is a grid_sample coordinate g in [-1, 1] (-2 = background); the kernels sample pixel ((g + 1) * size - 1) / 2, so
g = (2 i + 1) / size - 1 addresses pixel i exactly.  Every family is built in fp64 from such pixel coordinates and rounded to fp32 once.

Contract on flows (all families keep it): finite, and (g + 1) * size does not overflow fp32.  NaN, inf and overflowing magnitudes are
outside the kernels' contract and are never produced here.  With finite flows every tap copy clamps floor(pixel) to [-2, size + 1]
before the int conversion and tests 0 <= tap < size before it forms an address, so no family can move an address out of its tensor."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import emu_ops

FAMILIES = ("lattice", "half", "border", "collapse", "one_per_tile", "checker", "identity", "wild")
WILD_VALUES = (1e30, -1e30, 1e4, -1e4, 3.0, -3.0, -2.0)

# (B, ns, S, h, w): the smallest shapes that reach each path of the kernels
GEOMETRIES = ((1, 1, 8, 8, 8),          # one full tile, softmax over a single source
              (2, 2, 16, 16, 16),       # aligned tiles, the ns == 2 unrolled x-form
              (3, 3, 13, 13, 13),       # no resize, ragged on both edges, B = 3 in tile-major / frame-minor order
              (2, 3, 40, 9, 13),        # in-kernel resize, h != w, 2 x 2 cut tiles; 234 pixels divide by none of 4, 8, 16, 32
              (2, 2, 20, 7, 5),         # a feature map smaller than one tile
              (1, 2, 6, 1, 7),          # h = 1: the sc_y = 0 branch of the resize
              (1, 8, 12, 12, 12))       # ns = 8: the backward's register limit, the x-form's generic source loop
LARGE_X = (9, 2, None, 64, 64)          # x-form only, C = 128: 576 workgroups = the four-wave form (one frame alone: sixteen waves)
LARGE_X_FAMILIES = ("one_per_tile", "checker")

# bounds: the project's own (gpu_checks.check_lwb_attention_x, check_attention_backward, check_lwb_attention's flow resize)
FWD_TOL = {"f32": (1e-4, 5e-6), "bf16": (3e-2, 2e-3)}      # max_abs <= [0] * max(1, ref_max), mean_abs <= [1]
BWD_TOL = 5e-4                                              # relative to max(|ref| max, 1e-3 of the largest gradient)
KV_TOL = 1e-5                                               # K | V form against the two-tensor form (arrival order of the atomics)
STATS_TOL = (2e-6, 2e-6)                                    # mean, rstd relative
RESIZE_TOL = 4e-6                                           # * S * max(1, max |T|)
ERR32_FACTOR = 4.0                                          # in-kernel resize: bound = max(no-resize bound, 4 * err32)
ERR32_CAP = 2e-3                                            # 4 * err32 <= 2e-3 * max(1, ref_max), asserted on the CPU


def geom_id(g):
    return "B{}_ns{}_S{}_{}x{}".format(*g)


def uses_resize(geom):
    B, ns, S, h, w = geom
    return not (S == h and S == w)


def family_allowed(family, geom):
    """``wild`` only where no resize happens: interpolating between +1e30 and -1e30 is ill-conditioned."""
    return family != "wild" or not uses_resize(geom)


def _g(i, size):
    return (2.0 * i + 1.0) / size - 1.0


def flows(family, B, ns, H, W, seed, size=None):
    """fp32 (B, ns, H, W, 2) flow field of ``family``; [..., 0] is the x coordinate.  ``size`` = (h, w) of the feature map the pixel
    coordinates address, when the field is stored at another resolution and resized by the kernel (default: the field's own)."""
    h, w = (H, W) if size is None else size
    r = np.random.RandomState([seed, FAMILIES.index(family), B, ns, H, W])
    shape = (B, ns, H, W)
    if family == "lattice":
        ix, iy = r.randint(-2, w + 2, size=shape).astype(np.float64), r.randint(-2, h + 2, size=shape).astype(np.float64)
        gx, gy = _g(ix, w), _g(iy, h)
    elif family == "half":
        ix, iy = r.randint(-2, w + 1, size=shape) + 0.5, r.randint(-2, h + 1, size=shape) + 0.5
        gx, gy = _g(ix, w), _g(iy, h)
    elif family == "border":
        cx = np.array([-1.0, 0.0, w - 1.0, w])[r.randint(0, 4, size=shape)]
        cy = np.array([-1.0, 0.0, h - 1.0, h])[r.randint(0, 4, size=shape)]
        gx, gy = _g(cx + r.uniform(-0.02, 0.02, size=shape), w), _g(cy + r.uniform(-0.02, 0.02, size=shape), h)
    elif family == "collapse":
        gx, gy = np.full(shape, _g(w / 2.0 - 0.3, w)), np.full(shape, _g(h / 3.0 + 0.2, h))
    elif family == "one_per_tile":
        gx, gy = np.full(shape, -2.0), np.full(shape, -2.0)
        for b in range(B):
            for s in range(ns):
                for ty in range(0, H, 8):
                    for tx in range(0, W, 8):
                        th, tw = min(8, H - ty), min(8, W - tx)
                        p = r.randint(0, 64) % (th * tw)
                        gx[b, s, ty + p // tw, tx + p % tw], gy[b, s, ty + p // tw, tx + p % tw] = r.uniform(-1, 1, size=2)
    elif family == "checker":
        gx, gy = r.uniform(-1, 1, size=shape), r.uniform(-1, 1, size=shape)
        yy, xx, ss = np.arange(H)[None, :, None], np.arange(W)[None, None, :], np.arange(ns)[:, None, None]
        bg = np.broadcast_to(((yy + xx + ss) % 2 == 0)[None], shape)
        gx[bg], gy[bg] = -2.0, -2.0
    elif family == "identity":
        # field pixel Y sits at feature coordinate Y (h - 1) / (H - 1) under the align_corners=True resize: linear, so it survives the resize
        py = np.arange(H) * ((h - 1.0) / (H - 1.0) if H > 1 else 0.0)
        px = np.arange(W) * ((w - 1.0) / (W - 1.0) if W > 1 else 0.0)
        gx, gy = np.broadcast_to(_g(px, w)[None, :], shape).copy(), np.broadcast_to(_g(py, h)[:, None], shape).copy()
    elif family == "wild":
        gx, gy = r.uniform(-1, 1, size=shape), r.uniform(-1, 1, size=shape)
        odd = r.uniform(size=shape) < 0.5
        vals = np.array(WILD_VALUES)
        gx[odd], gy[odd] = vals[r.randint(0, len(vals), size=shape)][odd], vals[r.randint(0, len(vals), size=shape)][odd]
    else:
        raise ValueError(family)
    T = torch.tensor(np.stack([gx, gy], axis=-1).astype(np.float32))
    assert torch.isfinite(T).all() and torch.isfinite((T + 1) * float(max(h, w))).all()
    return T


def pixel_coords(T, h, w):
    """fp64 sampling positions (ix, iy) of a flow field already at (h, w)."""
    Td = T.double()
    return ((Td[..., 0] + 1) * w - 1) * 0.5, ((Td[..., 1] + 1) * h - 1) * 0.5


# ------------------------------------------------------------------------------------------------ operands
def rs(*key):
    return np.random.RandomState([int(k) for k in key])


def _n(r, shape, scale=1.0):
    return torch.tensor((r.standard_normal(shape) * scale).astype(np.float32))


def qkv_operands(r, B, ns, h, w, C, src_batched, peaked=False):
    """q (B,h,w,C), Ks, Vs (nsrc,h,w,C), bk, bv (C) - normal values, the biases x 0.1; ``peaked``: q x 40 (logits of order 40: a softmax
    far from uniform, the online rescaling corr = exp(mrun - mnew) at work)."""
    nsrc = B * ns if src_batched else ns
    q, Ks, Vs = _n(r, (B, h, w, C)), _n(r, (nsrc, h, w, C)), _n(r, (nsrc, h, w, C))
    bk, bv = _n(r, (C,), 0.1), _n(r, (C,), 0.1)
    return (q * 40.0 if peaked else q), Ks, Vs, bk, bv


def x_operands(r, B, ns, h, w, C, src_batched, peaked=False):
    """x (B,h,w,C), Kq, Vs (nsrc,h,w,C), kappa (nsrc,h,w), bv (C) of the x-form; ``peaked``: Kq and kappa x 40, x left alone."""
    nsrc = B * ns if src_batched else ns
    x, Kq, Vs = _n(r, (B, h, w, C)), _n(r, (nsrc, h, w, C)), _n(r, (nsrc, h, w, C))
    kappa, bv = _n(r, (nsrc, h, w)), _n(r, (C,), 0.1)
    return x, (Kq * 40.0 if peaked else Kq), (kappa * 40.0 if peaked else kappa), Vs, bv


def store(t, dt):
    """What the kernel is handed: ``t`` itself (fp32) or ``t`` rounded to bf16."""
    return t.to(torch.bfloat16) if dt == "bf16" else t


# ------------------------------------------------------------------------------------------------ references (tests/emu_ops.py in ``dtype``)
def ref_attention(q, Ks, Vs, bk, bv, T, src_batched, dtype=torch.float64):
    c = lambda t: t.to(dtype)        # noqa: E731
    return emu_ops.lwb_attention(c(q), c(Ks), c(Vs), c(bk), c(bv), c(T), torch.empty(q.shape, dtype=dtype), src_batched=src_batched)


def ref_attention_bwd(q, Ks, Vs, bk, bv, T, dout, src_batched, dtype=torch.float64):
    c = lambda t: t.to(dtype)        # noqa: E731
    return emu_ops.lwb_attention_bwd(c(q), c(Ks), c(Vs), c(bk), c(bv), c(T), c(dout), src_batched=src_batched)


def ref_attention_x(x, Kq, kappa, Vs, bv, T, src_batched, dtype=torch.float64):
    c = lambda t: t.to(dtype)        # noqa: E731
    return emu_ops.lwb_attention_x(c(x), c(Kq), c(kappa), c(Vs), c(bv), c(T), torch.empty(x.shape, dtype=dtype), stats=None, src_batched=src_batched)


def ref_flow_resize(T, h, w, dtype=torch.float64):
    return emu_ops.flow_resize(T.to(dtype), h, w)


def fwd_errors(got, ref):
    """(max_abs, mean_abs, ref_max) of ``got`` against the fp64 ``ref``."""
    err = (got.detach().cpu().double() - ref).abs()
    return err.max().item(), err.mean().item(), ref.abs().max().item()


def fwd_bound(dt, ref_max, err32=None):
    """(max bound, mean bound) of a forward case.  Without resize: check_lwb_attention_x's bounds.  With the in-kernel resize
    (``err32`` = (max, mean) error of the fp32 CPU evaluation of the same case): max(no-resize bound, 4 * err32) - the resize lambda's
    ~S * 2^-24 error is amplified by how far neighbouring flow samples jump, a property of the data; 4 allows another contraction order."""
    tmax, tmean = FWD_TOL[dt]
    bmax, bmean = tmax * max(1.0, ref_max), tmean
    if err32 is not None:
        bmax, bmean = max(bmax, ERR32_FACTOR * err32[0]), max(bmean, ERR32_FACTOR * err32[1])
    return bmax, bmean


def bwd_errors(got, ref):
    """check_attention_backward's measure: per gradient, max |d| / max(|ref| max, 1e-3 of the largest gradient).  (A field whose taps
    all fall outside the image has every gradient exactly zero: 1e-300 keeps the quotient defined, and any non-zero result fails.)"""
    gmax = max(r_.abs().max().item() for r_ in ref)
    return [(g_.detach().cpu().double() - r_).abs().max().item() / max(r_.abs().max().item(), 1e-3 * gmax, 1e-300) for g_, r_ in zip(got, ref)]


def forward_case(family, geom, C, src_batched, peaked, dt="f32", seed=0):
    """One forward case of the q / K / V kernels, the same on the CPU and on the GPU: operands in storage precision, the field at
    S x S, the fp64 reference on the stored values, and err32 (None without resize)."""
    B, ns, S, h, w = geom
    T = flows(family, B, ns, S, S, seed, size=(h, w))
    ops_ = [store(t, dt) if i < 3 else t for i, t in enumerate(qkv_operands(rs(seed, C, B, ns, h, w, int(src_batched)), B, ns, h, w, C, src_batched, peaked))]
    ref = ref_attention(*ops_, T, src_batched)
    err32 = None
    if uses_resize(geom):
        err32 = fwd_errors(ref_attention(*ops_, T, src_batched, dtype=torch.float32), ref)[:2]
    return ops_, T, ref, err32


def forward_table():
    """(family, geometry) pairs of the q / K / V forward and backward tests."""
    return [(f, g) for g in GEOMETRIES for f in FAMILIES if family_allowed(f, g)]


# ------------------------------------------------------------------------------------------------ deliberately wrong variants
VARIANTS = ("padding_border", "sample_align_corners", "resize_no_align_corners", "source_index", "softmax_axis")


def variant_attention(q, Ks, Vs, bk, bv, T, src_batched, variant=None, dtype=torch.float64):
    """emu_ops.lwb_attention's chain with one deliberate mistake (``variant`` None: the chain itself)."""
    q, Ks, Vs, bk, bv, T = (t.to(dtype) for t in (q, Ks, Vs, bk, bv, T))
    B, h, w, C = q.shape
    ns = T.shape[1]
    Tf = T.reshape(B * ns, T.shape[2], T.shape[3], 2)
    if (T.shape[2], T.shape[3]) != (h, w):
        Tf = F.interpolate(Tf.permute(0, 3, 1, 2), size=(h, w), mode="bilinear",
                           align_corners=variant != "resize_no_align_corners").permute(0, 2, 3, 1)
    if src_batched and variant == "source_index":
        Kn, Vn = Ks[:ns].repeat(B, 1, 1, 1), Vs[:ns].repeat(B, 1, 1, 1)          # row s where row b * ns + s belongs
    elif src_batched:
        Kn, Vn = Ks, Vs
    else:
        Kn, Vn = Ks.repeat(B, 1, 1, 1), Vs.repeat(B, 1, 1, 1)
    kw = dict(mode="bilinear", padding_mode="border" if variant == "padding_border" else "zeros", align_corners=variant == "sample_align_corners")
    Kw = F.grid_sample(Kn.permute(0, 3, 1, 2), Tf, **kw).view(B, ns, C, h, w) + bk.view(1, 1, C, 1, 1)
    Vw = F.grid_sample(Vn.permute(0, 3, 1, 2), Tf, **kw).view(B, ns, C, h, w) + bv.view(1, 1, C, 1, 1)
    logits = (Kw * q.permute(0, 3, 1, 2).unsqueeze(1)).sum(dim=2, keepdim=True) / math.sqrt(C)
    a = torch.softmax(logits, dim=0 if variant == "softmax_axis" else 1)         # over the frames instead of the sources
    return (a * Vw).sum(dim=1).permute(0, 2, 3, 1)


# ------------------------------------------------------------------------------------------------ independent reference
def attention_loops(q, Ks, Vs, bk, bv, T, src_batched):
    """The block as a plain numpy loop over pixels, sources and the four taps, in fp64, from the formulas in the header comment of
    csrc/lwb_attn.hip: flow resize S x S -> h x w with align_corners=True, pixel = ((g + 1) size - 1) / 2, zero padding,
    K_s = warp_s(Ks) + bk, V_s = warp_s(Vs) + bv, l_s = K_s . q / sqrt(C), out = sum_s softmax_s(l) V_s.  No torch sampling op."""
    q, Ks, Vs, bk, bv, T = (np.asarray(t, dtype=np.float64) for t in (q, Ks, Vs, bk, bv, T))
    B, h, w, C = q.shape
    ns, S = T.shape[1], T.shape[2]
    out = np.zeros((B, h, w, C))
    for b in range(B):
        for y in range(h):
            for x in range(w):
                Kp, Vp = np.zeros((ns, C)), np.zeros((ns, C))
                for s in range(ns):
                    if h == S and w == S:
                        g = T[b, s, y, x]
                    else:
                        sy = y * (S - 1) / (h - 1) if h > 1 else 0.0
                        sx = x * (S - 1) / (w - 1) if w > 1 else 0.0
                        y0, x0 = int(sy), int(sx)
                        y1, x1 = min(y0 + 1, S - 1), min(x0 + 1, S - 1)
                        ly, lx = sy - y0, sx - x0
                        g = (1 - ly) * ((1 - lx) * T[b, s, y0, x0] + lx * T[b, s, y0, x1]) + ly * ((1 - lx) * T[b, s, y1, x0] + lx * T[b, s, y1, x1])
                    ix, iy = ((g[0] + 1) * w - 1) / 2, ((g[1] + 1) * h - 1) / 2
                    fx, fy = math.floor(ix), math.floor(iy)
                    row = b * ns + s if src_batched else s
                    for ty, wy in ((fy, fy + 1 - iy), (fy + 1, iy - fy)):
                        for tx, wx in ((fx, fx + 1 - ix), (fx + 1, ix - fx)):
                            if 0 <= ty < h and 0 <= tx < w:
                                Kp[s] += wy * wx * Ks[row, int(ty), int(tx)]
                                Vp[s] += wy * wx * Vs[row, int(ty), int(tx)]
                logit = (Kp + bk) @ q[b, y, x] / math.sqrt(C)
                a = np.exp(logit - logit.max())
                a /= a.sum()
                out[b, y, x] = a @ (Vp + bv)
    return out


def touched(T, h, w, nsrc, src_batched, dilate=1):
    """(nsrc, h, w) bool: source texels within ``dilate`` pixels of an in-image tap of any flow (fp64 taps of the fp64-resized field;
    one pixel of dilation keeps an fp32 rounding of a coordinate across a pixel edge inside)."""
    B, ns = T.shape[:2]
    Tf = T.double() if (T.shape[2], T.shape[3]) == (h, w) else ref_flow_resize(T, h, w)
    ix, iy = pixel_coords(Tf, h, w)
    P = 6                               # margin: taps just outside the image are marked too, so their dilation reaches into it
    fx, fy = ix.floor().clamp(-4, w + 3).long() + P, iy.floor().clamp(-4, h + 3).long() + P
    hit = torch.zeros(nsrc, h + 2 * P, w + 2 * P)
    for b in range(B):
        for s in range(ns):
            for dy in (0, 1):
                for dx in (0, 1):
                    hit[b * ns + s if src_batched else s].view(-1)[((fy[b, s] + dy) * (w + 2 * P) + fx[b, s] + dx).flatten()] = 1.0
    if dilate:
        hit = F.max_pool2d(hit.unsqueeze(1), 2 * dilate + 1, 1, dilate)[:, 0]
    return hit[:, P:P + h, P:P + w] > 0
