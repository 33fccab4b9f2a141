"""CPU restatement of ``lwg_lwb_fuse_bwd_f32`` (include/lwg_hip.h): the contract of the kernel tap by tap in torch, NOT a call to
autograd - the flow resize (bilinear, align_corners=True), the grid_sample coordinates (align_corners=False), the four bilinear
taps with zero padding, the scatter into the sources' gradient and the recomputed gather for the gate's gradient.

Works in the dtype of its inputs (fp64 in the contract test, fp32 under the emulated ABI).  Tests patch it onto ``ops`` themselves,
after ``emu_ops.install(monkeypatch)``:  ``monkeypatch.setattr(ops, "lwb_fuse_bwd", lwbfuse_emu.lwb_fuse_bwd)``."""
import torch


def resize_flow(T, h, w):
    """(n,S,S,2) -> (n,h,w,2), the kernel's inline resize: source index = dst * (S - 1) / (size - 1), second tap clamped to S - 1."""
    n, S = T.shape[0], T.shape[1]
    if h == S and w == S:
        return T
    dt = T.dtype
    sy = torch.arange(h, dtype=dt) * ((S - 1) / (h - 1) if h > 1 else 0.0)
    sx = torch.arange(w, dtype=dt) * ((S - 1) / (w - 1) if w > 1 else 0.0)
    y0, x0 = sy.floor().long(), sx.floor().long()
    y1, x1 = y0 + (y0 < S - 1).long(), x0 + (x0 < S - 1).long()
    ly1, lx1 = (sy - y0.to(dt)).view(1, h, 1, 1), (sx - x0.to(dt)).view(1, 1, w, 1)
    ly0, lx0 = 1 - ly1, 1 - lx1
    t = lambda yy, xx: T[:, yy][:, :, xx]                         # noqa: E731
    return ly0 * (lx0 * t(y0, x0) + lx1 * t(y0, x1)) + ly1 * (lx0 * t(y1, x0) + lx1 * t(y1, x1))


def taps(Tf, h, w):
    """Tf (h,w,2) flow at feature size -> the four taps [(ty, tx, weight, in_range)] of every pixel, row-major 2 x 2."""
    ix = ((Tf[..., 0] + 1) * w - 1) * 0.5
    iy = ((Tf[..., 1] + 1) * h - 1) * 0.5
    fx0, fy0 = ix.floor(), iy.floor()
    wx1, wy1, wx0, wy0 = ix - fx0, iy - fy0, (fx0 + 1) - ix, (fy0 + 1) - iy
    tx0, ty0 = fx0.clamp(-2, w + 1).long(), fy0.clamp(-2, h + 1).long()
    out = []
    for t in range(4):
        ty, tx = ty0 + (t >> 1), tx0 + (t & 1)
        wt = (wy1 if (t >> 1) else wy0) * (wx1 if (t & 1) else wx0)
        out.append((ty, tx, wt, (ty >= 0) & (ty < h) & (tx >= 0) & (tx < w)))
    return out


def lwb_fuse_bwd(src_x, gate, T, dout, src_batched=False, scale_w=1.0, scale_o=1.0):
    """-> (d_tsf, d_src, d_gate | None); d_src starts at zero and is accumulated into, frames of a shared source adding up."""
    if not dout.is_cuda:
        raise RuntimeError("ipercore_amd ops need CUDA (HIP) tensors: the MI355X path has no CPU fallback")
    B, h, w, C = dout.shape
    ns, S = T.shape[1], T.shape[2]
    assert T.shape[0] == B and src_x.shape[0] == (B * ns if src_batched else ns) and tuple(src_x.shape[1:]) == (h, w, C)
    d_tsf = dout * scale_o
    d_src = torch.zeros_like(src_x)
    g = torch.ones_like(dout) if gate is None else gate
    v = (scale_o * scale_w) * g * dout                                     # what every tap of a pixel scatters, times its weight
    acc = torch.zeros_like(dout)
    Tf = resize_flow(T.reshape(B * ns, S, S, 2), h, w).reshape(B, ns, h, w, 2)
    for b in range(B):
        for s in range(ns):
            sidx = b * ns + s if src_batched else s
            rows = d_src[sidx].view(h * w, C)
            srows = src_x[sidx].reshape(h * w, C)
            for ty, tx, wt, ok in taps(Tf[b, s], h, w):
                idx = (ty * w + tx)[ok]
                rows.index_add_(0, idx, wt[ok].unsqueeze(1) * v[b][ok])
                if gate is not None:
                    acc[b][ok] += wt[ok].unsqueeze(1) * srows[idx]
    d_gate = None if gate is None else (scale_o * scale_w) * dout * acc
    return d_tsf, d_src, d_gate
