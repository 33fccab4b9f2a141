"""The F(2x2, 3x3) Winograd weight gradient in plain torch (the four lines of csrc/conv_wgrad_winograd.hip's header), shared by the CPU identity
test and the GPU kernel tests.  x (B, H, W, Cin) and dy (B, H, W, N) are NHWC like the kernel's operands; the result is nn.Conv2d's (N, Cin, 3, 3).

    V_t = B^T d_t B      d_t: the 4 x 4 input patch of output tile t (2 x 2 outputs) with its 1-pixel halo, zero outside the image
    Z_t = A dy_t A^T     dy_t: the tile's 2 x 2 output gradients, zero beyond a ragged edge
    dU[xi, nu][c][n] = sum_t V_t[xi, nu][c] Z_t[xi, nu][n]
    dw[n][c] = G^T dU[., .][c][n] G
"""
import torch

BT = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
AT = [[1, 1, 1, 0], [0, 1, -1, -1]]
G = [[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]]


def transforms(x, dy):
    """-> V (T, 4, 4, Cin), Z (T, 4, 4, N) with T = B * ceil(H/2) * ceil(W/2) tiles in (image, tile row, tile column) order - the kernel's order."""
    dt = x.dtype
    Bn, H, W, C = x.shape
    N = dy.shape[3]
    th, tw = (H + 1) // 2, (W + 1) // 2
    xp = x.new_zeros(Bn, 2 * th + 2, 2 * tw + 2, C)
    xp[:, 1:H + 1, 1:W + 1] = x
    dp = dy.new_zeros(Bn, 2 * th, 2 * tw, N)
    dp[:, :H, :W] = dy
    d = xp.unfold(1, 4, 2).unfold(2, 4, 2)                      # (B, th, tw, C, 4, 4)
    d = d.permute(0, 1, 2, 4, 5, 3).reshape(Bn * th * tw, 4, 4, C)
    g = dp.unfold(1, 2, 2).unfold(2, 2, 2).permute(0, 1, 2, 4, 5, 3).reshape(Bn * th * tw, 2, 2, N)
    bt, at = torch.tensor(BT, dtype=dt), torch.tensor(AT, dtype=dt)
    V = torch.einsum("xi,tijc,nj->txnc", bt, d, bt)             # B^T d B
    Z = torch.einsum("ix,tijn,jm->txmn", at, g, at)             # A dy A^T  (A = AT^T)
    return V, Z


def wgrad(x, dy, chunk=None):
    """dw (N, Cin, 3, 3) in x's dtype.  chunk: add the tiles in runs of that many (fp32 runs that want the kernel's own association), None = one sum."""
    V, Z = transforms(x, dy)
    if chunk is None:
        dU = torch.einsum("txnc,txnm->xncm", V, Z)
    else:
        dU = V.new_zeros(4, 4, V.shape[3], Z.shape[3])
        for t0 in range(0, V.shape[0], chunk):
            dU = dU + torch.einsum("txnc,txnm->xncm", V[t0:t0 + chunk], Z[t0:t0 + chunk])
    g = torch.tensor(G, dtype=x.dtype)
    return torch.einsum("xk,xncm,nl->mckl", g, dU, g).contiguous()          # G^T dU G, (N, Cin, 3, 3)


def reference(x, dy):
    """torch.nn.grad.conv2d_weight on the same NHWC operands in fp64 -> (N, Cin, 3, 3)."""
    xn, dn = x.double().permute(0, 3, 1, 2).contiguous(), dy.double().permute(0, 3, 1, 2).contiguous()
    return torch.nn.grad.conv2d_weight(xn, (dy.shape[3], x.shape[3], 3, 3), dn, stride=1, padding=1)
