"""CPU study: which Winograd tile can the ConvTranspose2d(4, 2, 1) kernel use without losing the accuracy bound of
tests/gpu_checks.py::check_winograd_adversarial (relative L2 error against fp64 <= 4x the direct kernel's)?

Each output parity of the layer is a 2 x 2-tap convolution; a tile F(my x mx, 2x2) is emulated in fp32 the way the kernels compute it:
the data transform in fp32, U = G_y g G_x^T formed in fp64 and rounded once, the K contraction accumulated in fp32 two products at a time
in order (one v_mfma_f32_32x32x2_f32 per k-pair), the output transform in fp32.  The direct kernel is emulated the same way over
K = 4 Cin in its panel order.  Operands: the six adversarial kinds of tests/gpu_checks.py (_adversarial_operands) at Cin = 64 and 256.

    python tools/convt_tile_study.py            # the table of DESIGN.md 3.12c (a few minutes)
"""
import os
import sys
from fractions import Fraction

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.gpu_checks import ADV_KINDS, _adversarial_operands, _rand  # noqa: E402


def toom(points, m):
    """F(m, 2) for the finite points + inf: A^T (m x n), G (n x 2), B^T (n x n) as fractions, B^T's rows scaled to integers (the factor moves into G)."""
    n = m + 1
    AT = [[Fraction(0)] * n for _ in range(m)]
    G = [[Fraction(0)] * 2 for _ in range(n)]
    for j, p in enumerate(points):
        p = Fraction(p)
        f = Fraction(1)
        for q in points:
            if Fraction(q) != p:
                f *= p - Fraction(q)
        for i in range(m):
            AT[i][j] = p ** i
        G[j] = [Fraction(1) / f, p / f]
    AT[m - 1][n - 1] = Fraction(1)
    G[n - 1] = [Fraction(0), Fraction(1)]
    # B^T from A^T diag(G g) B^T d = correlation, for all g, d: solve the linear system exactly (float solve, rounded to small fractions)
    rows = []
    rhs = []
    for i in range(m):
        for q in range(2):
            for s in range(n):
                rows.append([float(AT[i][j] * G[j][q]) if jj == s else 0.0 for j in range(n) for jj in range(n)])
                rhs.append(1.0 if s == i + q else 0.0)
    sol = np.linalg.lstsq(np.array(rows), np.array(rhs), rcond=None)[0].reshape(n, n)
    BT = [[Fraction(v).limit_denominator(64) for v in r] for r in sol]
    for j in range(n):                                        # integer rows: the scale factor into G
        den = 1
        for v in BT[j]:
            den = den * v.denominator // np.gcd(den, v.denominator)
        BT[j] = [v * den for v in BT[j]]
        G[j] = [v / den for v in G[j]]
    f64 = lambda M: np.array([[float(v) for v in r] for r in M])      # noqa: E731
    return f64(AT), f64(G), f64(BT)


F22 = (np.array([[1.0, 1, 0], [0, 1, 1]]), np.array([[1.0, 0], [1, 1], [0, 1]]), np.array([[1.0, -1, 0], [0, 1, 0], [0, -1, 1]]))
TILES = {
    "F(2x2,2x2)": (F22, F22),
    "F(2x4,2x2) {0,+-1,1/2,inf}": (F22, toom([0, 1, -1, Fraction(1, 2)], 4)),
    "F(2x4,2x2) {0,+-1,2,inf}": (F22, toom([0, 1, -1, 2], 4)),
    "F(4x4,2x2) {0,+-1,1/2,inf}": (toom([0, 1, -1, Fraction(1, 2)], 4), toom([0, 1, -1, Fraction(1, 2)], 4)),
    "F(3x3,2x2) {0,+-1,inf}": (toom([0, 1, -1], 3), toom([0, 1, -1], 3)),
}


def _pairs(V, U):
    """sum_c V[..., c] U[c, :] in fp32, two products per step in order (V: (..., C) fp32, U: (C, N) fp32)."""
    acc = np.zeros(V.shape[:-1] + (U.shape[1],), np.float32)
    for c in range(0, V.shape[-1], 2):
        acc = acc + (V[..., c:c + 1] * U[c] + V[..., c + 1:c + 2] * U[c + 1])
    return acc


def parity_kernels(w):
    """g[py][px][r][q] (Cin, N): the 2 x 2 sub-kernel of parity (py, px) in input-offset order: g[r][q] = w[:, :, 3 - py - 2 * r, 3 - px - 2 * q]."""
    return [[[[w[:, :, 3 - py - 2 * r, 3 - px - 2 * q] for q in range(2)] for r in range(2)] for px in range(2)] for py in range(2)]


def winograd(x, w, b, tile):
    (ATy, Gy, BTy), (ATx, Gx, BTx) = tile
    my, mx = ATy.shape[0], ATx.shape[0]
    B, H, W, C = x.shape
    N = w.shape[1]
    Hp, Wp = -(-H // my) * my, -(-W // mx) * mx
    xp = np.zeros((B, Hp + my + 2, Wp + mx + 2, C), np.float32)
    xp[:, 1:H + 1, 1:W + 1] = x
    g = parity_kernels(w.astype(np.float64))
    y = np.zeros((B, 2 * Hp, 2 * Wp, N), np.float32)
    for py in range(2):
        for px in range(2):
            gg = np.array(g[py][px])                                                   # (2, 2, C, N)
            U = np.einsum("ar,rqcn,bq->abcn", Gy, gg, Gx).astype(np.float32)
            # d[s][t] = x[i0 + py - 1 + s][j0 + px - 1 + t] = xp[i0 + py + s][j0 + px + t]
            d = np.stack([np.stack([xp[:, py + s:py + s + Hp:my, px + t:px + t + Wp:mx] for t in range(mx + 1)], 3) for s in range(my + 1)], 3)
            V = np.einsum("as,bt,...stc->...abc", BTy.astype(np.float32), BTx.astype(np.float32), d).astype(np.float32)
            M = np.stack([np.stack([_pairs(V[..., a, bb, :], U[a, bb]) for bb in range(V.shape[-2])], -2) for a in range(V.shape[-3])], -3)
            Y = np.einsum("ia,jb,...abn->...ijn", ATy.astype(np.float32), ATx.astype(np.float32), M).astype(np.float32)   # (B, Ty, Tx, my, mx, N)
            Y = Y.transpose(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, N)
            y[:, py::2, px::2] = Y + b.astype(np.float32)
    return y[:, :2 * H, :2 * W]


def direct(x, w, b):
    """The direct kernel: per parity K = 4 Cin, rows ((c / 32) 4 + tap) 32 + c % 32, fp32 pairs in order."""
    B, H, W, C = x.shape
    N = w.shape[1]
    xp = np.zeros((B, H + 2, W + 2, C), np.float32)
    xp[:, 1:H + 1, 1:W + 1] = x
    g = parity_kernels(w.astype(np.float32))
    y = np.zeros((B, 2 * H, 2 * W, N), np.float32)
    for py in range(2):
        for px in range(2):
            cols, rows = [], []
            for cb in range(C // 32):
                for r in range(2):
                    for q in range(2):
                        cols.append(xp[:, py + r:py + r + H, px + q:px + q + W, 32 * cb:32 * cb + 32])
                        rows.append(g[py][px][r][q][32 * cb:32 * cb + 32])
            y[:, py::2, px::2] = _pairs(np.concatenate(cols, -1), np.concatenate(rows, 0)) + b.astype(np.float32)
    return y


def main():
    rel = lambda y, ref: float(np.linalg.norm((y.astype(np.float64) - ref).ravel()) / np.linalg.norm(ref.ravel()))      # noqa: E731
    worst = {name: (np.inf, 0.0) for name in TILES}
    for (B, H, W, Cin, N) in ((2, 32, 48, 64, 64), (1, 32, 32, 256, 256)):
        for kind in ADV_KINDS:
            w, x = _adversarial_operands(kind, Cin, (Cin, N, 4, 4), (B, H // 2, W // 2, Cin), 410 + Cin, cin_dim=0, fan=4 * Cin)
            b = _rand((N,), 411, 0.1)
            ref = torch.nn.functional.conv_transpose2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), stride=2, padding=1).permute(0, 2, 3, 1).numpy()
            xn, wn, bn = x.numpy(), w.numpy(), b.numpy()
            ed = rel(direct(xn, wn, bn), ref)
            line = [f"Cin {Cin:3d} {kind:12s} direct {ed:.2e}"]
            for name, tile in TILES.items():
                r = rel(winograd(xn, wn, bn, tile), ref) / ed
                worst[name] = (min(worst[name][0], r), max(worst[name][1], r))
                line.append(f"{name.split()[0]} {r:.2f}x")
            print("  ".join(line), flush=True)
    print("\nerror / direct over all cases (gate: 4x):")
    for name, (lo, hi) in worst.items():
        print(f"  {name:28s} {lo:.2f} - {hi:.2f}x")


if __name__ == "__main__":
    main()
