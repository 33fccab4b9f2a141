"""CPU emulation of csrc/conv_winograd_bf16.hip at its documented rounding points, the direct bf16 form beside it, and the error ratios of the
two against fp64 on Gaussian and adversarial operands.  Shared by tests/test_bf16_winograd_cpu.py, tests/test_gpu_bf16_winograd.py (the kernel is
compared with this emulation) and tools/bf16wino_lab.py --ratios."""
import torch
import torch.nn.functional as F

from tests.gpu_checks import ADV_KINDS, _adversarial_operands

BT = torch.tensor([[1., 0., -1., 0.], [0., 1., 1., 0.], [0., -1., 1., 0.], [0., 1., 0., -1.]])
G = torch.tensor([[1., 0., 0.], [.5, .5, .5], [.5, -.5, .5], [0., 0., 1.]], dtype=torch.float64)
AT = torch.tensor([[1., 1., 1., 0.], [0., 1., -1., -1.]])
KINDS = ADV_KINDS + ("gaussian",)
# Bound on relL2(Winograd) / relL2(direct), both against fp64 on the same operands.  V = B^T d B is a sum of four bf16 values rounded to bf16, U a
# sum of up to nine weights rounded to bf16: each operand of the 16-term inverse transform carries ONE bf16 rounding (2^-9 relative) of a value
# up to 4x (V) / 2.25x (U, before the 1/4 of G G^T) a single input's, where the direct form carries one rounding of the weight only (the
# activations are bf16 already); the fp64 emulation measured 1.19-1.91x (2.46x before the output rounding), and the factor 3 leaves room for
# the fp32 accumulation order.  The ratios this emulation gives are in profiles/bf16wino_adversarial_ratios.txt (tools/bf16wino_lab.py --ratios).
RATIO_BOUND = 3.0


def r16(t):
    return t.to(torch.bfloat16).float()


def emulate_winograd(x, w):
    """x (B, H, W, C) bf16-valued fp32, w (N, C, 3, 3) fp32 -> y (B, H, W, N) bf16-valued fp32, with exactly the rounding points of
    csrc/conv_winograd_bf16.hip: V = B^T d B in fp32 (B^T d first) rounded once to bf16, U = G w G^T in fp64 rounded once to bf16, fp32
    accumulation over the channels, fp32 A^T M A, one rounding to bf16 at the end.  (Products of two bf16 values are exact in fp32.)"""
    B, H, W, C = x.shape
    N = w.shape[0]
    ph, pw = (H + 1) // 2, (W + 1) // 2
    xp = F.pad(x.permute(0, 3, 1, 2), (1, 2 * pw - W + 1, 1, 2 * ph - H + 1))                     # (B, C, 2 ph + 2, 2 pw + 2)
    d = xp.unfold(2, 4, 2).unfold(3, 4, 2)                                                        # (B, C, ph, pw, 4, 4)
    t = torch.einsum("xr,bcijrs->bcijxs", BT, d)                                                  # two non-zero terms per output: one fp32 rounding
    V = r16(torch.einsum("bcijxs,ns->bcijxn", t, BT))                                             # (B, C, ph, pw, xi, nu)
    U = torch.einsum("ar,ncrs,bs->abcn", G, w.double(), G).to(torch.bfloat16).float()             # (xi, nu, C, N)
    Vm = V.permute(4, 5, 0, 2, 3, 1).reshape(16, B * ph * pw, C)
    M = torch.bmm(Vm, U.reshape(16, C, N)).reshape(4, 4, B, ph, pw, N)                            # fp32 accumulation
    tm = torch.einsum("jn,xnbpqc->xjbpqc", AT, M)                                                 # M A first (the kernel folds nu in registers)
    Y = torch.einsum("ix,xjbpqc->bpiqjc", AT, tm).reshape(B, 2 * ph, 2 * pw, N)
    return r16(Y[:, :H, :W].contiguous())


def emulate_direct(x, w):
    """The direct bf16 form on the same operands: weights rounded to bf16, fp32 accumulation, output rounded."""
    return r16(F.conv2d(x.permute(0, 3, 1, 2), r16(w), padding=1).permute(0, 2, 3, 1))


def rel_l2(y, ref):
    return ((y.double() - ref).pow(2).sum().sqrt() / ref.pow(2).sum().sqrt()).item()


def adversarial_ratios():
    """{case: (relL2 Winograd, relL2 direct, ratio)} over KINDS x {128 -> 64, 64 -> 128} x {16 x 16, 17 x 31}."""
    out = {}
    for kind in KINDS:
        for cin, n in ((128, 64), (64, 128)):
            for h, wd in ((16, 16), (17, 31)):
                w, x = _adversarial_operands(kind, cin, (n, cin, 3, 3), (1, h, wd, cin), 4100 + cin + h)
                x = r16(x)
                ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), padding=1).permute(0, 2, 3, 1)
                ew, ed = rel_l2(emulate_winograd(x, w), ref), rel_l2(emulate_direct(x, w), ref)
                out[f"{kind} {cin}->{n} {h}x{wd}"] = (ew, ed, ew / ed)
    return out
