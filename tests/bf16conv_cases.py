"""Seeded exact-input cases, references, launch forms and planted faults for the bf16 convolution engine: the five kernels of
csrc/conv_igemm_bf16.hip (lwg_conv_bf16_hr2_kernel, lwg_conv_bf16_up4_kernel, lwg_conv_bf16_kernel, lwg_conv_bf16_pw_kernel,
lwg_conv_c8_bf16_kernel) and lwg_conv2d_winograd_bf16 (csrc/conv_winograd_bf16.hip).  CPU only (numpy and torch): tests/test_bf16conv_cases_cpu.py
checks this module itself - the family's exactness on every case, the planted faults, ``bf16_form`` against the text of the launch rules - and
tests/test_gpu_bf16_conv_exact.py feeds the same cases to the HIP library and compares bit for bit.

Why exact inputs.  The kernel-level checks of these kernels (gpu_checks._bf16_kernel_case: 1.2e-2 of the reference's maximum on Gaussian data;
test_gpu_bf16_winograd.py: 2.4e-2) bound a rounding error.  With Cin = 256 a 3 x 3 launch sums 2304 products of which a typical one is 0.5 % of
the output's maximum: an output that lost one product, took the bias of another column or read one wrong halo pixel is a plausible bf16
rounding of the right one.  Here nothing rounds, so one wrong product is one wrong bit pattern.

The family ("ternary").  All arithmetic of these kernels is bf16 x bf16 products accumulated in fp32, an fp32 epilogue and ONE rounding to bf16:
  x, w      uniform in {-1, 0, 1} (x fp32 for the first-layer kernel, bf16 elsewhere), seeded;
  bias      integers in [-8, 8]; the residual operand too;
  SPADE     xn integers in [-5, 5], mean integers in [-3, 3], rstd in {1, 2}; the gamma and beta weights have SPADE_NNZ = 6 non-zeros per output
            channel, so |gamma|, |beta| <= 6 + 8 < 15 and |(xn - mean) rstd (1 + gamma) + beta| <= 8 * 2 * 15 + 14 = 254.
Every product and every partial sum is an integer far below 2^24: exact in any summation order, with or without fma contraction.  F(2x2, 3x3)
Winograd: the transformed input B^T d B is an integer of magnitude <= 4, the transformed weight G w G^T a multiple of 1/4 of magnitude <= 9/4
- both bf16-exact -, every later sum a multiple of 1/4 below 2^22: the same integer as the direct form's.  The condition on the OUTPUT is
asserted per case on the reference, never on a kernel's result: every final value is bf16-representable (integers of magnitude <= 256 and the
even ones beyond), so the final rounding is the identity and the comparison is ``torch.equal`` over 100 % of the elements.
Other families: "dense" (x in [-4, 4], w in [-2, 2]: the fp32 accumulator frame of lwg_conv2d_nhwc_bf16_hr_acc, which no bf16 rounding follows),
"tie" (chosen outputs are 257, 259, -257, -259 and 385: the final rounding must be to nearest even - 256, 260, -256, -260, 384 -, the expected
frame is torch's rounding of the exact one) and "impulse" (one (pixel, channel) of each image is 1, the weights are a distinct bf16 code per
(n, tap, c) - up to the 65024 normal bf16 values, beyond which the code wraps -: every output names the one weight it read).

``bf16_form`` restates which entry point and tile form a launch takes (ops.conv2d_route, launch_epi_bf16 / launch_epi_bf16_hr,
lwg_conv_transpose4_nhwc_bf16, launch_cfg_bf16_pw_tm, lwg_conv2d_nhwc_c8_bf16); the GPU tests assert it for every case with the device's CU
count, and the shapes whose form depends on that count are computed from it.

Planted faults (``restated(case, fault=...)``, a plain torch statement of the convolution chunk by chunk and tap by tap): the indexing errors
the Gaussian checks cannot see.  ``covers(case, cus)`` names the faults a case claims to expose; the CPU test holds it to that."""
import collections
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

Case = collections.namedtuple("Case", "name kind B H W C0 C1 N k stride epi act pad family route extra")
# kind    "conv" (bf16 in), "first" (fp32 NHWC-8 in: lwg_conv2d_nhwc_c8_bf16), "convT" (ConvTranspose2d(4, 2, 1)), "acc" (the fp32 accumulator frame)
# H, W    of the INPUT;  k: 1, 3, or 10 (the 3 x 3 taps and (0, 2): the first-layer kernel's widest tap list);  N: panel columns (SPADE: 2 YC)
# epi     "plain" | "res" | "spade";  act: "none" | "relu";  pad: output-slice sentinels, y has N + pad channels and ycoff = 8 (0: the whole tensor)
# route   "default" | "lds" (BF16_HR = BF16_PW = False) | "wino" (conv_precision("bf16_winograd")) | "parity" (BF16_UP4 = False)
# extra   family "impulse": ((py, px, c) per image);  kind "first": "xpad" | "wpad"

HS = (1, 7, 8, 9, 15, 16, 17)                  # each side of the 8-row block and of the row pair (i, i + TM)
WS = (1, 15, 16, 17, 31, 32, 33)               # each side of the 16-column block, one and two blocks
REDUCED = ((1, 1), (1, 33), (17, 1), (17, 33), (9, 17))
UP4_HW = ((1, 1), (7, 15), (8, 16), (9, 17), (17, 33))
GENERAL_OHW = ((1, 127), (1, 128), (1, 129), (3, 43), (16, 16), (17, 15))     # B = 2: M on each side of 128 and 256, 512, 510
SPADE_NNZ = 6
TIE_TARGETS = (257, 259, -257, -259, 385)
TIE_ROUNDED = (256, 260, -256, -260, 384)
TIE_ROW = 5                                    # the weight row (output channel) that carries the ties
TIE_AT = ((1, 1), (1, 5), (1, 9), (1, 13), (5, 1))
IMPULSE_CH = (0, 7, 8, 63, 64)                 # ... and Cin - 1, where the case has that many channels
PW_BM = {64: 256, 128: 128, 256: 64}           # rows per tile of lwg_conv_bf16_pw_kernel<NCH, WAVES_N, 2>: (8 / WAVES_N) * 2 * 32
C8_SECOND_PASS = ((245, 2141), (727, 727))     # the grid caps at 2048 workgroups of four 64-row groups: M = 2048 * 256 + 257 exactly, and 2048 * 256 + 4241


def _case(name, kind, B, H, W, C0, N, k=3, stride=1, C1=0, epi="plain", act="none", pad=0, family="ternary", route="default", extra=None):
    return Case(name, kind, B, H, W, C0, C1, N, k, stride, epi, act, pad, family, route, extra)


def _rng(case):
    return np.random.default_rng([20261021, 16, zlib.crc32(case.name.encode())])


def bf16_exact(t):
    t = torch.as_tensor(t).float()
    return bool(torch.equal(t.to(torch.bfloat16).float(), t))


def batch_of(i):
    """B in {1, 2, 3} in turn."""
    return 1 + i % 3


def out_hw(case):
    if case.kind == "convT":
        return 2 * case.H, 2 * case.W
    if case.k == 1:
        return (case.H - 1) // case.stride + 1, (case.W - 1) // case.stride + 1
    return (case.H + 2 - 3) // case.stride + 1, (case.W + 2 - 3) // case.stride + 1          # 3 x 3 pad 1; the 10-tap list is 3 x 5 pad (1, 2)


def out_channels(case):
    return case.N // 2 if case.epi == "spade" else case.N


def rows(case):
    """M of the launch: output pixels (a transposed convolution: per parity launch, = input pixels)."""
    if case.kind == "convT":
        return case.B * case.H * case.W
    oh, ow = out_hw(case)
    return case.B * oh * ow


def taps_of(case):
    if case.k == 1:
        return [(0, 0)]
    t = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    return t + [(0, 2)] if case.k == 10 else t


# ------------------------------------------------------------------------------------------------------------------------------ which form runs
Form = collections.namedtuple("Form", "entry kernel tile info")


def bf16_form(case, cus, hr=True, pw=True, c8=True, up4=True):
    """(entry point, kernel template, (rows, columns) of a workgroup's tile, details) of the launch - of each of the four parity launches where a
    transposed convolution runs as those - under conv_precision "bf16" ("bf16_winograd" for route "wino") and the given lab switches."""
    if case.route == "lds":
        hr = pw = False
    if case.route == "parity":
        up4 = False
    cin, N, M = case.C0 + case.C1, case.N, rows(case)
    if case.kind == "first":
        assert c8 and cin == 8 and N == 64 and len(taps_of(case)) <= 10 and case.C1 == 0 and case.epi == "plain"
        groups4 = (M + 255) // 256
        return Form("lwg_conv2d_nhwc_c8_bf16", "lwg_conv_c8_bf16_kernel", (256, 64), {"grid": min(groups4, 2048), "passes": -(-groups4 // 2048)})
    assert cin % 64 == 0 and N % 64 == 0, case
    if case.kind == "acc":
        assert case.k == 3 and case.stride == 1 and N % 128 == 0 and case.C1 == 0
        return Form("lwg_conv2d_nhwc_bf16_hr_acc", "lwg_conv_bf16_hr2_kernel<3,3,1,ACC>", (128, 128), {})
    if case.kind == "convT":
        if up4 and hr and cin in (64, 128) and case.C1 == 0:
            wm = 1 if N % 128 == 0 else 2
            return Form("lwg_conv_transpose4_nhwc_bf16", "lwg_conv_bf16_up4_kernel<%d,%d>" % (cin // 64, wm), (128, 128 // wm), {"launches": 1})
        ntaps, same_grid, stride = 4, True, 1
    else:
        ntaps, same_grid, stride = len(taps_of(case)), out_hw(case) == (case.H, case.W), case.stride
    if case.route == "wino" and ntaps == 9 and stride == 1 and same_grid and case.kind == "conv":
        return Form("lwg_conv2d_winograd_bf16", "lwg_conv_winograd_bf16_kernel", (256, 64), {})
    if hr and stride == 1 and ntaps in (9, 4) and same_grid:
        wm = 1 if N % 128 == 0 else 2
        g = 3 if ntaps == 9 else 2
        return Form("lwg_conv2d_nhwc_bf16_hr", "lwg_conv_bf16_hr2_kernel<%d,%d,%d>" % (g, g, wm), (128, 128 // wm), {"chunks": cin // 64})
    if pw and ntaps == 1 and stride == 1 and case.C1 == 0 and case.epi == "plain" and N == cin and N in (64, 128, 256) and same_grid:
        bm = PW_BM[N]
        tiles, slots = (M + bm - 1) // bm, 2 * cus
        return Form("lwg_conv2d_nhwc_bf16_hr", "lwg_conv_bf16_pw_kernel<%d,%d,2>" % (N // 64, N // 32), (bm, N),
                    {"tiles": tiles, "slots": slots, "walk": -(-tiles // slots)})
    entry = "lwg_conv2d_nhwc_bf16"
    if N % 256 == 0 and ((M + 255) // 256) * (N // 256) >= cus:
        return Form(entry, "lwg_conv_bf16_kernel<2,4,4,2>", (256, 256), {"tiles_m": (M + 255) // 256})
    small = N % 128 == 0 and ((M + 127) // 128) * (N // 128) < 2 * cus
    if case.epi == "spade" or (N % 128 == 0 and not small):
        assert case.epi != "spade" or N % 128 == 0
        return Form(entry, "lwg_conv_bf16_kernel<2,2,2,2>", (128, 128), {"tiles_m": (M + 127) // 128})
    return Form(entry, "lwg_conv_bf16_kernel<4,1,1,2>", (128, 64), {"tiles_m": (M + 127) // 128})


# ------------------------------------------------------------------------------------------------------------------------------ case lists
def hr2_cross(N):
    """The full size cross of the 3 x 3 plain epilogue at Cin = 64."""
    return [_case("hr2_cross_N%d_%dx%d" % (N, H, W), "conv", batch_of(i), H, W, 64, N) for i, (H, W) in enumerate((h, w) for h in HS for w in WS)]


def hr2_axes():
    """Channel chunks, the two-pointer concat, output widths, epilogues and channel slices of lwg_conv_bf16_hr2_kernel<3,3> on the reduced set."""
    out = []
    for i, (H, W) in enumerate(REDUCED):
        B = batch_of(i)
        for ch in (1, 2, 3, 4, 5, 6):
            out.append(_case("hr2_chunks%d_%dx%d" % (ch, H, W), "conv", B, H, W, 64 * ch, 128 if ch % 2 else 64))
        for C0, C1 in ((64, 128), (128, 64), (128, 256)):
            out.append(_case("hr2_cat%d+%d_%dx%d" % (C0, C1, H, W), "conv", B, H, W, C0, 64 if C1 == 64 else 128, C1=C1))
        for N in (64, 128, 192, 256):
            out.append(_case("hr2_N%d_%dx%d" % (N, H, W), "conv", B, H, W, 128, N, act="relu" if (H, W) == (9, 17) else "none"))
            out.append(_case("hr2_slice_N%d_%dx%d" % (N, H, W), "conv", B, H, W, 64, N, pad=16))
        for N in (64, 128):
            out.append(_case("hr2_res_N%d_%dx%d" % (N, H, W), "conv", B, H, W, 128, N, epi="res"))
        for YC in (64, 128):
            out.append(_case("hr2_spade_YC%d_%dx%d" % (YC, H, W), "conv", B, H, W, 128, 2 * YC, epi="spade"))
    out.append(_case("hr2_spade_relu", "conv", 2, 9, 17, 64, 128, epi="spade", act="relu"))
    out.append(_case("hr2_res_slice", "conv", 2, 9, 17, 64, 64, epi="res", pad=16))
    return out


def hr2_parity():
    """lwg_conv_bf16_hr2_kernel<2,2>: the four parity launches of transposed convolutions the fused kernel does not take (Cin > 128): omul = 2,
    ooy / oox in {0, 1}, four (even) and three (odd) channel chunks, both column forms."""
    out = []
    for i, (H, W) in enumerate(REDUCED):
        for cin, N in ((256, 64), (256, 128), (192, 64)):
            out.append(_case("hr2_par_C%d_N%d_%dx%d" % (cin, N, H, W), "convT", batch_of(i), H, W, cin, N, k=4))
    out.append(_case("hr2_par_relu", "convT", 2, 9, 17, 256, 64, k=4, act="relu"))
    return out


def hr2_acc():
    return [_case("hr2_acc", "acc", 1, 9, 17, 128, 128, family="dense")]


def up4_cases():
    out = []
    for i, (H, W) in enumerate(UP4_HW):
        for cin in (64, 128):
            for N in (64, 128, 192):
                out.append(_case("up4_C%d_N%d_%dx%d" % (cin, N, H, W), "convT", 2, H, W, cin, N, k=4, act="relu" if (i + N // 64) % 2 else "none"))
    out.append(_case("up4_slice_C64", "convT", 2, 9, 17, 64, 64, k=4, pad=16))
    out.append(_case("up4_slice_C128", "convT", 2, 9, 17, 128, 128, k=4, pad=16))
    return out


def _in_hw(ohw, stride, odd):
    """An input size whose 3 x 3 pad-1 convolution of this stride has the output size ohw (stride 2: the odd or the even one)."""
    return tuple(o if stride == 1 else 2 * o - (1 if odd else 0) for o in ohw)


def general_small(lds_route=False):
    """lwg_conv_bf16_kernel's 128 x 64 form (N % 128 != 0, or fewer than two 128 x 128 tiles per CU) and its forced 128 x 128 SPADE form: B = 2,
    so the m / HW split crosses an image inside a tile."""
    out = []
    for i, ohw in enumerate(GENERAL_OHW):
        H, W = _in_hw(ohw, 2, i % 2 == 0)
        out.append(_case("gen_s2_64to128_%dx%d" % ohw, "conv", 2, H, W, 64, 128, stride=2))
        out.append(_case("gen_s2_128to192_%dx%d" % ohw, "conv", 2, H, W, 128, 192, stride=2, act="relu" if i % 2 else "none"))
        out.append(_case("gen_1x1_128to256_%dx%d" % ohw, "conv", 2, ohw[0], ohw[1], 128, 256, k=1))
        out.append(_case("gen_1x1_64to192_%dx%d" % ohw, "conv", 2, ohw[0], ohw[1], 64, 192, k=1))
        out.append(_case("gen_s2_cat64+64_%dx%d" % ohw, "conv", 2, H, W, 64, 64, stride=2, C1=64))
        out.append(_case("gen_spade_%dx%d" % ohw, "conv", 2, ohw[0], ohw[1], 64, 128, epi="spade", route="lds"))
    out.append(_case("gen_s2_slice", "conv", 2, 33, 29, 64, 64, stride=2, pad=16))
    out.append(_case("gen_s2_res", "conv", 2, 33, 29, 64, 128, stride=2, epi="res"))
    return out


def general_lds_route():
    """The BF16_HR = BF16_PW = False route: everything on lwg_conv_bf16_kernel."""
    return [_case("lds_3x3_plain", "conv", 2, 17, 15, 128, 128, route="lds"),
            _case("lds_3x3_N64", "conv", 3, 9, 17, 192, 64, route="lds"),
            _case("lds_3x3_res", "conv", 2, 17, 15, 64, 128, epi="res", route="lds"),
            _case("lds_3x3_spade", "conv", 2, 17, 15, 128, 256, epi="spade", route="lds"),
            _case("lds_1x1_pw", "conv", 2, 17, 15, 128, 128, k=1, route="lds"),
            _case("lds_parity_C64", "convT", 2, 9, 17, 64, 64, k=4, route="lds"),
            _case("lds_parity_C256", "convT", 1, 17, 15, 256, 128, k=4, route="lds")]


def general_big(cus):
    """CU-count dependent forms of lwg_conv_bf16_kernel: the 8-wave 256 x 256 form (N = 256, one tile per CU and a ragged one of 37 rows) as a 1 x 1
    and as a 3 x 3 / stride 2 launch, and the 128 x 128 form on a plain epilogue (two tiles per CU, 3 rows more)."""
    M = 256 * cus + 37
    return [_case("big256_1x1_cus%d" % cus, "conv", 1, 1, M, 128, 256, k=1),
            _case("big256_s2_cus%d" % cus, "conv", 1, 2, 2 * M - 1, 64, 256, stride=2),
            _case("big128_1x1_cus%d" % cus, "conv", 1, 1, 2 * cus * 128 + 3, 64, 128, k=1)]


def pw_small():
    out = []
    for C, bm in PW_BM.items():
        for M in (1, bm - 1, bm, bm + 1, 2 * bm + 3):
            out.append(_case("pw_C%d_M%d" % (C, M), "conv", 1, 1, M, C, C, k=1, act="relu" if M == bm + 1 else "none"))
        out.append(_case("pw_slice_C%d" % C, "conv", 1, 3, bm // 2 + 1, C, C, k=1, pad=8))
    return out


def pw_persistent(cus, C):
    """More tiles than twice the workgroup slots, so some workgroups walk three tiles, and a ragged last tile."""
    return _case("pw_persist_C%d_cus%d" % (C, cus), "conv", 1, 1, (2 * cus * 2 + 1) * PW_BM[C] + 5, C, C, k=1)


def c8_small():
    out = []
    for i, ohw in enumerate(((1, 63), (1, 64), (1, 65), (5, 51), (16, 16), (1, 257))):       # M = B OH OW on each side of 64 and 256
        for k in (1, 3, 10):
            for stride in (1, 2):
                H, W = ohw if k == 1 and stride == 1 else (tuple(2 * o - 1 for o in ohw) if k == 1 else _in_hw(ohw, stride, i % 2 == 0))
                B = 1 if ohw[0] == 1 else batch_of(i)
                out.append(_case("c8_k%d_s%d_%dx%d" % (k, stride, ohw[0], ohw[1]), "first", B, H, W, 8, 64, k=k, stride=stride,
                                 act="relu" if i % 2 else "none", extra="xpad" if (i + k + stride) % 2 else "wpad"))
    return out


def c8_second_pass():
    return [_case("c8_second_pass_%dx%d" % hw, "first", 1, hw[0], hw[1], 8, 64, extra="wpad" if i else "xpad") for i, hw in enumerate(C8_SECOND_PASS)]


def wino_cross():
    return [c._replace(name="wino_" + c.name, route="wino") for c in hr2_cross(64)]


def wino_axes():
    out = []
    for i, (H, W) in enumerate(REDUCED):
        B = batch_of(i)
        for ch in (2, 4):
            out.append(_case("wino_chunks%d_%dx%d" % (ch, H, W), "conv", B, H, W, 64 * ch, 64, route="wino"))
        out.append(_case("wino_cat64+64_%dx%d" % (H, W), "conv", B, H, W, 64, 64, C1=64, route="wino"))
        for N in (128, 192):
            out.append(_case("wino_N%d_%dx%d" % (N, H, W), "conv", B, H, W, 64, N, route="wino", act="relu" if (H, W) == (9, 17) else "none"))
        out.append(_case("wino_res_%dx%d" % (H, W), "conv", B, H, W, 64, 64, epi="res", route="wino"))
        out.append(_case("wino_spade_%dx%d" % (H, W), "conv", B, H, W, 128, 128, epi="spade", route="wino"))
        out.append(_case("wino_slice_%dx%d" % (H, W), "conv", B, H, W, 64, 64, pad=16, route="wino"))
    return out


def tie_cases():
    """One case per store path: store_dt's packed path (the plain epilogue of the halo-tile kernel and of the LDS-DMA kernel), the SPADE uintx2 path
    of both, and the first-layer kernel's."""
    return [_case("tie_hr2_plain", "conv", 1, 9, 17, 64, 64, family="tie"),
            _case("tie_hr2_spade", "conv", 1, 9, 17, 64, 128, epi="spade", family="tie"),
            _case("tie_lds_plain", "conv", 1, 9, 17, 64, 128, family="tie", route="lds"),
            _case("tie_lds_spade", "conv", 1, 9, 17, 64, 128, epi="spade", family="tie", route="lds"),
            _case("tie_c8", "first", 1, 9, 17, 8, 64, family="tie", extra="wpad")]


def _place(pixels, cin):
    """(py, px, c) per image: the pixels in turn, the channels IMPULSE_CH and Cin - 1 in turn, every pixel as often as any other."""
    ch = [c for c in IMPULSE_CH if c < cin - 1] + [cin - 1]
    n = -(-max(len(ch), len(pixels)) // len(pixels)) * len(pixels)
    return tuple(tuple(pixels[i % len(pixels)]) + (ch[i % len(ch)],) for i in range(n))


def impulse_cases():
    """One per kernel (none for the Winograd kernel, whose transformed weights G w G^T of a coded weight are not bf16 values): image i carries one
    impulse, on each side of a block corner - (8, 16) of the halo-tile kernels, row 128 of the linear kernels' tiles, 64 / 256 of the first layer's."""
    corner = ((7, 15), (7, 16), (8, 15), (8, 16))
    lin = ((3, 28), (3, 29), (7, 24), (7, 25))                # W = 33: m = 127, 128, 255, 256
    pwp = ((0, 127), (0, 128), (0, 255), (0, 256))
    c8p = ((0, 63), (0, 64), (2, 55), (2, 56))                # W = 100: m = 63, 64, 255, 256
    return _impulse_list(corner, lin, pwp, c8p)


def _impulse_list(corner, lin, pwp, c8p):
    def mk(name, kind, H, W, cin, N, px, **kw):
        return _case(name, kind, len(_place(px, cin)), H, W, cin, N, family="impulse", extra=_place(px, cin), **kw)
    return [mk("imp_hr2", "conv", 17, 33, 128, 64, corner),
            mk("imp_hr2_par", "convT", 17, 33, 256, 64, corner, k=4),
            mk("imp_up4", "convT", 9, 17, 128, 64, corner, k=4),
            mk("imp_lds_3x3", "conv", 9, 33, 128, 64, lin, route="lds"),
            mk("imp_gen_s2", "conv", 17, 33, 128, 64, corner, stride=2),
            mk("imp_pw", "conv", 1, 300, 128, 128, pwp, k=1),
            mk("imp_c8", "first", 3, 100, 8, 64, c8p)]


def gaussian_cases():
    """Two launches of gpu_checks.check_bf16_conv_kernels with its data (``_bf16_kernel_case``: seed 1000 + index), for the record of what its
    1.2e-2 criterion lets through."""
    return [_case("gauss_3x3_64to128", "conv", 2, 20, 36, 64, 128, act="relu", family="gauss", extra=1000),
            _case("gauss_3x3_256to256", "conv", 1, 16, 16, 256, 256, act="relu", family="gauss", extra=1001)]


GAUSS_TOL = 1.2e-2


# ------------------------------------------------------------------------------------------------------------------------------ operands
def _ternary(rng, shape):
    return torch.tensor(rng.integers(-1, 2, shape).astype(np.float32))


def _ints(rng, lo, hi, shape):
    return torch.tensor(rng.integers(lo, hi + 1, shape).astype(np.float32))


def _sparse_rows(rng, shape, nnz):
    """(rows, ...) ternary with exactly ``nnz`` non-zeros per row."""
    w = np.zeros((shape[0], int(np.prod(shape[1:]))), np.float32)
    for r in range(shape[0]):
        w[r, rng.choice(w.shape[1], nnz, replace=False)] = rng.choice([-1.0, 1.0], nnz)
    return torch.tensor(w.reshape(shape))


def impulse_code(n):
    """n distinct bf16 values (the normal ones, positive then negative; past 65024 the sequence repeats) as float32."""
    i = np.arange(n) % 65024
    pat = (0x0080 + i % 32512) | np.where(i >= 32512, 0x8000, 0)
    return torch.tensor(pat.astype(np.uint16).view(np.int16)).view(torch.bfloat16).float()


def weight_shape(case):
    cin = case.C0 + case.C1
    if case.kind == "convT":
        return (cin, case.N, 4, 4)
    return (case.N, cin, 1, 1) if case.k == 1 else (case.N, cin, 3, 5 if case.k == 10 else 3)


def _tap_mask(case):
    """1 at the kernel positions that are taps (all, but for the 10-tap list inside its 3 x 5 window)."""
    shape = weight_shape(case)
    m = torch.ones(shape[2:])
    if case.k == 10:
        m.zero_()
        for dy, dx in taps_of(case):
            m[dy + 1, dx + 2] = 1
    return m


@functools.lru_cache(maxsize=64)
def operands(case):
    """CPU float32 tensors of a case (NHWC activations, torch-layout weights): x0, x1, w, bias and the epilogue's.  SPADE: w / bias are None and
    wg, bg, wb, bb the two convolutions' (the panel is packing.pack_spade_gamma_beta's)."""
    rng = _rng(case)
    B, H, W, cin = case.B, case.H, case.W, case.C0 + case.C1
    oh, ow = out_hw(case)
    o = {"x1": None, "res": None}
    ws = weight_shape(case)
    if case.epi == "spade":
        ws = (case.N // 2,) + ws[1:]
    if case.family == "gauss":
        g = torch.Generator().manual_seed(case.extra)
        rnd = lambda *sh, sc=1.0: (torch.randn(*sh, generator=g) * sc).to(torch.bfloat16).float()          # noqa: E731
        x = rnd(B, H, W, cin)
        o["w"], o["bias"] = rnd(*ws, sc=(cin * 9) ** -0.5), 0.1 * torch.randn(case.N, generator=g)
    elif case.family == "dense":
        x, o["w"], o["bias"] = _ints(rng, -4, 4, (B, H, W, cin)), _ints(rng, -2, 2, ws), None
    elif case.family == "impulse":
        x = torch.zeros(B, H, W, cin)
        for b, (py, px, c) in enumerate(case.extra):
            x[b, py, px, c] = 1.0
        o["w"], o["bias"] = impulse_code(int(np.prod(ws))).reshape(ws) * _tap_mask(case), torch.zeros(case.N)
    elif case.family == "tie":
        x = torch.zeros(B, H, W, cin)
        for (cy, cx), t in zip(TIE_AT, TIE_TARGETS):
            s, r = (1.0 if t > 0 else -1.0), abs(t) - 1            # bias 1 (of sign s): r = 256 | 258 | 384 from the 3 x 3 neighbourhood
            x[0, cy, cx, 0] = x[0, cy, cx + 1, 0] = 128 * s
            if r == 384:
                x[0, cy + 1, cx, 0] = 128 * s
            elif r % 256:
                x[0, cy - 1, cx - 1, 0] = (r % 256) * s
        # the biased row reads +1; negative targets need the bias -1: a second row, TIE_ROW + 1, carries the same weights with bias -1
        w, bias = _ternary(rng, ws), _ints(rng, -8, 8, (ws[0],))
        w[TIE_ROW:TIE_ROW + 2] = 0
        w[TIE_ROW:TIE_ROW + 2, 0] = 1
        bias[TIE_ROW], bias[TIE_ROW + 1] = 1, -1
        o["w"], o["bias"] = w, bias
    else:
        x = _ternary(rng, (B, H, W, cin))
        o["w"], o["bias"] = _ternary(rng, ws) * _tap_mask(case), _ints(rng, -8, 8, (case.N,))
    if case.kind == "first" and case.family != "impulse":           # channels 6, 7: live input on zero weights, or the other way round
        if case.extra == "xpad":
            o["w"][:, 6:] = 0
        else:
            x[..., 6:] = 0
    if case.epi == "res":
        o["res"] = _ints(rng, -8, 8, (B, oh, ow, case.N))
    if case.epi == "spade":
        YC = case.N // 2
        if case.family == "tie":        # out = beta: gamma = 0, xn = mean = 0
            o["wg"], o["bg"], o["wb"], o["bb"] = torch.zeros(YC, cin, 3, 3), torch.zeros(YC), o["w"], o["bias"]
            o["xn"], o["mean"], o["rstd"] = torch.zeros(B, oh, ow, YC), torch.zeros(B, YC), torch.ones(B, YC)
        else:
            o["wg"], o["wb"] = _sparse_rows(rng, (YC, cin, 3, 3), SPADE_NNZ), _sparse_rows(rng, (YC, cin, 3, 3), SPADE_NNZ)
            o["bg"], o["bb"] = _ints(rng, -8, 8, (YC,)), _ints(rng, -8, 8, (YC,))
            o["xn"], o["mean"], o["rstd"] = _ints(rng, -5, 5, (B, oh, ow, YC)), _ints(rng, -3, 3, (B, YC)), _ints(rng, 1, 2, (B, YC))
        o["w"] = o["bias"] = None
    o["x0"] = x[..., :case.C0].contiguous()
    if case.C1:
        o["x1"] = x[..., case.C0:].contiguous()
    return o


def _nchw(t, dtype):
    return t.to(dtype).permute(0, 3, 1, 2)


def _conv(case, x, w, bias, dtype):
    """torch's convolution of the NHWC tensor x (all input channels) -> NHWC."""
    xn, w = _nchw(x, dtype), w.to(dtype)
    bias = None if bias is None else bias.to(dtype)
    if case.kind == "convT":
        y = F.conv_transpose2d(xn, w, bias, stride=2, padding=1)
    elif case.k == 1:
        y = F.conv2d(xn, w, bias, stride=case.stride)
    else:
        y = F.conv2d(xn, w, bias, stride=case.stride, padding=(1, 2) if case.k == 10 else 1)
    return y.permute(0, 2, 3, 1).contiguous()


def _epilogue(case, o, y, gamma_beta=None):
    """The fused epilogue on the pre-activations y (NHWC, bias included) in y's dtype."""
    if case.epi == "res":
        y = y + o["res"].to(y.dtype)
    elif case.epi == "spade":
        gamma, beta = gamma_beta
        dt = gamma.dtype
        y = (o["xn"].to(dt) - o["mean"].to(dt)[:, None, None, :]) * o["rstd"].to(dt)[:, None, None, :] * (1 + gamma) + beta
    return torch.relu(y) if case.act == "relu" else y


def _cat(o):
    return o["x0"] if o["x1"] is None else torch.cat([o["x0"], o["x1"]], dim=3)


@functools.lru_cache(maxsize=8)
def reference(case, dtype=torch.float64):
    """The exact result (B, OH, OW, out_channels) in ``dtype``: torch's conv2d / conv_transpose2d on the CPU and the epilogue."""
    o = operands(case)
    x = _cat(o)
    if case.epi == "spade":
        return _epilogue(case, o, None, (_conv(case, x, o["wg"], o["bg"], dtype), _conv(case, x, o["wb"], o["bb"], dtype)))
    return _epilogue(case, o, _conv(case, x, o["w"], o["bias"], dtype))


def expected_bf16(case, dtype=torch.float64):
    """What the kernel must store: the reference, which on the exact families IS a bf16 frame (asserted here, on the reference); the tie family:
    torch's round-to-nearest-even of it."""
    ref = reference(case, dtype).float()
    if case.family == "tie":
        return ref.to(torch.bfloat16)
    assert case.family in ("ternary", "impulse"), case
    assert bf16_exact(ref), "%s: a reference value is not a bf16 value (max |ref| %g): change the seed or thin the weights" % (case.name, ref.abs().max())
    return ref.to(torch.bfloat16)


def assert_family(case):
    """The family's conditions on a case: bf16-exact operands, integer bounds, a bf16-exact reference that float32 reproduces bit for bit."""
    o = operands(case)
    for k, t in o.items():
        assert t is None or bf16_exact(t), (case.name, k)
    if case.family == "ternary":
        assert float(_cat(o).abs().max()) <= 1, case.name
        for k, bound in (("w", 1), ("wg", 1), ("wb", 1), ("bias", 8), ("bg", 8), ("bb", 8), ("res", 8), ("xn", 5), ("mean", 3), ("rstd", 2)):
            t = o.get(k)
            assert t is None or (float(t.abs().max()) <= bound and torch.equal(t, t.round())), (case.name, k)
        if case.epi == "spade":
            x = _cat(o)
            for w, b in ((o["wg"], o["bg"]), (o["wb"], o["bb"])):
                assert int((w != 0).flatten(1).sum(1).max()) == SPADE_NNZ and float(_conv(case, x, w, b, torch.float64).abs().max()) <= 15, case.name
            assert float(o["rstd"].min()) >= 1
    r64, r32 = reference(case, torch.float64), reference(case, torch.float32)
    assert torch.equal(r32.double(), r64), case.name + ": the float32 reference is not the float64 one"
    if case.family in ("ternary", "dense"):
        assert torch.equal(r64, r64.round()), case.name
    if case.family == "ternary":
        assert float(r64.abs().max()) <= 256, (case.name, float(r64.abs().max()))
    if case.family != "dense":
        expected_bf16(case)
    if case.family == "tie":
        picks = [reference(case)[0, cy, cx, TIE_ROW + (t < 0)].item() for (cy, cx), t in zip(TIE_AT, TIE_TARGETS)]
        assert tuple(picks) == TIE_TARGETS, (case.name, picks)
        got = [expected_bf16(case)[0, cy, cx, TIE_ROW + (t < 0)].item() for (cy, cx), t in zip(TIE_AT, TIE_TARGETS)]
        assert tuple(got) == TIE_ROUNDED, (case.name, got)


def acc_frame_columns(N):
    """lwg_conv2d_nhwc_bf16_hr_acc's frame (lwg_bf16_hr_list.h: hrl_acc_offset / hrl_acc_column): per pixel the N accumulators, each 32-column tile
    stored [khalf][r] - position 32 t + 16 khalf + r holds the panel's column 32 t + 8 (r / 4) + 4 khalf + r % 4.  -> that column per position."""
    p = torch.arange(N)
    t, khalf, r = p // 32, (p % 32) // 16, p % 16
    return 32 * t + 8 * (r // 4) + 4 * khalf + r % 4


def impulse_decode(case, value):
    """The (n | cin index, ...) positions of the coded weight tensor (torch layout) that hold ``value``: which weight an impulse output read."""
    w = operands(case)["w"]
    return [tuple(int(i) for i in idx) for idx in (w == float(value)).nonzero()]


# ------------------------------------------------------------------------------------------------------------------------------ planted faults
FAULTS = ("drop_tap_row", "drop_tap_col", "halo_neighbour", "skip_last_odd_chunk", "swap_concat", "bias_next_tile", "parity_swap", "pw_stale_tile")
_CT = {0: ((1, 0), (3, -1)), 1: ((0, 1), (2, 0))}      # ConvTranspose2d(4, 2, 1): output parity -> ((kernel index, input offset), ...)


def covers(case, cus=256):
    """The planted faults this case claims to expose."""
    if case.kind in ("acc",) or case.family in ("impulse", "tie", "dense") or case.route == "wino":
        return set()
    oh, ow = out_hw(case)
    s = {"drop_tap_row", "bias_next_tile"}
    ow_launch = case.W if case.kind == "convT" else ow
    if ow_launch >= 16:
        s.add("drop_tap_col")
    if case.stride == 1 and case.k != 1 and case.W >= 16 and case.kind != "first":
        s.add("halo_neighbour")
    if case.kind != "first" and ((case.C0 + case.C1) // 64) % 2 == 1:
        s.add("skip_last_odd_chunk")
    if case.C1:
        s.add("swap_concat")
    if case.kind == "convT":
        s.add("parity_swap")
    f = bf16_form(case, cus) if case.kind != "first" else None
    if f is not None and "pw_kernel" in f.kernel and f.info["walk"] > 1:
        s.add("pw_stale_tile")
    return s


def _shifted(xp, P, dy, dx, oh, ow, stride):
    """xp: x zero-padded by P on both sides of H and W -> the pixels (oy stride + dy, ox stride + dx)."""
    return xp[:, P + dy: P + dy + (oh - 1) * stride + 1: stride, P + dx: P + dx + (ow - 1) * stride + 1: stride]


def _restated_taps(x, taps, wt, oh, ow, stride, fault, chunk, width):
    """sum over (channel chunk, tap) of x[oy s + dy, ox s + dx, chunk] @ wt[tap][chunk] in float64, with the tap-level faults."""
    B, H, W, cin = x.shape
    P = 16
    xp = F.pad(x, (0, 0, P, P, P, P))
    nch = max(1, cin // chunk)
    y = x.new_zeros(B, oh, ow, wt[0].shape[1])
    oy, ox = torch.arange(oh)[:, None], torch.arange(ow)[None, :]
    for ci in range(nch):
        if fault == "skip_last_odd_chunk" and nch % 2 == 1 and ci == nch - 1:
            continue
        cs = slice(ci * chunk, cin if ci == nch - 1 else (ci + 1) * chunk)
        for t, (dy, dx) in enumerate(taps):
            g = _shifted(xp, P, dy, dx, oh, ow, stride)[..., cs]
            if fault == "halo_neighbour" and dx == -1:          # block column 0 reads its own last column where its left neighbour's belongs
                wrong = _shifted(xp, P, dy, dx + 16, oh, ow, stride)[..., cs]
                g = torch.where(((ox % 16 == 0) & (oy >= 0))[None, :, :, None], wrong, g)
            c = g @ wt[t][cs]
            if fault in ("drop_tap_row", "drop_tap_col") and ci == 0 and (dy, dx) == (0, 0):      # this tap of the first ``width`` channels
                lost = g[..., :width] @ wt[t][cs][:width]
                seam = (oy % 8 == 0) & (ox >= 0) if fault == "drop_tap_row" else (ox % 16 == 15) & (oy >= 0)
                c = c - lost * seam[None, :, :, None]
            y = y + c
    return y


def restated(case, fault=None, cus=256, width=8):
    """The case's result (float64) from a plain statement of the convolution - 64-channel chunks outside, taps inside - with one planted fault.
    width: how many channels of the centre tap the two drop faults lose along their seam (8: one 16-byte k-octet; 1: a single product)."""
    o = operands(case)
    f64 = torch.float64
    x = _cat(o).to(f64)
    if fault == "swap_concat" and case.C1:
        x = torch.cat([o["x1"], o["x0"]], dim=3).to(f64)
    chunk = 64 if case.kind != "first" else 8
    roll = (lambda b: torch.roll(b, -32)) if fault == "bias_next_tile" else (lambda b: b)

    def conv(w, bias):
        w = w.to(f64)
        if case.kind == "convT":
            y = x.new_zeros(case.B, 2 * case.H, 2 * case.W, case.N)
            for py in (0, 1):
                for px in (0, 1):
                    taps = [(dy, dx) for _, dy in _CT[py] for _, dx in _CT[px]]
                    wt = [w[:, :, ky, kx] for ky, _ in _CT[py] for kx, _ in _CT[px]]
                    part = _restated_taps(x, taps, wt, case.H, case.W, 1, fault, chunk, width)
                    qy, qx = (px, py) if fault == "parity_swap" else (py, px)
                    y[:, qy::2, qx::2] = part
        else:
            taps = taps_of(case)
            wt = [w[:, :, 0, 0].t()] if case.k == 1 else [w[:, :, dy + 1, dx + (2 if case.k == 10 else 1)].t() for dy, dx in taps]
            oh, ow = out_hw(case)
            if fault == "pw_stale_tile":
                form = bf16_form(case, cus)
                bm, slots = form.tile[0], form.info["slots"]
                xr = x.reshape(-1, x.shape[3]).clone()
                src = xr.clone()
                for t in range(slots, form.info["tiles"]):             # tile t of a workgroup's walk reads the stage that still holds tile t - slots
                    n = min(bm, xr.shape[0] - t * bm)
                    xr[t * bm: t * bm + n] = src[(t - slots) * bm: (t - slots) * bm + n]
                y = (xr @ wt[0]).reshape(case.B, oh, ow, case.N)
            else:
                y = _restated_taps(x, taps, wt, oh, ow, case.stride, fault, chunk, width)
        return y if bias is None else y + roll(bias.to(f64))

    if case.epi == "spade":
        g, b = conv(o["wg"], o["bg"]), conv(o["wb"], o["bb"])
        if fault == "bias_next_tile":        # the gamma | beta interleave: the next 32-column tile of a gamma block is its beta block
            g, b = b, g
        return _epilogue(case, o, None, (g, b))
    return _epilogue(case, o, conv(o["w"], o["bias"]))


def gauss_rel(case, got):
    """``_bf16_kernel_case``'s figure: max |bf16(got) - reference| over the reference's maximum."""
    want = reference(case)
    return float((got.float().to(torch.bfloat16).double() - want).abs().max() / want.abs().max())
