"""The definition of the opt-in bf16-operand forward / data-gradient convolution (csrc/conv_igemm_bf16op.hip, ops.conv_precision("bf16_operands"),
DESIGN 3.10d), shared by the CPU tests and the GPU kernel tests:

    y = epilogue(conv(bf16(x), bf16(w)) accumulated in fp32 + bias)

both fp32 operands rounded to bf16 (round to nearest even: tensor.bfloat16()), the products - exact in fp32 - accumulated in fp32, the bias added in
fp32.  x (B, H, W, Cin) and y (B, OH, OW, N) are NHWC like the kernel's tensors; w is nn.Conv2d's (N, Cin, k, k).

The two bounds (theorems, not tuned numbers; operands in fp32's normal range; T = ntaps * Cin + 1 terms per output - the products and the bias; S and
S^ = the fp64 convolution of the absolute operands plus |bias|, as given and rounded):
  accumulation  |kernel - rounded_reference| <= 2 (T + 8) 2^-24 S^: any order of T fp32 additions - the split-K one, partial sums added in slice
                order, included - is within (T - 1) u S^ of the exact sum (u = 2^-24, Higham's gamma_n to first order); the factor 2 covers an adder
                that truncates;
  rounding      |kernel - reference| <= (2^-7 + 2^-16) S + the accumulation bound: bf16 has 8 significant bits, unit roundoff 2^-8, so a product of
                two rounded values is off by at most ((1 + 2^-8)^2 - 1) |x w|.
ReLU is 1-Lipschitz: both bounds carry through it.  The ReLU mask (y = res > 0 ? acc + bias : 0): the bounds where res > 0, exact zeros elsewhere.
A plain residual (y = act(acc + bias + res)) is one more fp32 term: T + 1 terms, |res| joins S and S^ (res is not rounded).
"""
import torch
import torch.nn.functional as F

U_ACC = 2.0 ** -24
U_PROD = 2.0 ** -7 + 2.0 ** -16
ACT_NONE, ACT_RELU, ACT_RELU_MASK = 0, 1, 5


def rounded(t):
    """The operand as the kernel's matrix instruction sees it: bf16, round to nearest even, back in fp32 (exact)."""
    return t.bfloat16().float()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _conv(x, w, bias, stride, pad, dtype):
    y = F.conv2d(x.to(dtype).permute(0, 3, 1, 2).contiguous(), w.to(dtype), None if bias is None else bias.to(dtype), stride=stride, padding=pad)
    return _nhwc(y)


def epilogue(acc, act=ACT_NONE, res=None):
    """acc = conv + bias -> y.  res with ACT_RELU_MASK: the mask source; res otherwise: added before the activation."""
    if act == ACT_RELU_MASK:
        return torch.where(res > 0, acc, torch.zeros_like(acc))
    if res is not None:
        acc = acc + res.to(acc.dtype)
    return acc.relu() if act == ACT_RELU else acc


def reference(x, w, bias=None, k=3, stride=1, pad=1, act=ACT_NONE, res=None):
    """fp64 convolution of the operands as given -> (B, OH, OW, N)."""
    return epilogue(_conv(x, w, bias, stride, pad, torch.float64), act, res)


def rounded_reference(x, w, bias=None, k=3, stride=1, pad=1, act=ACT_NONE, res=None):
    """The same of x.bfloat16() and w.bfloat16() (the bias as given): what the kernel computes, up to the order and rounding of its fp32 additions."""
    return epilogue(_conv(rounded(x), rounded(w), bias, stride, pad, torch.float64), act, res)


def emulate(x, w, bias=None, k=3, stride=1, pad=1, act=ACT_NONE, res=None):
    """bf16 operands, fp32 accumulation in torch's own order: a second evaluation of the definition, held to the same two bounds."""
    return epilogue(_conv(rounded(x), rounded(w), bias, stride, pad, torch.float32), act, res)


def bounds_of(T, S_hat, S):
    """-> (accumulation bound, rounding bound) from the fp64 convolutions of the absolute operands (+ |bias|), rounded (S_hat) and as given (S)."""
    acc = 2.0 * (T + 8) * U_ACC * S_hat
    return acc, U_PROD * S + acc


def bounds(x, w, bias=None, k=3, stride=1, pad=1, res=None):
    """-> (accumulation bound, rounding bound), elementwise (B, OH, OW, N) in fp64.  res: a plain residual (one more term), None for the ReLU mask."""
    T = w.shape[2] * w.shape[3] * w.shape[1] + 1 + (res is not None)
    ab = None if bias is None else bias.abs()
    S_hat, S = _conv(rounded(x).abs(), rounded(w).abs(), ab, stride, pad, torch.float64), _conv(x.abs(), w.abs(), ab, stride, pad, torch.float64)
    if res is not None:
        S_hat, S = S_hat + res.double().abs(), S + res.double().abs()
    return bounds_of(T, S_hat, S)


def _convt(x, w, dtype, output_padding=0):
    return _nhwc(F.conv_transpose2d(x.to(dtype).permute(0, 3, 1, 2).contiguous(), w.to(dtype), stride=2, padding=1, output_padding=output_padding))


def convt_reference(x, w, output_padding=0):
    """fp64 nn.ConvTranspose2d(4, 2, 1): x (B, H, W, Cin) NHWC, w (Cin, N, 4, 4) -> (B, 2H (+ output_padding), .., N).  With w = a Conv2d(4, 2, 1) weight
    (N', Cin', 4, 4) and x = its output gradient this is that convolution's data gradient (output_padding 1 for an odd input size)."""
    return _convt(x, w, torch.float64, output_padding)


def convt_rounded_reference(x, w, output_padding=0):
    return _convt(rounded(x), rounded(w), torch.float64, output_padding)


def convt_bounds(x, w, output_padding=0):
    """The two bounds for the transposed convolution, built the same way: an output pixel sees 2 x 2 taps: T = 4 * Cin + 1 (no bias: the + 1 is slack)."""
    T = 4 * w.shape[0] + 1
    return bounds_of(T, _convt(rounded(x).abs(), rounded(w).abs(), torch.float64, output_padding), _convt(x.abs(), w.abs(), torch.float64, output_padding))


def inside(got, ref, rref, bnds, where=None):
    """-> (inside both bounds everywhere [where the mask holds], err / accumulation bound, err / rounding bound) of a result against the references."""
    acc, rnd = bnds
    g = got.double().cpu()
    ea, er = (g - rref).abs(), (g - ref).abs()
    if where is not None:
        ea, er = ea[where], er[where]
        acc, rnd = acc[where], rnd[where]
    fa = float((ea / acc.clamp_min(1e-300)).max()) if ea.numel() else 0.0
    fr = float((er / rnd.clamp_min(1e-300)).max()) if er.numel() else 0.0
    return bool((ea <= acc).all()) and bool((er <= rnd).all()), fa, fr


# The kernel matrix of tests/test_gpu_conv_bf16op.py, held by the emulation too (tests/test_conv_bf16op_cpu.py):
# ((B, H, W, C0, C1, N), (k, stride, pad), (YC, ycoff) of a wider output or None)
BIG = ((1, 128, 128, 128, 0, 128), (3, 1, 1), None)          # full 128 x 128 tiles
MATRIX = [
    ((1, 3, 5, 64, 0, 64), (3, 1, 1), None),                 # 15 rows: less than a tile
    ((3, 9, 7, 64, 0, 64), (3, 1, 1), None),                 # odd sizes, tiles straddle images
    ((2, 16, 32, 64, 0, 128), (3, 1, 1), None),              # two 64-column tiles
    ((1, 32, 32, 64, 0, 192), (3, 1, 1), None),              # N % 128 != 0
    ((1, 16, 16, 128, 256, 256), (3, 1, 1), None),           # two inputs
    ((1, 8, 8, 32, 96, 64), (3, 1, 1), None),                # two inputs, 32-granular
    ((2, 9, 9, 64, 0, 64), (3, 2, 1), None),                 # stride 2
    ((1, 16, 16, 64, 0, 128), (4, 2, 1), None),              # the discriminator's layers
    ((2, 8, 8, 96, 0, 64), (1, 1, 0), None),                 # single tap
    ((1, 16, 16, 64, 0, 64), (3, 1, 1), (128, 64)),          # written into channels 64..127 of a 128-channel y
    BIG,
]
SPLITK = [((1, 16, 16, 512, 0, 512), (3, 1, 1), None), ((1, 64, 64, 256, 0, 256), (3, 1, 1), None)]      # the plan must split these
MASK_SHAPE = ((2, 16, 16, 64, 0, 64), (3, 1, 1), None)
KINDS = ["randn", "dc10", "dc100", "post_relu", "chan_scales", "dy_1e-3", "student_t_dy"]
KINDS_SHAPE = ((2, 32, 32, 128, 0, 128), (3, 1, 1), None)


def out_hw(H, W, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def operands(kind, sx, sw, seed):
    """Seeded fp32 operands of one kind - the seven kinds of tests/wgradbf16_emu.operands with the weights in the role of dy (scaled by
    1 / sqrt(fan-in) first: a layer's weights) -, all within fp32's normal range."""
    g = torch.Generator().manual_seed(seed)
    x, w = torch.randn(sx, generator=g), torch.randn(sw, generator=g) / float(sw[1] * sw[2] * sw[3]) ** 0.5
    if kind == "dc10":
        x = x + 10.0
    elif kind == "dc100":
        x = x + 100.0
    elif kind == "post_relu":
        x = x.relu()
    elif kind == "chan_scales":
        x = x * torch.logspace(-2, 2, sx[3]).view(1, 1, 1, -1)
    elif kind == "dy_1e-3":
        w = w * 1e-3
    elif kind == "student_t_dy":
        chi2 = sum(torch.randn(sw, generator=g).pow(2) for _ in range(3))           # Student-t, 3 degrees of freedom: z / sqrt(chi2_3 / 3)
        w = w / torch.sqrt(chi2 / 3.0)
    else:
        assert kind == "randn", kind
    return x.contiguous(), w.contiguous()


def case(shape, geom, kind="randn"):
    """-> (x, w, bias, res): the operands of a matrix case; bias (N,) and res (B, OH, OW, N) for the tests that use them."""
    B, H, W, C0, C1, N = shape
    k, stride, pad = geom
    seed = 1900 + H + C0 + C1 + N + 7 * k + stride
    x, w = operands(kind, (B, H, W, C0 + C1), (N, C0 + C1, k, k), seed)
    g = torch.Generator().manual_seed(seed + 1)
    OH, OW = out_hw(H, W, k, stride, pad)
    return x, w, 0.1 * torch.randn(N, generator=g), torch.randn((B, OH, OW, N), generator=g)
