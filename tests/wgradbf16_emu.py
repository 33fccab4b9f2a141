"""The definition of the opt-in bf16-operand weight gradient (csrc/conv_wgrad_bf16.hip, ops.wgrad_mode("bf16")), shared by the CPU
tests and the GPU kernel tests: both fp32 operands are rounded to bf16 (round to nearest even: tensor.bfloat16()), the products - exact in fp32 - are
accumulated in fp32.  x (B, H, W, Cin) and dy (B, OH, OW, N) are NHWC like the kernel's operands; results are nn.Conv2d's (N, Cin, k, k).

The two bounds (theorems, not tuned numbers; operands in fp32's normal range, T = B * OH * OW terms per weight element):
  accumulation  |kernel - rounded_reference| <= 2 (T + 8) 2^-24 S^,  S^ = conv2d_weight(|x^|, |dy^|) in fp64: any order of T fp32 additions is within
                (T - 1) u S^ of the exact sum (u = 2^-24, Higham's gamma_n to first order); the factor 2 covers an adder that truncates;
  rounding      |kernel - reference| <= (2^-7 + 2^-16) S + the accumulation bound,  S = conv2d_weight(|x|, |dy|): bf16 has 8 significant bits, unit
                roundoff 2^-8, so a product of two rounded values is off by at most ((1 + 2^-8)^2 - 1) |x dy|.
"""
import torch

U_ACC = 2.0 ** -24
U_PROD = 2.0 ** -7 + 2.0 ** -16


def _w(x, dy, k, stride, pad, dtype):
    xn, dn = x.to(dtype).permute(0, 3, 1, 2).contiguous(), dy.to(dtype).permute(0, 3, 1, 2).contiguous()
    return torch.nn.grad.conv2d_weight(xn, (dy.shape[3], x.shape[3], k, k), dn, stride=stride, padding=pad)


def rounded(t):
    """The operand as the kernel's matrix instruction sees it: bf16, round to nearest even, back in fp32 (exact)."""
    return t.bfloat16().float()


def reference(x, dy, k=3, stride=1, pad=1):
    """fp64 torch.nn.grad.conv2d_weight of the operands as given -> (N, Cin, k, k)."""
    return _w(x, dy, k, stride, pad, torch.float64)


def rounded_reference(x, dy, k=3, stride=1, pad=1):
    """The same of x.bfloat16() and dy.bfloat16(): what the kernel computes, up to the order and rounding of its fp32 additions."""
    return _w(rounded(x), rounded(dy), k, stride, pad, torch.float64)


def emulate(x, dy, k=3, stride=1, pad=1):
    """bf16 operands, fp32 accumulation in torch's own order: a second evaluation of the definition, held to the same two bounds."""
    return _w(rounded(x), rounded(dy), k, stride, pad, torch.float32)


def bounds_of(T, S_hat, S):
    """-> (accumulation bound, rounding bound) from the fp64 weight gradients of the absolute operands, rounded (S_hat) and as given (S)."""
    acc = 2.0 * (T + 8) * U_ACC * S_hat
    return acc, U_PROD * S + acc


def bounds(x, dy, k=3, stride=1, pad=1):
    """-> (accumulation bound, rounding bound), elementwise (N, Cin, k, k) in fp64."""
    T = dy.shape[0] * dy.shape[1] * dy.shape[2]
    return bounds_of(T, _w(rounded(x).abs(), rounded(dy).abs(), k, stride, pad, torch.float64), _w(x.abs(), dy.abs(), k, stride, pad, torch.float64))


def convt_weight(x, dy):
    """fp64 weight gradient (Cin, N, 4, 4) of nn.ConvTranspose2d(4, 2, 1): x (B, H, W, Cin), dy (B, 2H, 2W, N), both NHWC."""
    xn, dn = x.double().permute(0, 3, 1, 2).contiguous(), dy.double().permute(0, 3, 1, 2).contiguous()
    w = torch.zeros(x.shape[3], dy.shape[3], 4, 4, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv_transpose2d(xn, w, stride=2, padding=1).backward(dn)
    return w.grad


def convt_bounds(x, dy):
    """The two bounds for the transposed convolution's weight gradient: T = B * H * W input positions per weight element."""
    T = x.shape[0] * x.shape[1] * x.shape[2]
    return bounds_of(T, convt_weight(rounded(x).abs(), rounded(dy).abs()), convt_weight(x.abs(), dy.abs()))


# The kernel matrix of tests/test_gpu_wgrad_bf16.py, held by the emulation too (tests/test_wgrad_bf16_cpu.py):
# ((B, H, W, C0, C1, N), (k, stride, pad), (cin, nout) of the unpadded layer or None)
BIG = ((1, 128, 128, 128, 0, 128), (3, 1, 1), None)          # 256 chunks: many slabs
MATRIX = [
    ((1, 3, 5, 64, 0, 64), (3, 1, 1), None),                 # 15 positions: less than one chunk
    ((3, 9, 7, 64, 0, 64), (3, 1, 1), None),                 # odd sizes, chunks straddle images
    ((2, 16, 32, 64, 0, 128), (3, 1, 1), None),              # two column blocks
    ((1, 32, 32, 64, 0, 192), (3, 1, 1), None),              # N is not a multiple of 128: 64-column tiles
    ((1, 16, 16, 128, 256, 256), (3, 1, 1), None),           # two inputs
    ((1, 8, 8, 32, 96, 64), (3, 1, 1), None),                # two inputs, 32-granular
    ((1, 16, 16, 64, 0, 64), (3, 1, 1), (60, 61)),           # padded channels dropped
    ((2, 9, 9, 64, 0, 64), (3, 2, 1), None),                 # stride 2
    ((1, 16, 16, 64, 0, 128), (4, 2, 1), None),              # the discriminator's layers
    ((2, 8, 8, 96, 0, 64), (1, 1, 0), None),                 # single tap
    BIG,
]
KINDS = ["randn", "dc10", "dc100", "post_relu", "chan_scales", "dy_1e-3", "student_t_dy"]
KINDS_SHAPE = ((2, 32, 32, 128, 0, 128), (3, 1, 1), None)


def out_hw(H, W, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def operands(kind, sx, sy, seed):
    """Seeded fp32 operands of one kind (the seven kinds of tests/test_gpu_wgrad_winograd.py), all within fp32's normal range."""
    g = torch.Generator().manual_seed(seed)
    x, dy = torch.randn(sx, generator=g), torch.randn(sy, generator=g)
    if kind == "dc10":
        x = x + 10.0
    elif kind == "dc100":
        x = x + 100.0
    elif kind == "post_relu":
        x = x.relu()
    elif kind == "chan_scales":
        x = x * torch.logspace(-2, 2, sx[3]).view(1, 1, 1, -1)
    elif kind == "dy_1e-3":
        dy = dy * 1e-3
    elif kind == "student_t_dy":
        chi2 = sum(torch.randn(sy, generator=g).pow(2) for _ in range(3))          # Student-t, 3 degrees of freedom: z / sqrt(chi2_3 / 3)
        dy = dy / torch.sqrt(chi2 / 3.0)
    else:
        assert kind == "randn", kind
    return x.contiguous(), dy.contiguous()


def case(shape, geom, drop=None, kind="randn"):
    """-> (x, dy, cin, nout): the operands of a matrix case; the channels beyond cin / nout carry data that the launch must drop."""
    B, H, W, C0, C1, N = shape
    k, stride, pad = geom
    OH, OW = out_hw(H, W, k, stride, pad)
    x, dy = operands(kind, (B, H, W, C0 + C1), (B, OH, OW, N), 900 + H + C0 + C1 + N + 7 * k + stride)
    cin, nout = drop or (C0 + C1, N)
    return x, dy, cin, nout
