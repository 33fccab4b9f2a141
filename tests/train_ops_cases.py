"""Seeded cases, references and error bounds for the loss / optimizer kernels of the training step (csrc/train_ops.hip): the fused Adam update,
the activation backward, the per-channel PReLU, MaxPool2d(2, 2), the device-side head crop and the panel pack / unpack.
CPU only (torch and numpy): tests/test_train_ops_primitives_cpu.py checks this module itself - every bound against a numpy-float32 restatement of
the kernel's arithmetic, and against planted errors - and tests/test_gpu_train_ops_primitives.py feeds the same cases to the HIP library.

Every bound is a count of fp32 roundings (u = 2^-24 per rounding), never a figure measured on the kernels:
  Adam   m: two products and a sum (or one product and a fused multiply-add) -> 2^-22 A, A = |b1 m| + |(1 - b1) g|
         v: the same with one more product, every term positive            -> 2^-22 v64
         p: one rounding of the result + nine in the update (step, isq, m, sqrt v, the two products, the sum, the division, the product with
            step) -> 2^-23 |p64| + r_t step A / den with r_t = 2^-20 + 2^-23 b1^t / (1 - b1^t) + 2^-23 b2^t / (1 - b2^t): the last two are 2 ulp
            of powf, amplified by the subtraction from 1
  tanh / sigmoid backward: at most three roundings                          -> 2^-22 |dy|
  PReLU + residual: two roundings, or one fused                             -> 2^-23 (|PReLU(x)| + |res|)
Everything else is an index map or a selection and is compared for equality."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import emu_ops

ACT_NONE, ACT_RELU, ACT_TANH, ACT_SIGMOID, ACT_LRELU = 0, 1, 2, 3, 4      # include/lwg_hip.h (ipercore_amd._lib carries the same values)


def _rng(*seed):
    return np.random.default_rng([20261020] + [int(s) for s in seed])


def _randn(shape, *seed):
    return torch.from_numpy(_rng(*seed).standard_normal(shape, dtype=np.float32))


def worst_ratio(err, bound):
    """max |error| / bound as a float; an exact element counts as 0 whatever its bound (0 / 0 where dy = 0), an error where the bound is 0 as inf."""
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())


def bits(t):
    """fp32 tensor -> its bit patterns (-0.0 and +0.0 differ)."""
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------------------------------ Adam
ADAM_SIZES = (4, 1000, 1028, 8388612)        # 8 388 612 = 2 097 153 float4s = 8192 * 256 + 1: the grid-stride loop wraps once, one-element tail
ADAM_LR, ADAM_BETAS, ADAM_EPS = 1e-2, (0.9, 0.999), 1e-8        # the trainer's
ADAM_FIRST_STEPS = 6                         # t_dev = 0, stepped six times
ADAM_PRESETS = (999, 99999)                  # t_dev preset, then one step (t = 1000, t = 100 000)
ADAM_CPU_TS = (1, 2, 3, 10, 100, 1000, 100000)


def adam_abi(x):
    """A hyperparameter as the C ABI receives it (a float argument)."""
    return float(np.float32(x))


def adam_inputs(n, fresh, *seed):
    """p ~ N(0,1); g = N(0,1) 10^k with k uniform in {-6..1} per element and min(8, n / 2) elements exactly 0 (the last one among them);
    m = v = 0 when ``fresh`` (before the first step), else m ~ 0.1 N(0,1), v ~ 0.01 U(0,1)."""
    r = _rng(1, n, *seed)
    p = torch.from_numpy(r.standard_normal(n, dtype=np.float32))
    k = torch.from_numpy(r.integers(-6, 2, size=n).astype(np.float32))
    g = torch.from_numpy(r.standard_normal(n, dtype=np.float32)) * torch.pow(torch.tensor(10.0), k)
    zeros = np.concatenate([r.choice(n - 1, size=min(8, n // 2) - 1, replace=False), [n - 1]])
    g[torch.from_numpy(zeros)] = 0.0
    if fresh:
        m, v = torch.zeros(n), torch.zeros(n)
    else:
        m = 0.1 * torch.from_numpy(r.standard_normal(n, dtype=np.float32))
        v = 0.01 * torch.from_numpy(r.random(n, dtype=np.float32))
    return p, g, m, v


def adam_step_gradient(g, step):
    """The gradient of step ``step`` of a multi-step run: the same values at other elements (a rotation by a prime), so every element sees all scales."""
    return g if step == 0 else torch.roll(g, 4099 * step % g.numel()).contiguous()


def adam_ref64(p, g, m, v, t, lr=ADAM_LR, betas=ADAM_BETAS, eps=ADAM_EPS, abi=True):
    """One float64 Adam step (the formula of lwg_adam_kernel's header comment) from fp32 state, hyperparameters as the ABI rounds them
    (abi = False: the Python values as they are).  -> dict with m, v, p (float64) and the three bounds."""
    lr, b1, b2, eps = (adam_abi(lr), adam_abi(betas[0]), adam_abi(betas[1]), adam_abi(eps)) if abi else (lr, betas[0], betas[1], eps)
    p, g, m, v = (a.double() for a in (p, g, m, v))
    A = (b1 * m).abs() + ((1 - b1) * g).abs()
    m64 = b1 * m + (1 - b1) * g
    v64 = b2 * v + (1 - b2) * g * g
    step = lr / (1 - b1 ** t)
    den = (v64 / (1 - b2 ** t)).sqrt() + eps
    p64 = p - step * m64 / den
    r_t = 2.0 ** -20 + 2.0 ** -23 * b1 ** t / (1 - b1 ** t) + 2.0 ** -23 * b2 ** t / (1 - b2 ** t)
    return {"m": m64, "v": v64, "p": p64, "m_bound": 2.0 ** -22 * A, "v_bound": 2.0 ** -22 * v64,
            "p_bound": 2.0 ** -23 * p64.abs() + r_t * step * A / den}


def adam_ratios(p, m, v, ref):
    """Worst |error| / bound of an Adam step's three outputs (an error where the bound is 0 counts as inf; 0 / 0 as 0)."""
    out = {}
    for name, got in (("m", m), ("v", v), ("p", p)):
        err, bound = (got.double() - ref[name]).abs(), ref[name + "_bound"]
        out[name] = worst_ratio(err, bound)
    return out


def adam_f32(p, g, m, v, t, lr=ADAM_LR, betas=ADAM_BETAS, eps=ADAM_EPS):
    """lwg_adam_kernel restated operation by operation in numpy float32 (no contraction) -> p, m, v."""
    f = np.float32
    p, g, m, v = (a.numpy().astype(f) for a in (p, g, m, v))
    lr, b1, b2, eps, one = f(lr), f(betas[0]), f(betas[1]), f(eps), f(1)
    bc1, bc2 = one - np.power(b1, f(t), dtype=f), one - np.power(b2, f(t), dtype=f)
    step, isq = lr / bc1, one / np.sqrt(bc2)
    mm = b1 * m + (one - b1) * g
    vv = b2 * v + (one - b2) * g * g
    pp = p - step * mm / (np.sqrt(vv) * isq + eps)
    assert pp.dtype == f and mm.dtype == f and vv.dtype == f
    return torch.from_numpy(pp), torch.from_numpy(mm), torch.from_numpy(vv)


# --------------------------------------------------------------------------------------------------------------------- activation backward
ACT_SIZES = (4, 1028, 8388612)
ACT_CODES = {"none": ACT_NONE, "relu": ACT_RELU, "lrelu": ACT_LRELU, "tanh": ACT_TANH, "sigmoid": ACT_SIGMOID}
ACT_PLANTED = {ACT_NONE: (0.0, -0.0), ACT_RELU: (0.0, -0.0), ACT_LRELU: (0.0, -0.0), ACT_TANH: (0.0, -0.0, 1.0, -1.0), ACT_SIGMOID: (0.0, -0.0, 1.0)}


def act_inputs(n, act):
    """dy ~ N(0,1); y ~ N(0,1) mapped through tanh / sigmoid for those codes, with min(16, n / number of values) elements planted at each value of
    ACT_PLANTED[act] (the kinks and the saturated outputs); the last element is always a planted one (it lies in the kernel's tail)."""
    dy, y = _randn(n, 2, n, act), _randn(n, 3, n, act)
    if act == ACT_TANH:
        y = torch.tanh(y)
    elif act == ACT_SIGMOID:
        y = torch.sigmoid(y)
    vals = ACT_PLANTED[act]
    per = min(16, n // len(vals))
    pos = _rng(4, n, act).choice(n - 1, size=per * len(vals) - 1, replace=False).tolist() + [n - 1]
    for j, q in enumerate(pos):
        y[q] = vals[j % len(vals)]
    return dy, y


def act_bwd_f32(dy, y, act):
    """The fp32 expressions that NONE / RELU / LRELU must equal bit for bit (a masked-out negative dy gives -0.0 in the kernel and here)."""
    if act == ACT_NONE:
        return dy.clone()
    if act == ACT_RELU:
        return dy * (y > 0).float()
    assert act == ACT_LRELU
    return dy * torch.where(y > 0, torch.tensor(1.0), torch.tensor(np.float32(0.2)))


def act_bwd_ref64(dy, y, act):
    """float64 dy (1 - y^2) / dy y (1 - y) and the bound 2^-22 |dy|."""
    d, yy = dy.double(), y.double()
    ref = d * (1 - yy * yy) if act == ACT_TANH else d * yy * (1 - yy)
    return ref, 2.0 ** -22 * d.abs()


def act_bwd_kernel_f32(dy, y, act):
    """lwg_dact_from_y restated in numpy float32, no contraction."""
    f = np.float32
    d, v = dy.numpy(), y.numpy()
    if act == ACT_RELU:
        k = np.where(v > 0, f(1), f(0))
    elif act == ACT_LRELU:
        k = np.where(v > 0, f(1), f(0.2))
    elif act == ACT_TANH:
        k = f(1) - v * v
    elif act == ACT_SIGMOID:
        k = v * (f(1) - v)
    else:
        k = np.ones_like(v)
    out = d * k.astype(f)
    assert out.dtype == f
    return torch.from_numpy(out)


# ----------------------------------------------------------------------------------------------------------------------------------- PReLU
# (700 000, 12): 2 100 000 float4s with C / 4 = 3 and 8192 * 256 = 2 097 152 = 1 (mod 3): a channel taken from anything but the global index fails
PRELU_CASES = ((1, 4), (7, 12), (5, 260), (33, 64), (700000, 12))
PRELU_SLOPES = (0.25, 0.0, -0.5, 1.0, 1.75)


def prelu_inputs(rows, C):
    """x, res, dy ~ N(0,1) (rows, C); slope (C): even channels cycle through PRELU_SLOPES, odd channels ~ N(0,1); +0.0 and -0.0 planted in every
    channel (rows >= 2: two rows per channel, else alternating channels)."""
    x, res, dy = (_randn((rows, C), 5 + j, rows, C) for j in range(3))
    slope = _randn(C, 8, rows, C)
    slope[0::2] = torch.tensor(PRELU_SLOPES)[torch.arange((C + 1) // 2) % len(PRELU_SLOPES)]
    r = _rng(9, rows, C)
    for c in range(C):
        if rows >= 2:
            r0, r1 = r.choice(rows, size=2, replace=False)
            x[r0, c], x[r1, c] = 0.0, -0.0
        else:
            x[0, c] = 0.0 if c % 2 == 0 else -0.0
    return x, slope, res, dy


def prelu_f32(x, slope):
    return torch.where(x > 0, x, slope * x)


def prelu_bwd_f32(x, slope, dy):
    """ATen's rule: at x = +-0 the gradient is slope * dy."""
    return torch.where(x > 0, dy, slope * dy)


def prelu_bwd_f32_ge(x, slope, dy):
    """The planted error (and the kernel's rule before it followed ATen): x >= 0 keeps dy."""
    return torch.where(x >= 0, dy, slope * dy)


def prelu_res_ref64(x, slope, res):
    a = torch.where(x > 0, x.double(), slope.double() * x.double())
    return a + res.double(), 2.0 ** -23 * (a.abs() + res.double().abs())


# --------------------------------------------------------------------------------------------------------------------------------- MaxPool
# (1, 2050, 4100, 8): 4 202 500 output float4s > 16384 * 256: the grid-stride loop wraps
POOL_CASES = ((1, 2, 2, 4), (2, 6, 10, 4), (3, 4, 14, 12), (1, 10, 6, 260), (1, 2050, 4100, 8))
POOL_SPECIAL = ("signed_zero", "neg_inf")


def pool_inputs(B, H, W, C, kind="ties"):
    """x (B,H,W,C) NHWC and dy ~ N(0,1) (B,H/2,W/2,C).  "ties": integers from {-1, 0, 0, 1} (most windows tie in every arrangement);
    "signed_zero": +0.0 / -0.0 only; "neg_inf": {-inf, -inf, -inf, 0, 1} (about a tenth of the windows are entirely -inf)."""
    table = {"ties": (-1.0, 0.0, 0.0, 1.0), "signed_zero": (0.0, -0.0), "neg_inf": (-math.inf, -math.inf, -math.inf, 0.0, 1.0)}[kind]
    gen = torch.Generator().manual_seed(1000003 * H + 1009 * W + C + len(table))
    idx = torch.randint(0, len(table), (B, H, W, C), dtype=torch.uint8, generator=gen)
    x = torch.empty(B, H, W, C)
    for j, val in enumerate(table):
        x.masked_fill_(idx == j, val)
    dy = torch.randn(B, H // 2, W // 2, C, generator=gen)
    return x, dy


def pool_reference(x, dy):
    """F.max_pool2d and its autograd on the CPU (NHWC in and out)."""
    xr = x.detach().clone().requires_grad_(True)
    y = F.max_pool2d(xr.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    dx, = torch.autograd.grad(y, xr, dy)
    return y.detach().contiguous(), dx.contiguous()


def pool_kernel_np(x, dy, row_stride_on="W"):
    """lwg_maxpool2_fwd_kernel / _bwd_kernel restated on flat arrays with the kernels' own index arithmetic -> y, dx.
    row_stride_on = "H" plants the error of a row stride built on OH instead of OW."""
    B, H, W, C = x.shape
    OH, OW, C4 = H // 2, W // 2, C // 4
    xf, dyf = x.numpy().reshape(-1, 4), dy.numpy().reshape(-1, 4)            # float4s
    i = np.arange(B * OH * OW * C4, dtype=np.int64)
    c, p = i % C4, i // C4
    ox, q = p % OW, p // OW
    oy, b = q % OH, q // OH
    base = ((b * 2 * OH + 2 * oy) * 2 * OW + 2 * ox) * C4 + c
    rs = 2 * (OW if row_stride_on == "W" else OH) * C4
    off = (0, C4, rs, rs + C4)
    v = np.stack([xf[base + o] for o in off])                               # (4 taps, n, 4 lanes)
    best, m = np.zeros(v.shape[1:], dtype=np.int64), v[0].copy()
    for t in range(1, 4):
        up = v[t] > m
        m, best = np.where(up, v[t], m), np.where(up, t, best)
    y = m                                                                   # the first maximum's own bits (of tied -0 / +0 the first)
    dx = np.full_like(xf, np.nan)
    for t in range(4):
        dx[base + off[t]] = np.where(best == t, dyf, np.float32(0))
    return torch.from_numpy(y.reshape(B, OH, OW, C)), torch.from_numpy(dx.reshape(B, H, W, C))


# ------------------------------------------------------------------------------------------------------------------------------- head crop
CROP_IMAGE = (14, 2, 37, 53)                                 # N, C, H, W: H != W, and N, C > 1 are grid dimensions
CROP_OUT = ((112, 96), (7, 5), (17, 31), (1, 1), (1, 9), (6, 1))      # (17, 31) = 527 pixels: two blocks and a 15-thread tail; OH / OW = 1: the s = 0 branches
CROP_OUT_BWD = ((112, 96), (7, 5), (17, 31))
CROP_BOXES = ((0, 53, 0, 37), (52, 53, 36, 37), (10, 11, 0, 37), (40, 90, 30, 70), (5, 5, 0, 10), (7, 20, 9, 9), (53, 57, 0, 5), (-3, 10, 0, 10),
              (20, 10, 0, 10), (0, 2 ** 40, 0, 2 ** 40), (2 ** 40, 2 ** 40 + 5, 0, 5), (3, 6, 2, 5), (0, 53, 35, 37), (52, 60, 36, 99))      # min_x, max_x, min_y, max_y
CROP_VALID = (1, 1, 1, 1, 0, 0, 0, 0, 0, 1, 0, 1, 1, 1)
CROP_FWD_TOL = 2e-6                                          # absolute, gpu_checks.check_face_loss's for images of this scale
CROP_BWD_TOL = 2e-5                                          # * max(1, max |dx_ref| of the sample): check_face_loss's rule, per sample


def crop_inputs():
    N, C, H, W = CROP_IMAGE
    assert len(CROP_BOXES) == N
    return 0.5 * _randn((N, C, H, W), 10), torch.tensor(CROP_BOXES, dtype=torch.int64)


def crop_dy(out_hw):
    N, C, _, _ = CROP_IMAGE
    return _randn((N, C) + tuple(out_hw), 11, *out_hw)


def crop_rect(box, H, W):
    """The clamped rectangle (x0, y0, cw, ch) of a kept box, None for a dropped one: lwg_crop_geom."""
    bx0, bx1, by0, by1 = (int(b) for b in box)
    if bx0 == bx1 or by0 == by1 or bx0 < 0 or by0 < 0:
        return None
    bx1, by1 = min(bx1, W), min(by1, H)
    if bx1 <= bx0 or by1 <= by0:
        return None
    return bx0, by0, bx1 - bx0, by1 - by0


def crop_bwd_ref(dy, box, in_hw, dtype=torch.float32):
    """emu_ops.crop_resize_bwd (autograd through the slice + F.interpolate) in ``dtype``."""
    x = torch.zeros(dy.shape[0], dy.shape[1], *in_hw, dtype=dtype, requires_grad=True)
    y, _ = emu_ops._crop_ref(x, box, dy.shape[2:])
    (y * dy.to(dtype)).sum().backward()
    return x.grad.detach()


def crop_bwd_tol(dx_ref):
    """Per-sample tolerance (N, 1, 1, 1)."""
    return CROP_BWD_TOL * dx_ref.abs().amax(dim=(1, 2, 3), keepdim=True).clamp_min(1.0)


def _crop_taps(rect, OH, OW, npix):
    f = np.float32
    x0, y0, cw, ch = rect
    sx = f(cw - 1) / f(OW - 1) if OW > 1 else f(0)
    sy = f(ch - 1) / f(OH - 1) if OH > 1 else f(0)
    p = np.arange(npix)
    oy, ox = p // OW, p % OW
    fy, fx = sy * oy.astype(f), sx * ox.astype(f)
    iy0, ix0 = fy.astype(np.int64), fx.astype(np.int64)
    iy1, ix1 = iy0 + (iy0 < ch - 1), ix0 + (ix0 < cw - 1)
    ly1, lx1 = fy - iy0.astype(f), fx - ix0.astype(f)
    ly0, lx0 = f(1) - ly1, f(1) - lx1
    assert ly0.dtype == f and fx.dtype == f
    return p, y0 + iy0, y0 + iy1, x0 + ix0, x0 + ix1, ly0, ly1, lx0, lx1


def crop_kernel_np(x, box, out_hw, blocks=None):
    """lwg_crop_resize_kernel restated in numpy float32, no contraction -> (y, valid); y starts as NaN, as the GPU test's buffer does.
    ``blocks``: 256-pixel blocks launched per (sample, channel) - default the kernel's (OH OW + 255) / 256; one fewer plants a dropped tail block."""
    N, C, H, W = x.shape
    OH, OW = out_hw
    blocks = (OH * OW + 255) // 256 if blocks is None else blocks
    npix = min(blocks * 256, OH * OW)
    xs = x.numpy()
    y = np.full((N, C, OH * OW), np.nan, dtype=np.float32)
    valid = np.zeros(N, dtype=np.float32)
    for i in range(N):
        rect = crop_rect(box[i].tolist(), H, W)
        valid[i] = 0.0 if rect is None else 1.0
        if rect is None:
            y[i, :, :npix] = 0.0
            continue
        p, ya, yb, xa, xb, ly0, ly1, lx0, lx1 = _crop_taps(rect, OH, OW, npix)
        s = xs[i]
        y[i][:, p] = ly0 * (lx0 * s[:, ya, xa] + lx1 * s[:, ya, xb]) + ly1 * (lx0 * s[:, yb, xa] + lx1 * s[:, yb, xb])
    return torch.from_numpy(y.reshape(N, C, OH, OW)), torch.from_numpy(valid)


def crop_bwd_kernel_np(dy, box, in_hw):
    """lwg_crop_resize_bwd_kernel restated in numpy float32 (the atomic adds in pixel order)."""
    N, C, OH, OW = dy.shape
    H, W = in_hw
    d = dy.numpy().reshape(N, C, OH * OW)
    dx = np.zeros((N, C, H, W), dtype=np.float32)
    for i in range(N):
        rect = crop_rect(box[i].tolist(), H, W)
        if rect is None:
            continue
        p, ya, yb, xa, xb, ly0, ly1, lx0, lx1 = _crop_taps(rect, OH, OW, OH * OW)
        for c in range(C):
            for yy, xx, wgt in ((ya, xa, ly0 * lx0), (ya, xb, ly0 * lx1), (yb, xa, ly1 * lx0), (yb, xb, ly1 * lx1)):
                np.add.at(dx[i, c], (yy, xx), wgt * d[i, c])
    return torch.from_numpy(dx)


# ------------------------------------------------------------------------------------------------------------------ panel pack and unpack
# (weight shape, transposed, kidx, cin, cin_pad, nout, n_pad).  The first seven: the requests of gpu_checks.check_panel_cache_refresh (what
# packing.pack_conv / pack_dgrad_conv / pack_conv_transpose ask for); then 49 * 4 = 196 -> 224 rows in the unchunked K order, cin = 40 of
# cin_pad = 64 transposed, and a single tap with padded columns
PANEL_CASES = (((64, 6, 7, 7), False, tuple(range(49)), 6, 8, 64, 64),
               ((128, 64, 3, 3), False, tuple(range(9)), 64, 64, 128, 128),
               ((128, 64, 3, 3), True, tuple(reversed(range(9))), 128, 128, 64, 64),
               ((64, 128, 3, 3), False, tuple(range(9)), 128, 128, 64, 64),
               ((128, 64, 4, 4), True, (5, 7, 13, 15), 128, 128, 64, 64),
               ((128, 64, 4, 4), True, (0, 2, 8, 10), 128, 128, 64, 64),
               ((40, 64, 3, 3), False, tuple(range(9)), 64, 64, 40, 64),
               ((64, 4, 7, 7), False, tuple(range(49)), 4, 4, 64, 64),
               ((40, 64, 3, 3), True, tuple(reversed(range(9))), 40, 64, 64, 64),
               ((24, 8, 3, 3), False, (4,), 8, 8, 24, 32))
PARITY_TAPS = ((5, 7, 13, 15), (4, 6, 12, 14), (1, 3, 9, 11), (0, 2, 8, 10))     # the four sub-kernels of a 4x4 / stride 2 transposed convolution
# (dw shape, transposed, tap sets written one after another, cin, cin_pad, nout, n_pad): dw larger than (cin, nout) in both dimensions, so rows and
# columns that no tap maps to exist next to the ones that are written
UNPACK_CASES = (((48, 32, 4, 4), True, PARITY_TAPS, 40, 64, 24, 32),
                ((72, 8, 7, 7), False, (tuple(range(49)),), 6, 8, 64, 64),
                ((40, 70, 3, 3), False, ((8, 6, 4, 2, 0),), 64, 64, 40, 64))
SENTINEL = -7.5


def panel_id(case):
    sh, tr, kidx, cin, cin_pad, nout, n_pad = case[:7]
    return "w{}_{}_t{}_c{}of{}_n{}of{}".format("x".join(map(str, sh)), "T" if tr else "N", len(kidx), cin, cin_pad, nout, n_pad)


def index_weight(shape):
    """A weight that holds its own flat index (exact in fp32: all < 2^24)."""
    n = int(np.prod(shape))
    assert n < 2 ** 24
    return torch.arange(n, dtype=torch.float32).view(*shape)


def pack_kernel_np(w, transposed, kidx, cin, cin_pad, nout, n_pad, chunked_form=False):
    """lwg_pack_panel_kernel restated with its own index arithmetic (k -> tap, c by lwg_korder_decode); chunked_form = True: the chunked branch of
    lwg_pack_panels_kernel (a thread per output column x four channels walking the taps; cin_pad % 32 == 0 only).  The output starts as NaN."""
    D0, D1, KH, KW = w.shape
    KHW, ntaps = KH * KW, len(kidx)
    Kp = (ntaps * cin_pad + 31) // 32 * 32
    wf, kx = w.numpy().reshape(-1), np.asarray(kidx)
    out = np.full(((Kp // 4) * n_pad, 4), np.nan, dtype=np.float32)
    if chunked_form:
        assert cin_pad % 32 == 0
        i = np.arange((cin_pad // 4) * n_pad)
        cq, n = i // n_pad, i % n_pad
        c0 = cq * 4
        ob = ((c0 >> 5) * ntaps * 8 + ((c0 & 31) >> 2)) * n_pad + n
        for tap in range(ntaps):
            for kk in range(4):
                c = c0 + kk
                ok = (n < nout) & (c < cin)
                cs, ns = np.where(ok, c, 0), np.where(ok, n, 0)
                src = ((cs if transposed else ns) * D1 + (ns if transposed else cs)) * KHW + kx[tap]
                out[ob + tap * 8 * n_pad, kk] = np.where(ok, wf[src], np.float32(0))
        return torch.from_numpy(out.reshape(Kp // 4, n_pad, 4))
    i = np.arange((Kp // 4) * n_pad)
    k4, n = i // n_pad, i % n_pad
    for kk in range(4):
        k = k4 * 4 + kk
        if cin_pad % 32 == 0:
            chunk = k // (ntaps * 32)
            rem = k - chunk * ntaps * 32
            tap, c = rem >> 5, chunk * 32 + (rem & 31)
        else:
            tap = k // cin_pad
            c = k - tap * cin_pad
        ok = (k < ntaps * cin_pad) & (n < nout) & (c < cin)
        cs, ns, ts = np.where(ok, c, 0), np.where(ok, n, 0), np.where(ok, tap, 0)
        src = ((cs if transposed else ns) * D1 + (ns if transposed else cs)) * KHW + kx[ts]
        out[:, kk] = np.where(ok, wf[src], np.float32(0))
    return torch.from_numpy(out.reshape(Kp // 4, n_pad, 4))


def unpack_kernel_np(dwk, dw, transposed, kidx, cin, cin_pad, nout):
    """lwg_unpack_wgrad_kernel restated with its own index arithmetic, in place on dw."""
    D0, D1, KH, KW = dw.shape
    KHW, ntaps, n_pad = KH * KW, len(kidx), dwk.shape[1]
    i = np.arange(ntaps * cin * nout)
    n, r = i % nout, i // nout
    c, tap = r % cin, r // cin
    k = ((c >> 5) * ntaps + tap) * 32 + (c & 31) if cin_pad % 32 == 0 else tap * cin_pad + c
    dst = ((c if transposed else n) * D1 + (n if transposed else c)) * KHW + np.asarray(kidx)[tap]
    assert len(np.unique(dst)) == len(dst)
    dw.view(-1).numpy()[dst] = dwk.reshape(-1).numpy()[k * n_pad + n]
    return dw


def unpack_reference(case):
    """-> (dwk per tap set, dw after each tap set by emu_ops.unpack_wgrad starting from the SENTINEL-filled dw, the mask of positions ever written)."""
    sh, tr, tapsets, cin, cin_pad, nout, n_pad = case
    dw = torch.full(sh, SENTINEL)
    dwks, stages = [], []
    for j, kidx in enumerate(tapsets):
        rows = len(kidx) * cin_pad
        dwk = (torch.arange(rows * n_pad, dtype=torch.float32) + 1000.0 * j).view(rows, n_pad)
        emu_ops.unpack_wgrad(dwk, dw, tr, kidx, cin, cin_pad, nout)
        dwks.append(dwk)
        stages.append(dw.clone())
    written = torch.zeros(sh, dtype=torch.bool)
    flat = written.view(sh[0], sh[1], -1)
    for kidx in tapsets:
        flat[:cin if tr else nout, :nout if tr else cin][:, :, list(kidx)] = True
    return dwks, stages, written
