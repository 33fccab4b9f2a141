"""Seeded cases, float64 references, error bounds and planted faults for the output-head kernels: lwg_head_compose_kernel<2|4> and
lwg_head_q4_kernel<1,2|2,4> (csrc/head.hip), lwg_head_bf16_kernel (csrc/bf16_ops.hip), the head phase of lwg_up4_head_bf16_kernel
(csrc/up4_head_bf16.hip), lwg_thin_conv_kernel<5|7, 2|4>, the two layout kernels and lwg_frames_to_u8.  CPU only (numpy and torch):
tests/test_head_cases_cpu.py checks this module itself - every bound against a numpy-float32 restatement of each form's arithmetic in that form's
documented order, and against planted faults - and tests/test_gpu_head_kernels.py feeds the same cases to the HIP library.

Why "exact" inputs.  With x ~ N(0, 1), w ~ 0.03 N(0, 1) and C = 64 the rigorous fp32 bound gamma(25 C) sum |x||w| on a pre-activation is about 2.7e-3,
and dropping one tap of one channel moves the median output by only 2.7 times that: a toleranced comparison on random data cannot see an indexing
error.  The exact ("dyadic") family makes the pre-activation s exact in ANY summation order, fused or not, vector ALU or matrix pipe:
  x        integers in [-8, 8];
  weights  integers in [-8, 8] times 2^-k, k = 10 for C = 64 and smaller for smaller C (pre-activations keep a spread of order 1);
so every product and every partial sum is an integer multiple of 2^-k below 2^24 2^-k (asserted per case: 2^k sum |x||w| < 2^24), and both
operands are bf16-representable (asserted): the same x and w, rounded to nothing, feed every form.  For the fused up-sampling head the
intermediate ReLU(ConvTranspose2d) is rounded to bf16, so it is exact too: transposed-conv weights in {-1, 0, 1} with at most 4 non-zeros per
(output channel, output parity), x in {-2 .. 2}, an integer bias - the intermediate is an integer of magnitude <= 128 (asserted).
Variants: "unsat" (above), "sat" (weight scale 2^-4: |s| reaches tens to hundreds, the mask hits 0 and 1, expf overflows), "cancel" (the weights of
channel 2 i + 1 are minus those of channel 2 i and x repeats each even channel in the odd one: s = 0 everywhere although every partial sum is
not, so img = 0, mask = 0.5, pred = 0.5 bg), and the coded impulse: x zero but for one (pixel, channel) = 1 and weights that are a distinct code
per (output, ky, kx) (pass "tap", 100 values n 2^-6, |n| <= 100) or per (output, channel) (pass "chan", n 2^-7, |n| <= 256), so each output is
the transcendental of exactly one weight.

The bound, s exact (u = 2^-24; roundings are counted as tests/lbs_cases.py does: a library transcendental - tanhf, expf - 2 ulp = 4 u, division
2 u, every other operation u; second-order terms by a factor SECOND = 1 + 2^-10; FLOOR = 2^-126 absolute for flushed denormals and for expf
overflowing to inf, which makes the mask exactly 0 where the true value is below 2^-126):
  img   = tanhf(s)                 E_img  = 4 u |tanh s| + FLOOR
  e     = expf(-s)                 relative 4 u
  d     = 1 + e                    relative u;  de / d = 4 u e / (1 + e) = 4 u (1 - m)
  mask  = 1 / d                    relative 2 u: E_mask = m (3 u + 4 u (1 - m)) SECOND + FLOOR
  q     = 1 - mask                 E_q    = E_mask + u (1 - m)
  pred  = mask bg + q img          the two products and the add round once each on at most m |bg| + (1 - m) |img| (contracted into an fma, one
                                   product does not round: the bound covers both):
                                   E_pred = (E_mask |bg| + E_q |img| + (1 - m) E_img + 2 u (m |bg| + (1 - m) |img|)) SECOND + FLOOR
Nothing here is a figure measured on the kernels.  The thin conv has no transcendental: on the exact family its outputs equal float64 bit for bit.

The random-data family (x ~ N(0, 1), w at scales 0.03 and 0.3, C = 64) is for magnitude and conditioning, not indexing: reference = float64
from the same (bf16-rounded where the form takes bf16) operands; the pre-activation carries E_s = gamma(25 C + 8) sum |x||w| (25 C multiply-adds
in any order, up to 8 more adds for per-tap partial sums), which reaches img with Lipschitz constant 1, the mask with 1/4 (and pred through both),
on top of the exact-family terms.  The fused up-sampling head keeps the 2e-2 of gpu_checks.check_bf16_up4_head on this family: an fp32 sum of the
transposed convolution that rounds to the other bf16 neighbour moves a pre-activation by 2^-9 of it, which no rounding count of the head covers."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
SECOND = 1.0 + 2.0 ** -10
FLOOR = 2.0 ** -126
SIZES = (1, 2, 3, 5, 15, 16, 17, 27, 28, 29, 31, 32, 33, 63, 64, 65)      # each side of the 16 / 32 / 64-pixel tile edges and of the 4 x 28 bf16 tile
CHANNELS = {"f32": (8, 24, 64), "q4": (4, 12, 64), "bf16": (64,), "thin": (8, 24, 64)}
FORMS = ("f32", "q4", "bf16")
VARIANTS = ("unsat", "sat", "cancel")
THIN = ((5, 3), (5, 4), (7, 3), (7, 4))                                    # (ks, N)
LARGE_S = (33, 65)
PROPERTY_S = (5, 29, 33)                                                   # inside the halo, one bf16 tile column + 1, one 32-pixel tile + 1
UP4_HW = ((1, 1), (1, 7), (6, 14), (7, 15), (5, 23), (23, 5))             # input (H, W): output 2H x 2W against the 12 x 28 tile
UP4_MANY = (5, 96, 96)                                                     # (B, H, W): 5 * 16 * 7 = 560 tiles, more than the CUs of the device
UP4_RANDOM_TOL = 2e-2
IMPULSE_S = {"f32": (29, 33, 65), "q4": (29, 33, 65), "bf16": (29, 33, 65)}
IMPULSE_CH = (0, 3, 4, 7, 8, 31, 32)


def gamma(k):
    return k * U / (1.0 - k * U)


def _rng(*seed):
    return np.random.default_rng([20261021, 7] + [int(s) for s in seed])


def worst_ratio(err, bound):
    """max |error| / bound; an exact element counts as 0 whatever its bound, a NaN as inf."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


def bits(t):
    return t.contiguous().view(torch.int32)


def bf16_exact(t):
    t = torch.as_tensor(t, dtype=torch.float32)
    return bool(torch.equal(t.to(torch.bfloat16).float(), t))


# ------------------------------------------------------------------------------------------------------------------------------ which form runs
def head_form(kind, B, S):
    """The tile form the entry point takes (the rules of lwg_head_compose_f32 / lwg_thin_conv_f32 / lwg_head_compose_q4_f32) and its (rows, columns)."""
    if kind in ("f32", "thin"):
        t = (S + 31) // 32
        return ("J4", (32, 32)) if t * t * B >= 512 else ("J2", (16, 32))
    if kind == "q4":
        big = ((S + 63) // 64) * ((S + 31) // 32) * B
        return ("NX2_RY4", (32, 64)) if big >= 512 else ("NX1_RY2", (16, 32))
    if kind == "bf16":
        return "NCB2", (4, 28)
    if kind == "up4":
        return "up4", (12, 28)
    raise ValueError(kind)


def large_form_batch(kind, S):
    """The smallest batch at which the entry point takes the large-tile form at size S."""
    B = 1
    while head_form(kind, B, S)[0] in ("J2", "NX1_RY2"):
        B += 1
    return B


def batch_of(S):
    """The batch (1, 2 or 3 in turn) of the exact family's cases at size S."""
    return 1 + SIZES.index(S) % 3


def weight_shift(C):
    """k of the exact family's weight scale 2^-k: 10 at C = 64, half a bit less per halving of C (the spread of a sum of 25 C terms goes as sqrt C)."""
    return 10 - int(round(0.5 * np.log2(64.0 / C)))


# ------------------------------------------------------------------------------------------------------------------------------ cases
def _bg(rng, B, S_h, S_w, per_frame):
    return torch.tensor(rng.uniform(-1.0, 1.0, (B if per_frame else 1, 3, S_h, S_w)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def exact_case(variant, B, S, C, per_frame_bg=True, ks=5, N=4):
    """x (B, S, S, C), w (N, C, ks, ks) (outputs 0..2 = the image regressor, 3 = the attention regressor), bg (B | 1, 3, S, S), k."""
    rng = _rng(VARIANTS.index(variant), B, S, C, ks, N)
    x = rng.integers(-8, 9, (B, S, S, C)).astype(np.float32)
    wi = rng.integers(-8, 9, (N, C, ks, ks)).astype(np.float32)
    k = 4 if variant == "sat" else weight_shift(C)
    if variant == "cancel":
        x[..., 1::2] = x[..., 0::2]
        wi[:, 1::2] = -wi[:, 0::2]
    case = {"x": torch.tensor(x), "w": torch.tensor(wi * 2.0 ** -k), "bg": _bg(rng, B, S, S, per_frame_bg), "k": k,
            "name": "%s_B%d_S%d_C%d_ks%d_N%d" % (variant, B, S, C, ks, N)}
    assert_exact(case)
    return case


def assert_exact(case):
    """The exactness conditions of the family: bf16-representable operands, integer multiples of 2^-k, and 2^k sum |x||w| < 2^24 at every output."""
    x, w, k = case["x"], case["w"], case["k"]
    assert bf16_exact(x) and bf16_exact(w), case["name"] + ": operands are not bf16-representable"
    wi = w.double() * 2.0 ** k
    assert bool((wi == wi.round()).all()) and bool((x == x.round()).all()), case["name"] + ": operands are not on the grid"
    mag = F.conv2d(x.double().abs().permute(0, 3, 1, 2), wi.abs(), padding=w.shape[-1] // 2)
    assert float(mag.max()) < 2.0 ** 24, case["name"] + ": 2^k sum |x||w| = %g" % float(mag.max())
    case["mag"] = float(mag.max())


def impulse_codes(pas, C):
    """(4, C, 5, 5) weights: pass "tap": a distinct bf16-exact code per (output, ky, kx), the same for every channel; "chan": per (output, channel)."""
    w = np.zeros((4, C, 5, 5), np.float32)
    if pas == "tap":
        n = (np.arange(100).reshape(4, 5, 5) + 1) * np.where(np.arange(100).reshape(4, 5, 5) % 2 == 0, 1.0, -1.0)
        w[:] = (n * 2.0 ** -6)[:, None]
    else:
        o, c = np.meshgrid(np.arange(4), np.arange(C), indexing="ij")
        w[:] = ((c * 4 + o + 1) * np.where(c % 2 == 0, 1.0, -1.0) * 2.0 ** -7)[:, :, None, None]
    return torch.tensor(w)


def seam_coords(n, edges):
    """0, 1, n - 2, n - 1 and both sides of every multiple of an edge inside [0, n)."""
    c = {0, 1, n - 2, n - 1}
    for e in edges:
        for m in (range(e, n, e) if e > 0 else range(-e, min(n, 17), -e)):        # a negative edge: its multiples up to 16 only
            c.update((m - 1, m))
    return sorted(v for v in c if 0 <= v < n)


def impulse_placements(S_h, S_w, C, edges_y, edges_x):
    """(y, x, channel) of one impulse per frame: corners, edges and both sides of every tile seam, channels 0, 3/4, 7/8, 31/32 and C - 1 in turn."""
    ys, xs = seam_coords(S_h, edges_y), seam_coords(S_w, edges_x)
    chans = [c for c in IMPULSE_CH if c < C - 1] + [C - 1]
    n = max(len(ys), len(xs))
    pos = [(ys[i % len(ys)], xs[i % len(xs)]) for i in range(n)]
    pos += [(ys[i % len(ys)], xs[(n - 1 - i) % len(xs)]) for i in range(n)]
    pos += [(0, 0), (0, S_w - 1), (S_h - 1, 0), (S_h - 1, S_w - 1)]
    pos = list(dict.fromkeys(pos))
    return [(y, x, chans[i % len(chans)]) for i, (y, x) in enumerate(pos)]


# (row edges, column edges) of each form's tiles; the bf16 head's tile is 4 rows: every fourth row up to 16, then every 16th
IMPULSE_EDGES = {"f32": ((16, 32), (32,)), "q4": ((16, 32), (32, 64)), "bf16": ((-4, 16), (28,)), "up4": ((12,), (28,))}


@functools.lru_cache(maxsize=None)
def impulse_case(kind, pas, S, C):
    """One frame per placement (a per-frame background): frame f is zero but for x[f, y, x, c] = 1."""
    place = impulse_placements(S, S, C, *IMPULSE_EDGES[kind])
    x = torch.zeros(len(place), S, S, C)
    for f, (py, px, c) in enumerate(place):
        x[f, py, px, c] = 1.0
    case = {"x": x, "w": impulse_codes(pas, C), "bg": _bg(_rng(99, S, C), len(place), S, S, True), "k": 7, "place": place,
            "name": "impulse_%s_%s_S%d_C%d" % (kind, pas, S, C)}
    assert_exact(case)
    return case


@functools.lru_cache(maxsize=None)
def random_case(scale, B, S, C=64, bf16=False):
    rng = _rng(5, int(scale * 100), B, S, C)
    x = torch.tensor(rng.standard_normal((B, S, S, C)).astype(np.float32))
    w = torch.tensor((rng.standard_normal((4, C, 5, 5)) * scale).astype(np.float32))
    if bf16:
        x, w = x.to(torch.bfloat16).float(), w.to(torch.bfloat16).float()
    return {"x": x, "w": w, "bg": _bg(rng, B, S, S, True), "name": "random_%g_B%d_S%d_C%d%s" % (scale, B, S, C, "_bf16" if bf16 else "")}


# ------------------------------------------------------------------------------------------------------------------------------ the fused up-sampling head
@functools.lru_cache(maxsize=None)
def up4_case(variant, B, H, W, per_frame_bg=True):
    """x (B, H, W, 128) in {-2 .. 2}; wup (128, 64, 4, 4) ConvTranspose2d(4, 2, 1) weights in {-1, 0, 1}, at most 4 non-zeros per (output channel,
    output parity); an integer bias; the head's weights as exact_case's.  "cancel": odd intermediate channels repeat the even ones."""
    rng = _rng(11, VARIANTS.index(variant), B, H, W)
    x = rng.integers(-2, 3, (B, H, W, 128)).astype(np.float32)
    wup = np.zeros((128, 64, 4, 4), np.float32)
    kpar = ((1, 3), (0, 2))                                  # kernel rows (columns) that reach even / odd output rows (columns): oy = 2 iy - 1 + ky
    for n in range(64):
        for py in range(2):
            for px in range(2):
                for _ in range(4):
                    wup[rng.integers(128), n, kpar[py][rng.integers(2)], kpar[px][rng.integers(2)]] = rng.choice((-1.0, 1.0))
    bias = rng.integers(-2, 5, (64,)).astype(np.float32)
    wh = rng.integers(-8, 9, (4, 64, 5, 5)).astype(np.float32)
    k = 4 if variant == "sat" else 10
    if variant == "cancel":
        wup[:, 1::2], bias[1::2], wh[:, 1::2] = wup[:, 0::2], bias[0::2], -wh[:, 0::2]
    case = {"x": torch.tensor(x), "wup": torch.tensor(wup), "bias": torch.tensor(bias), "w": torch.tensor(wh * 2.0 ** -k), "k": k,
            "bg": _bg(rng, B, 2 * H, 2 * W, per_frame_bg), "name": "up4_%s_B%d_%dx%d" % (variant, B, H, W)}
    assert_up4_exact(case)
    return case


def up4_intermediate64(case):
    """ReLU(ConvTranspose2d(4, 2, 1)(x) + bias) in float64, (B, 2H, 2W, 64)."""
    t = F.conv_transpose2d(case["x"].double().permute(0, 3, 1, 2), case["wup"].double(), case["bias"].double(), stride=2, padding=1)
    return t.relu().permute(0, 2, 3, 1).contiguous()


def assert_up4_exact(case):
    wup = case["wup"]
    assert bf16_exact(case["x"]) and bf16_exact(wup), case["name"]
    nz = torch.zeros(64, 2, 2)
    for ky in range(4):
        for kx in range(4):
            nz[:, (ky + 1) % 2, (kx + 1) % 2] += (wup[:, :, ky, kx] != 0).sum(0)
    assert float(nz.max()) <= 4, case["name"] + ": %d non-zeros in a parity" % int(nz.max())
    t = up4_intermediate64(case)
    assert bool((t == t.round()).all()) and float(t.abs().max()) <= 128, case["name"] + ": intermediate %g" % float(t.abs().max())
    case["t"] = t.float()
    assert_exact({"x": case["t"], "w": case["w"], "k": case["k"], "name": case["name"]})


UP4_IMPULSE_CH = (0, 3, 4, 7, 8, 31, 32, 63)


@functools.lru_cache(maxsize=None)
def up4_impulse_case(pas, H, W):
    """One frame per placement in the OUTPUT (2H x 2W).  Input channel j = 4 i + 2 (oy & 1) + (ox & 1) carries ONE transposed-conv weight = 1, to
    intermediate channel UP4_IMPULSE_CH[i] through kernel tap (1 + (oy & 1), 1 + (ox & 1)) (oy = 2 iy - 1 + ky): x[f, oy // 2, ox // 2, j] = 1 makes
    frame f's intermediate zero but for (oy, ox, that channel) = 1.  Zero bias."""
    place = impulse_placements(2 * H, 2 * W, 64, *IMPULSE_EDGES["up4"])
    x = torch.zeros(len(place), H, W, 128)
    wup = torch.zeros(128, 64, 4, 4)
    for i, c in enumerate(UP4_IMPULSE_CH):
        for par in range(4):
            wup[4 * i + par, c, 1 + (par >> 1), 1 + (par & 1)] = 1.0
    for f, (oy, ox, c) in enumerate(place):
        x[f, oy // 2, ox // 2, 4 * UP4_IMPULSE_CH.index(c) + 2 * (oy & 1) + (ox & 1)] = 1.0
    case = {"x": x, "wup": wup, "bias": torch.zeros(64), "w": impulse_codes(pas, 64), "k": 7, "place": place,
            "bg": _bg(_rng(98, H, W), len(place), 2 * H, 2 * W, True), "name": "up4_impulse_%s_%dx%d" % (pas, H, W)}
    assert_up4_exact(case)
    for f, (oy, ox, c) in enumerate(place):
        assert float(case["t"][f].sum()) == 1.0 and float(case["t"][f, oy, ox, c]) == 1.0, (case["name"], f)
    return case


@functools.lru_cache(maxsize=None)
def up4_random_case(scale, B, H, W):
    """The random-data family for the fused up-sampling head, operands already rounded to bf16 (the layer's weights and the head's at ``scale``)."""
    rng = _rng(13, int(scale * 100), B, H, W)
    r = lambda a: torch.tensor(a.astype(np.float32)).to(torch.bfloat16).float()
    return {"x": r(rng.standard_normal((B, H, W, 128))), "wup": r(rng.standard_normal((128, 64, 4, 4)) / np.sqrt(128 * 4)),
            "bias": torch.tensor((rng.standard_normal(64) * 0.1).astype(np.float32)), "w": r(rng.standard_normal((4, 64, 5, 5)) * scale),
            "bg": _bg(rng, B, 2 * H, 2 * W, True), "name": "up4_random_%g_B%d_%dx%d" % (scale, B, H, W)}


def up4_random_reference(case):
    """float64 from the bf16-rounded operands, the intermediate rounded to bf16 as the kernel stores it; every bound is UP4_RANDOM_TOL."""
    t = up4_intermediate64(case).to(torch.bfloat16).double()
    pred, m, img, _ = compose64(preact(t.numpy(), case["w"].numpy()), case["bg"].numpy())
    tol = lambda a: np.full_like(a, UP4_RANDOM_TOL)
    return {"pred": pred, "mask": m, "img": img, "E_pred": tol(pred), "E_mask": tol(m), "E_img": tol(img)}


# ------------------------------------------------------------------------------------------------------------------------------ reference and faults
FAULTS = ("tap_off_last_col", "drop_last_stage", "halo_row_zero", "prev_frame_pad", "swap_out23", "drop_kx4_first_cols", "bg_stride0", "tiles_swapped")


def _taps(x, ks, fault, tile):
    """src[ky][kx] = (B, H, W, C): the input value tap (ky, kx) reads for every output pixel, zero padding applied - with the planted fault if any."""
    B, H, W, C = x.shape
    p = ks // 2
    xp = np.zeros((B, H + 2 * p + 1, W + 2 * p + 1, C), x.dtype)
    xp[:, p:p + H, p:p + W] = x
    if fault == "prev_frame_pad":                      # the top padding of frame b holds frame b - 1's last rows (a missed gy >= 0)
        for r in range(min(p, H)):
            xp[1:, p - 1 - r, p:p + W] = x[:-1, H - 1 - r]
    th, tw = tile
    oy, ox = np.arange(H)[:, None], np.arange(W)[None, :]
    src = [[xp[:, ky:ky + H, kx:kx + W].copy() for kx in range(ks)] for ky in range(ks)]
    if fault == "tap_off_last_col":                    # tap (2, 3) one pixel to the right, for outputs in a tile's last column only
        sel = np.broadcast_to(ox % tw == tw - 1, (H, W))
        src[2][3][:, sel] = xp[:, 2:2 + H, 4:4 + W][:, sel]
    if fault == "halo_row_zero":                       # the halo row just above the second tile row reads as zero for that tile row's outputs
        for ky in range(ks):
            sel = np.broadcast_to((oy // th == 1) & (oy + ky - p == th - 1), (H, W))
            for kx in range(ks):
                src[ky][kx][:, sel] = 0
    if fault == "drop_kx4_first_cols":                 # the fifth horizontal tap dropped for a tile's first two columns
        sel = np.broadcast_to(ox % tw < 2, (H, W))
        for ky in range(ks):
            src[ky][4][:, sel] = 0
    return src


def preact(x, w, dtype=np.float64, order="ref", fault=None, tile=(16, 32), stage=8):
    """(B, H, W, N) pre-activations of the ks x ks convolution (zero padding ks // 2, no bias) of x (B, H, W, C) with w (N, C, ks, ks), every product
    and every add rounded to dtype, terms added in the form's documented order:
      "ref"   tap by tap, a tap's channels as one dot product (the float64 reference)
      "f32"   staged channels (8 at a time) -> ky -> kx -> channel      (lwg_head_compose_kernel, lwg_thin_conv_kernel)
      "q4"    channel quad -> kx -> ky -> channel                       (lwg_head_q4_kernel)
      "mfma"  per horizontal tap kx: ky -> channel, then the five partial sums in turn   (lwg_head_bf16_kernel, the fused up-sampling head)"""
    x, w = np.asarray(x, dtype), np.asarray(w, dtype)
    B, H, W, C = x.shape
    N, ks = w.shape[0], w.shape[2]
    if order == "ref" and fault is None and dtype == np.float64:
        s = F.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(w), padding=ks // 2)
        return s.permute(0, 2, 3, 1).contiguous().numpy()
    src = _taps(x, ks, fault, tile)
    if fault == "drop_last_stage":
        w = w.copy()
        w[:, C - (4 if order == "q4" else stage):] = 0
    acc = np.zeros((B, H, W, N), dtype)

    def term(ky, kx, c):
        return (src[ky][kx][..., c, None] * w[None, None, None, :, c, ky, kx]).astype(dtype)

    if order == "ref":
        for ky in range(ks):
            for kx in range(ks):
                acc = acc + src[ky][kx] @ w[:, :, ky, kx].T
    elif order == "f32":
        for c0 in range(0, C, stage):
            for ky in range(ks):
                for kx in range(ks):
                    for c in range(c0, min(C, c0 + stage)):
                        acc = (acc + term(ky, kx, c)).astype(dtype)
    elif order == "q4":
        for c0 in range(0, C, 4):
            for kx in range(ks):
                for ky in range(ks):
                    for c in range(c0, c0 + 4):
                        acc = (acc + term(ky, kx, c)).astype(dtype)
    elif order == "mfma":
        for kx in range(ks):
            part = np.zeros_like(acc)
            for ky in range(ks):
                for c in range(C):
                    part = (part + term(ky, kx, c)).astype(dtype)
            acc = (acc + part).astype(dtype)
    else:
        raise ValueError(order)
    if fault == "swap_out23" and N == 4:
        acc = acc[..., [0, 1, 3, 2]]
    return acc


def _nchw(a):
    return np.ascontiguousarray(np.moveaxis(a, -1, 1))


def compose64(s, bg, fault=None):
    """float64 (pred (B,3,H,W), mask (B,1,H,W), img (B,3,H,W), q = 1 - mask) from pre-activations s (B, H, W, 4)."""
    s, bg = np.asarray(s, np.float64), np.asarray(bg, np.float64)
    img = _nchw(np.tanh(s[..., :3]))
    m = _nchw(np.exp(-np.logaddexp(0.0, -s[..., 3:4])))
    q = _nchw(np.exp(-np.logaddexp(0.0, s[..., 3:4])))
    if fault == "bg_stride0":
        bg = bg[:1]
    return m * bg + q * img, m, img, q


def compose32(s, bg):
    """The kernels' epilogue in numpy float32: 1 / (1 + exp(-s)), tanh, m * bg + (1 - m) * img, each operation rounded."""
    s, bg = np.asarray(s, np.float32), np.asarray(bg, np.float32)
    with np.errstate(over="ignore", under="ignore"):
        img = _nchw(np.tanh(s[..., :3]))
        m = _nchw(np.float32(1) / (np.float32(1) + np.exp(-s[..., 3:4])))
        pred = m * bg + (np.float32(1) - m) * img
    return pred, m, img


def bounds(s, bg, e_s=None):
    """(E_pred, E_mask, E_img) of the module docstring at float64 pre-activations s; e_s: a bound on the pre-activation's own error (random family)."""
    _, m, img, q = compose64(s, bg)
    bg = np.abs(np.asarray(bg, np.float64))
    e_img = 4 * U * np.abs(img) + FLOOR
    e_m = m * (3 * U + 4 * U * q) * SECOND + FLOOR
    if e_s is not None:
        e_s = np.asarray(e_s, np.float64)
        e_img = e_img + _nchw(e_s[..., :3]) * SECOND
        e_m = e_m + 0.25 * _nchw(e_s[..., 3:4]) * SECOND
    e_q = e_m + U * q
    e_pred = (e_m * bg + e_q * np.abs(img) + q * e_img + 2 * U * (m * bg + q * np.abs(img))) * SECOND + FLOOR
    return e_pred, e_m, e_img


def preact_error_bound(x, w):
    """gamma(25 C + 8) sum |x||w| per output, (B, H, W, 4)."""
    C, ks = w.shape[1], w.shape[2]
    mag = preact(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64)))
    return gamma(ks * ks * C + 8) * mag


def reference(case, e_s=False):
    """{"s", "pred", "mask", "img"} in float64 and {"E_pred", "E_mask", "E_img"} for a head case (the up-sampling head: from its exact intermediate)."""
    x = case["t"] if "t" in case else case["x"]
    s = preact(x.numpy(), case["w"].numpy())
    bg = case["bg"].numpy()
    pred, m, img, _ = compose64(s, bg)
    es = preact_error_bound(x.numpy(), case["w"].numpy()) if e_s else None
    e_pred, e_m, e_img = bounds(s, bg, es)
    return {"s": s, "pred": pred, "mask": m, "img": img, "E_pred": e_pred, "E_mask": e_m, "E_img": e_img}


def ratios(got, ref, frames=None):
    """Worst |error| / bound of (pred, mask, img) arrays against reference(); frames: indices of the reference's frames that ``got`` holds."""
    out = {}
    for name, g in zip(("pred", "mask", "img"), got):
        if g is None:
            continue
        want, bound = ref[name], ref["E_" + name]
        if frames is not None:
            want, bound = want[list(frames)], bound[list(frames)]
        g = np.asarray(g, np.float64)
        assert g.shape == want.shape, (name, g.shape, want.shape)
        out[name] = worst_ratio(np.abs(g - want), bound)
    return out


def tiles_swapped(a, tile):
    """What a kernel that decodes its tile index with tiles_x and tiles_y exchanged writes into planes a (..., H, W): tile k of the row-major order
    lands at (k % tiles_y, k // tiles_y) - right values where it lands, nothing (NaN) where no tile lands."""
    H, W = a.shape[-2:]
    th, tw = tile
    ty, tx = -(-H // th), -(-W // tw)
    out = np.full_like(a, np.nan)
    for k in range(tx * ty):
        x0, y0 = (k % ty) * tw, (k // ty) * th
        out[..., y0:y0 + th, x0:x0 + tw] = a[..., y0:y0 + th, x0:x0 + tw]
    return out


# ------------------------------------------------------------------------------------------------------------------------------ layout kernels
LAYOUT_P = (1, 31, 32, 33, 65)
LAYOUT_C = (1, 3, 6, 31, 32, 33, 130)
LAYOUT_B = (1, 3)


def layout_pads(C):
    return sorted({C, C + 1, -(-C // 8) * 8})


def layout_src(B, C, P):
    """(B, C, P) of distinct values: every element names its own position (exact in fp32: B C P < 2^24)."""
    assert B * C * P < 2 ** 24
    return torch.arange(B * C * P, dtype=torch.float32).view(B, C, P) + 1.0


def nchw_to_nhwc_ref(src, Cp):
    B, C, P = src.shape
    out = torch.zeros(B, P, Cp)
    out[..., :C] = src.permute(0, 2, 1)
    return out


# ------------------------------------------------------------------------------------------------------------------------------ frames_to_u8
def u8_ref(x):
    """numpy's fp32 sequence of cv_utils.save_cv2_img(normalize=True)."""
    x = np.asarray(x, np.float32)
    return ((x + np.float32(1)) / np.float32(2.0) * np.float32(255)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def u8_threshold_values():
    """For every k in 1 .. 255 the fp32 neighbours (2 steps either way) of the smallest x in [-1, 1] whose output is k, then +-1, +-0 and the smallest
    normals: all inside the documented domain."""
    vals = []
    for k in range(1, 256):
        lo, hi = np.float32(-1), np.float32(1)
        while np.nextafter(lo, hi) < hi:                 # bisection on the fp32 number line: u8_ref is monotone on [-1, 1]
            mid = np.float32((np.float64(lo) + np.float64(hi)) / 2)
            mid = mid if lo < mid < hi else np.nextafter(lo, hi)
            if u8_ref(mid) >= k:
                hi = mid
            else:
                lo = mid
        assert u8_ref(hi) == k and u8_ref(lo) == k - 1, k
        v = hi
        for _ in range(2):
            v = np.nextafter(v, np.float32(-2))
        for _ in range(5):
            vals.append(v)
            v = np.nextafter(v, np.float32(2))
    tiny = np.float32(2.0 ** -126)
    vals += [np.float32(1), np.float32(-1), np.float32(0.0), np.float32(-0.0), tiny, -tiny]
    vals = np.array([v for v in vals if -1 <= v <= 1], np.float32)
    return vals


def u8_threshold_frames():
    """(1, 3, S, S): the threshold values dealt round the three channels (each channel starts at another value), padded by repetition."""
    v = u8_threshold_values()
    S = int(np.ceil(np.sqrt(len(v))))
    a = np.stack([np.resize(np.roll(v, 7 * c), S * S) for c in range(3)]).reshape(1, 3, S, S)
    return torch.tensor(a)


def u8_position_coded(B, S):
    """(B, 3, S, S) in [-1, 1] whose OUTPUT byte names its position: pixel i of channel c gives (i * 7 + c * 85 + i // 251) % 256 at the middle of the
    byte's interval (well inside: no threshold question)."""
    i = np.arange(B * S * S, dtype=np.int64).reshape(B, 1, S, S)
    c = np.arange(3, dtype=np.int64).reshape(1, 3, 1, 1)
    k = (i * 7 + c * 85 + i // 251) % 256
    x = ((k + 0.5) / 255.0 * 2.0 - 1.0).clip(-1, 1).astype(np.float32)
    assert np.array_equal(u8_ref(x), k.astype(np.uint8))
    return torch.tensor(x), torch.tensor(k.astype(np.uint8))
