"""The fp32 / bf16 convolutions on the GPU at the edges of their 32-bit buffer-offset contracts (tests/test_conv_offsets_cpu.py audits the offsets
themselves): images whose tiles lie mostly right of or below the image, output images past 2 GiB and at the size limit, channel slices of a wider
tensor whose other channels must stay untouched, and batches at the batch-slicing boundary.

Inputs come from a seeded generator on the device (no multi-GiB host tensors); outputs are pre-filled with a NaN sentinel with a guard tail in the
same allocation - every output element must be written, nothing else.  Values are compared with an fp64 F.conv2d / F.conv_transpose2d on the CPU
over windows of at most 64 x 64 output pixels cut with their halo: image corners, the tile seams at the right / bottom edge, the rows where byte
offsets cross 2^31, and the pixels a wrapped dropped store would hit."""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ipercore_amd import _lib, ops
from ipercore_amd.networks import packing
from tests.gpu_checks import DEV, _cmp, _rand, _spec_dev

pytestmark = pytest.mark.gpu

SENT = 0x7FC0DEAD                                    # a quiet NaN with a payload no computation produces
SENT16 = 0x7FDA                                      # ... the same for bf16 outputs
GUARD = 4096                                         # elements of guard tail behind every output


def _gen_dev(shape, seed, dtype=torch.float32, scale=1.0):
    """Seeded normal values generated on the device in pieces (no multi-GiB temporaries)."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    out = torch.empty(shape, device=DEV, dtype=dtype)
    flat, step = out.view(-1), 1 << 27
    for i in range(0, flat.numel(), step):
        n = min(step, flat.numel() - i)
        flat[i:i + n] = torch.randn(n, generator=g, device=DEV) * scale
    return out


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32), (SENT16 if t.dtype == torch.bfloat16 else SENT)


def _sentinel(shape, dtype=torch.float32):
    """(view of shape, whole allocation) pre-filled with the sentinel; the allocation has GUARD elements of tail."""
    n = int(np.prod(shape))
    if dtype == torch.bfloat16:
        buf = torch.full((n + GUARD,), SENT16, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    else:
        buf = torch.full((n + GUARD,), SENT, dtype=torch.int32, device=DEV).view(torch.float32)
    return buf[:n].view(shape), buf


def _tail_ok(buf, n):
    return _untouched(buf[n:])


def _untouched(t):
    if not t.numel():
        return True
    b, sent = _bits(t)
    return bool((b == sent).all())


def _written_at(t, k=6):
    """The first k indices of t whose sentinel was overwritten (for failure messages)."""
    b, sent = _bits(t)
    return (b != sent).nonzero()[:k].tolist()


def _slice_ok(y, buf, c0, c1):
    """Channels c0 .. c1 of y all written (finite), every other channel and the guard tail untouched."""
    return (_tail_ok(buf, y.numel()) and _untouched(y[..., :c0]) and _untouched(y[..., c1:]) and bool(torch.isfinite(y[..., c0:c1].float()).all()))


@contextlib.contextmanager
def _mode(prec, **flags):
    prev = {k: getattr(ops, k) for k in flags}
    for k, v in flags.items():
        setattr(ops, k, v)
    try:
        with ops.conv_precision(prec):
            yield
    finally:
        for k, v in prev.items():
            setattr(ops, k, v)


def _wins(lo, hi, n, w=64):
    """Window starts (clipped to [0, n - w]) at the given positions."""
    return sorted({min(max(0, p), max(0, n - w)) for p in (lo + hi)})


# ---- transposed convolution (4, 2, 1) ----

def _convt_layer(Cin, N, seed):
    w = _rand((Cin, N, 4, 4), seed, 1.0 / np.sqrt(Cin * 4))
    b = _rand((N,), seed + 1, 0.1)
    return w, b, [_spec_dev(s_) for s_ in packing.pack_conv_transpose(w, b)]


def _convt_ref(x, w, b, act, r0, c0, h=64, wd=64):
    """fp64 ConvTranspose2d(4, 2, 1) of the device input x (1, H, W, C) at output rows r0 .. r0 + h, columns c0 .. c0 + wd (clipped), NHWC."""
    H, W = x.shape[1], x.shape[2]
    r1, c1 = min(2 * H, r0 + h), min(2 * W, c0 + wd)
    ia, ib = max(0, r0 // 2 - 1), min(H, r1 // 2 + 1)
    ja, jb = max(0, c0 // 2 - 1), min(W, c1 // 2 + 1)
    xs = x[:, ia:ib, ja:jb].cpu().double().permute(0, 3, 1, 2)
    y = F.conv_transpose2d(xs, w.double(), b.double(), stride=2, padding=1)
    y = y[:, :, r0 - 2 * ia:r1 - 2 * ia, c0 - 2 * ja:c1 - 2 * ja]
    if act == ops.ACT_RELU:
        y = torch.relu(y)
    return y.permute(0, 2, 3, 1), (r0, r1, c0, c1)


def _convt_launch(fn, x, specs, y, ycoff, act, q4):
    a = ops.conv_args(x, specs[0], y, act=act, q4=q4)
    a.ycoff = ycoff
    a.w = ops._ptr(ops._wwino_t24(specs) if fn.endswith("24_f32") else ops._wwino_t(specs))
    return getattr(_lib.lib(), fn)(a, ops._stream())


_CONVT = ("lwg_conv_transpose4_winograd_f32", "lwg_conv_transpose4_winograd24_f32")


@pytest.mark.parametrize("fn", _CONVT)
@pytest.mark.parametrize("q4", [False, True])
def test_convt_winograd_wide_ragged_channel_slice(fn, q4):
    """E1 + E5: four input rows of 150001 pixels (= 1 mod 16: the last column block has 1 of its 16 input columns inside the image), output channels
    32..63 of a 64-channel tensor.  With 16 passes of 2 output rows x 300002 x 64 x 4 bytes, the dropped stores' pass offsets reach 1 GiB: added to
    the out-of-range marker they wrapped past 2^32 into channels 0..3 of pixels (0/2/4/6, 5724) - the sentinel channels must stay bitwise intact."""
    B, H, W, Cin, N, YC, ycoff = 1, 4, 150001, 32, 32, 64, 32
    w, b, specs = _convt_layer(Cin, N, 700)
    x = _gen_dev((B, H, W, Cin), 701)
    shape = (B, YC // 4, 2 * H, 2 * W, 4) if q4 else (B, 2 * H, 2 * W, YC)
    y, buf = _sentinel(shape)
    assert _convt_launch(fn, x, specs, y, ycoff, ops.ACT_RELU, q4) == 0
    torch.cuda.synchronize()
    yn = y.permute(0, 2, 3, 1, 4).reshape(B, 2 * H, 2 * W, YC) if q4 else y
    assert _tail_ok(buf, y.numel()), fn + ": a store past the output"
    assert _untouched(yn[..., :ycoff]), "%s: channels below the launch's slice written at (b, y, x, c) %s (a dropped store wrapped into the image?)" % (
        fn, _written_at(yn[..., :ycoff]))
    assert bool(torch.isfinite(yn[..., ycoff:ycoff + N]).all()), fn + ": output elements left unwritten"
    for c0 in _wins([0, 5724 - 32, 2 * W // 2], [2 * W - 64], 2 * W):
        want, (r0, r1, a0, a1) = _convt_ref(x, w, b, ops.ACT_RELU, 0, c0)
        _cmp(yn[:, r0:r1, a0:a1, ycoff:ycoff + N], want.float(), 2e-5, "%s wide cols %d.." % (fn, c0))


@pytest.mark.parametrize("fn", _CONVT)
def test_convt_winograd_tall_narrow(fn):
    """E2: three input pixels of width, 65537 rows: every block is mostly right of the image, the last row block mostly below it."""
    B, H, W, Cin, N, YC = 1, 65537, 3, 32, 64, 96
    w, b, specs = _convt_layer(Cin, N, 710)
    x = _gen_dev((B, H, W, Cin), 711)
    y, buf = _sentinel((B, 2 * H, 2 * W, YC))
    assert _convt_launch(fn, x, specs, y, 0, ops.ACT_NONE, False) == 0
    torch.cuda.synchronize()
    assert _tail_ok(buf, y.numel()) and _untouched(y[..., N:]) and bool(torch.isfinite(y[..., :N]).all()), fn
    for r0 in _wins([0, H], [2 * H - 64], 2 * H):
        want, (a0, a1, c0, c1) = _convt_ref(x, w, b, ops.ACT_NONE, r0, 0)
        _cmp(y[:, a0:a1, c0:c1, :N], want.float(), 2e-5, "%s tall rows %d.." % (fn, r0))


def _convt_limit_w(H, YC):
    """The widest input the transposed Winograd contract accepts at H rows: (2H + 32) rows of 2 W pixels x YC x 4 bytes < 3 GiB."""
    W = 0xC0000000 // ((2 * H + 32) * 2 * YC * 4)
    while (2 * H + 32) * 2 * (W + 1) * YC * 4 < 0xC0000000:
        W += 1
    while (2 * H + 32) * 2 * W * YC * 4 >= 0xC0000000:
        W -= 1
    return W


@pytest.mark.parametrize("fn", _CONVT)
def test_convt_winograd_at_the_size_limit(fn):
    """E3 + E4: the largest output image the contract accepts at 1201 input rows (3.1 GiB: byte offsets cross 2^31 near row 2100); one pixel wider
    is refused on the host and leaves the output untouched.  Windows: corners, the 2^31 crossing, the last rows at the right edge."""
    H, Cin, N, YC = 1201, 32, 32, 32
    W = _convt_limit_w(H, YC)
    assert 2 * H * 2 * W * YC * 4 > 2 ** 31
    w, b, specs = _convt_layer(Cin, N, 720)
    x1 = _gen_dev((1, H, W + 1, Cin), 721)
    y1, buf = _sentinel((1, 2 * H, 2 * (W + 1), YC))                   # (sized for the refused shape: nothing could land outside it)
    assert _convt_launch(fn, x1, specs, y1, 0, ops.ACT_RELU, False) == 1
    torch.cuda.synchronize()
    assert _untouched(buf), fn + ": a refused launch wrote"
    del x1
    x = _gen_dev((1, H, W, Cin), 722)
    n = 2 * H * 2 * W * YC
    y = buf[:n].view(1, 2 * H, 2 * W, YC)
    assert _convt_launch(fn, x, specs, y, 0, ops.ACT_RELU, False) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all()), fn + ": output elements left unwritten"
    assert _untouched(buf[n:]), fn + ": a store past the output image"
    rx = 2 ** 31 // (2 * W * YC * 4)
    for r0 in _wins([0, rx - 32, rx], [2 * H - 64], 2 * H):
        for c0 in _wins([0], [2 * W - 64], 2 * W):
            want, (a0, a1, d0, d1) = _convt_ref(x, w, b, ops.ACT_RELU, r0, c0)
            _cmp(y[:, a0:a1, d0:d1], want.float(), 2e-5, "%s limit rows %d cols %d" % (fn, r0, c0))
    del x, y, y1, buf
    torch.cuda.empty_cache()


# ---- 3 x 3 / stride 1 convolutions ----

def _conv_ref(x, w, b, r0, c0, h=64, wd=64, res=None):
    """fp64 3 x 3 / pad 1 convolution of the device input x (1, H, W, C) at rows r0 .. r0 + h, columns c0 .. c0 + wd (clipped), NHWC; + res."""
    H, W = x.shape[1], x.shape[2]
    r1, c1 = min(H, r0 + h), min(W, c0 + wd)
    ia, ja = max(0, r0 - 1), max(0, c0 - 1)
    xs = x[:, ia:min(H, r1 + 1), ja:min(W, c1 + 1)].cpu().double().permute(0, 3, 1, 2)
    y = F.conv2d(xs, w.double(), b.double(), padding=1)[:, :, r0 - ia:r1 - ia, c0 - ja:c1 - ja].permute(0, 2, 3, 1)
    if res is not None:
        y = y + res[:, r0:r1, c0:c1].cpu().double()
    return y, (r0, r1, c0, c1)


def _conv_layer(Cin, N, seed):
    w = _rand((N, Cin, 3, 3), seed, (Cin * 9) ** -0.5)
    b = _rand((N,), seed + 1, 0.1)
    return w, b, _spec_dev(packing.pack_conv(w, b, stride=1, pad=1))


_CONV_MODES = {
    "direct": dict(prec="fp32"),
    "split": dict(prec="split"),
    "winograd": dict(prec="winograd", WINO4=False),
    "winograd4": dict(prec="winograd", WINO4=True, WINO4_MIN_CIN=0),
}


@pytest.mark.parametrize("mode", list(_CONV_MODES))
def test_conv3x3_wide_ragged_residual_slice(mode):
    """E1 + E5 for the fp32 3 x 3 engines: four rows of 262145 pixels (= 1 mod 16; rows x row stride = 1.07 GB), a residual epilogue into channels
    128..191 of a 256-channel tensor."""
    B, H, W, Cin, N, YC, ycoff = 1, 4, 262145, 64, 64, 256, 128
    w, b, spec = _conv_layer(Cin, N, 730)
    x = _gen_dev((B, H, W, Cin), 731)
    res = _gen_dev((B, H, W, YC), 732)
    y, buf = _sentinel((B, H, W, YC))
    kw = dict(_CONV_MODES[mode])
    prec = kw.pop("prec")
    seen = []
    prev, ops.CONV_HOOK = ops.CONV_HOOK, (lambda begin, M, spec, epi=0, info=None: seen.append(info["kind"]) if not begin else None)
    try:
        with _mode(prec, **kw):
            ops.conv2d(x, spec, y, epi=ops.EPI_RESIDUAL, act=ops.ACT_RELU, res=res, ycoff=ycoff)
    finally:
        ops.CONV_HOOK = prev
    torch.cuda.synchronize()
    assert seen == [mode], seen
    assert _slice_ok(y, buf, ycoff, ycoff + N), "%s: writes outside the channel slice at %s, or outputs left unwritten" % (mode, _written_at(y[..., :ycoff]))
    for c0 in _wins([0, W // 2], [W - 64], W):
        want, (r0, r1, a0, a1) = _conv_ref(x, w, b, 0, c0, res=res[..., ycoff:ycoff + N])
        _cmp(y[:, r0:r1, a0:a1, ycoff:ycoff + N], torch.relu(want).float(), 2e-5, "%s wide cols %d.." % (mode, c0))


def test_winograd4_past_2gib():
    """E3 for the F(4x4, 3x3) kernel: one 2049 x 4097 x 64 image (2.15 GiB in and out, plus a residual of the same size): output and residual
    offsets cross 2^31 inside the image; windows at the crossing, the last rows and the right edge."""
    H, W, C = 2049, 4097, 64
    w, b, spec = _conv_layer(C, C, 740)
    x = _gen_dev((1, H, W, C), 741)
    res = _gen_dev((1, H, W, C), 742)
    y, buf = _sentinel((1, H, W, C))
    with _mode("winograd", WINO4=True, WINO4_MIN_CIN=0):
        ops.conv2d(x, spec, y, epi=ops.EPI_RESIDUAL, act=ops.ACT_NONE, res=res)
    torch.cuda.synchronize()
    assert _tail_ok(buf, y.numel()) and bool(torch.isfinite(y).all())
    rx = 2 ** 31 // (W * C * 4)
    for r0 in _wins([0, rx - 32, rx], [H - 64], H):
        for c0 in _wins([0], [W - 64], W):
            want, (a0, a1, d0, d1) = _conv_ref(x, w, b, r0, c0, res=res)
            _cmp(y[:, a0:a1, d0:d1], want.float(), 2e-5, "winograd4 rows %d cols %d" % (r0, c0))
    del x, res, y, buf
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_batch_slicing_boundary(dtype):
    """E6: lwg_conv_run_sliced.  A batch of 256 x 256 x 64 frames whose input is one frame under 3 GiB runs as one launch; one frame more makes
    B * per = 0xC0000000 and is cut into slices of (0xC0000000 - 1) / per frames: the last slice is ONE frame.  Every frame equals its one-frame
    launch bitwise; a few frames against fp64 (fp32: 2e-5; bf16: the bf16 checks' bound on rounded operands)."""
    Hs, C = 256, 64
    esz = 2 if dtype == torch.bfloat16 else 4
    per = Hs * Hs * C * esz
    n = 0xC0000000 // per
    assert n * per == 0xC0000000
    w, b, spec = _conv_layer(C, C, 750)
    x = _gen_dev((n, Hs, Hs, C), 751, dtype)
    for B in (n - 1, n):
        xb = x[:B]
        a = ops.conv_args(xb, spec, torch.empty(1, Hs, Hs, C, device=DEV, dtype=dtype))
        a.B, a.M = B, B * Hs * Hs
        assert _lib.lib().lwg_conv_slice_count(a) == (1 if B < n else 2)
        y = torch.empty((B, Hs, Hs, C), device=DEV, dtype=dtype)
        ops.conv2d(xb, spec, y, act=ops.ACT_RELU)
        y1 = torch.empty((1, Hs, Hs, C), device=DEV, dtype=dtype)
        frames = range(B) if B == n else (0, B // 2, B - 1)
        for f in frames:
            ops.conv2d(xb[f:f + 1], spec, y1, act=ops.ACT_RELU)
            assert torch.equal(y1[0], y[f]), "frame %d of %d differs from its one-frame launch" % (f, B)
        for f in (0, B - 1):
            want, (r0, r1, c0, c1) = _conv_ref(xb[f:f + 1].float(), w, b, Hs - 64, Hs - 64)
            got = y[f:f + 1, r0:r1, c0:c1].float()
            if dtype == torch.float32:
                _cmp(got, torch.relu(want).float(), 2e-5, "sliced frame %d" % f)
            else:
                wq, bq = w.to(torch.bfloat16).double(), b
                wantq, _ = _conv_ref(xb[f:f + 1].float(), wq, bq, Hs - 64, Hs - 64)
                _cmp(got, torch.relu(wantq).float(), 2e-2, "sliced bf16 frame %d" % f)
        del y
    del x
    torch.cuda.empty_cache()


def _conv_ref_s(x, w, b, stride=1, pad=1):
    """fp64 convolution of a whole (small) NHWC input, NHWC result."""
    return F.conv2d(x.cpu().double().permute(0, 3, 1, 2), w.double(), None if b is None else b.double(), stride=stride, padding=pad).permute(0, 2, 3, 1)


def test_winograd4_wide_two_inputs():
    """E1 + E5 for the F(4x4, 3x3) kernel with a skip concatenation: two 32-channel inputs, four rows of 262145 pixels, output channels 128..191 of a
    256-channel tensor (1.07 GB)."""
    H, W, C0, C1, N, YC, ycoff = 4, 262145, 32, 32, 64, 256, 128
    w, b, spec = _conv_layer(C0 + C1, N, 770)
    x0, x1 = _gen_dev((1, H, W, C0), 771), _gen_dev((1, H, W, C1), 772)
    y, buf = _sentinel((1, H, W, YC))
    with _mode("winograd", WINO4=True, WINO4_MIN_CIN=0):
        ops.conv2d(x0, spec, y, x1=x1, act=ops.ACT_RELU, ycoff=ycoff)
    torch.cuda.synchronize()
    assert _slice_ok(y, buf, ycoff, ycoff + N), _written_at(y[..., :ycoff])
    for c0 in _wins([0, W // 2], [W - 64], W):
        want, (r0, r1, a0, a1) = _conv_ref(torch.cat([x0[:, :, max(0, c0 - 1):c0 + 65], x1[:, :, max(0, c0 - 1):c0 + 65]], 3), w, b, 0, min(c0, 1))
        _cmp(y[:, r0:r1, c0:c0 + (a1 - a0), ycoff:ycoff + N], torch.relu(want).float(), 2e-5, "winograd4 two inputs cols %d.." % c0)


def test_winograd4_wide_spade():
    """E1 for the F(4x4, 3x3) kernel's SPADE epilogue: four rows of 262145 pixels, 256 channels (gamma | beta: 512 GEMM columns), the normalised
    tensor read with the output's offsets (1.07 GB each)."""
    H, W, Cin, C = 4, 262145, 64, 256
    wg, bg_, wb, bb_ = _rand((C, Cin, 3, 3), 780, 0.03), _rand((C,), 781, 0.1), _rand((C, Cin, 3, 3), 782, 0.03), _rand((C,), 783, 0.1)
    sp = _spec_dev(packing.pack_spade_gamma_beta(wg, bg_, wb, bb_))
    x, xn = _gen_dev((1, H, W, Cin), 784), _gen_dev((1, H, W, C), 785, scale=2.0)
    mean, rstd = _gen_dev((1, C), 786, scale=0.1), _gen_dev((1, C), 787, scale=0.1).abs() + 0.5
    y, buf = _sentinel((1, H, W, C))
    with _mode("winograd", WINO4=True, WINO4_MIN_CIN=0):
        ops.conv2d(x, sp, y, epi=ops.EPI_SPADE, act=ops.ACT_RELU, xn=xn, mean=mean, rstd=rstd)
    torch.cuda.synchronize()
    assert _slice_ok(y, buf, 0, C)
    wcat, bcat = torch.cat([wg, wb]), torch.cat([bg_, bb_])
    for c0 in _wins([0, W // 2], [W - 64], W):
        gb, (r0, r1, a0, a1) = _conv_ref(x, wcat, bcat, 0, c0)
        xs = xn[:, r0:r1, a0:a1].cpu().double()
        want = torch.relu((xs - mean.cpu().double().view(1, 1, 1, C)) * rstd.cpu().double().view(1, 1, 1, C) * (1 + gb[..., :C]) + gb[..., C:])
        _cmp(y[:, r0:r1, a0:a1], want.float(), 1e-4, "winograd4 SPADE cols %d.." % c0)


def test_direct_splitk_workspace_channel_slice():
    """E5 for the split-K workspace form of the direct kernel (lwg_conv2d_nhwc_f32_ws; only small-M launches are split, so no wide image reaches it):
    a ragged 15 x 17 frame, 256 -> 256 channels written at 64..319 of a 384-channel tensor through the finishing kernel."""
    H, W, Cin, N, YC, ycoff = 15, 17, 256, 256, 384, 64
    w, b, spec = _conv_layer(Cin, N, 790)
    x = _gen_dev((1, H, W, Cin), 791)
    y, buf = _sentinel((1, H, W, YC))
    a = ops.conv_args(x, spec, y, act=ops.ACT_RELU, ycoff=ycoff)
    assert _lib.lib().lwg_conv2d_ws_floats(a) > 0, "the launch is not split: the test no longer reaches the workspace form"
    with _mode("fp32"):
        ops.conv2d(x, spec, y, act=ops.ACT_RELU, ycoff=ycoff, splitk=True)
    torch.cuda.synchronize()
    assert _slice_ok(y, buf, ycoff, ycoff + N), _written_at(y[..., :ycoff])
    _cmp(y[..., ycoff:ycoff + N], torch.relu(_conv_ref_s(x, w, b)).float(), 2e-5, "split-K workspace form")


# ---- bf16 convolutions; the direct transposed forms ----

@pytest.mark.parametrize("hr", [True, False])
def test_bf16_conv3x3_wide_slice_and_past_2gib(hr):
    """E1 + E5 and E3 for lwg_conv2d_nhwc_bf16_hr (hr) and lwg_conv2d_nhwc_bf16: four rows of 262145 pixels into channels 128..191 of a 512-channel
    bf16 tensor (1.07 GB), then one 2049 x 4097 x 128 image (2.15 GB in and out: offsets cross 2^31 inside it)."""
    w, b, spec = _conv_layer(64, 64, 800)
    wq = w.to(torch.bfloat16).double()
    with _mode("fp32", BF16_HR=hr, BF16_PW=False):
        H, W, YC, ycoff = 4, 262145, 512, 128
        x = _gen_dev((1, H, W, 64), 801, torch.bfloat16)
        y, buf = _sentinel((1, H, W, YC), torch.bfloat16)
        ops.conv2d(x, spec, y, act=ops.ACT_RELU, ycoff=ycoff)
        torch.cuda.synchronize()
        assert _slice_ok(y, buf, ycoff, ycoff + 64), _written_at(y[..., :ycoff])
        for c0 in _wins([0, W // 2], [W - 64], W):
            want, (r0, r1, a0, a1) = _conv_ref(x.float(), wq, b, 0, c0)
            _cmp(y[:, r0:r1, a0:a1, ycoff:ycoff + 64].float(), torch.relu(want).float(), 2e-2, "bf16 hr=%s wide cols %d.." % (hr, c0))
        del x, y, buf
        w2, b2, spec2 = _conv_layer(128, 128, 805)
        w2q = w2.to(torch.bfloat16).double()
        H, W = 2049, 4097
        x = _gen_dev((1, H, W, 128), 806, torch.bfloat16)
        y, buf = _sentinel((1, H, W, 128), torch.bfloat16)
        ops.conv2d(x, spec2, y, act=ops.ACT_RELU)
        torch.cuda.synchronize()
        assert _slice_ok(y, buf, 0, 128)
        rx = 2 ** 31 // (W * 128 * 2)
        for r0 in _wins([0, rx - 32, rx], [H - 64], H):
            for c0 in _wins([0], [W - 64], W):
                want, (a0, a1, d0, d1) = _conv_ref(x, w2q, b2, r0, c0)
                _cmp(y[:, a0:a1, d0:d1].float(), torch.relu(want).float(), 2e-2, "bf16 hr=%s past 2 GiB rows %d cols %d" % (hr, r0, c0))
    del x, y, buf
    torch.cuda.empty_cache()


def test_bf16_c8_first_layer_wide_slice():
    """E1 + E5 for lwg_conv2d_nhwc_c8_bf16 (fp32 8-channel input rounded to bf16 in registers, bf16 output): three rows of 262145 pixels into
    channels 64..127 of a 1024-channel tensor (1.6 GB)."""
    H, W, YC, ycoff = 3, 262145, 1024, 64
    w, b, spec = _conv_layer(8, 64, 810)
    x = _gen_dev((1, H, W, 8), 811)
    y, buf = _sentinel((1, H, W, YC), torch.bfloat16)
    assert spec.Cin == 8 and spec.N == 64                                   # (what ops.conv2d routes to the c8 kernel)
    with _mode("fp32", BF16_C8=True):
        ops.conv2d(x, spec, y, act=ops.ACT_RELU, ycoff=ycoff)
    torch.cuda.synchronize()
    assert _slice_ok(y, buf, ycoff, ycoff + 64), _written_at(y[..., :ycoff])
    wq = w.to(torch.bfloat16).double()
    for c0 in _wins([0, W // 2], [W - 64], W):
        want, (r0, r1, a0, a1) = _conv_ref(x.to(torch.bfloat16).float(), wq, b, 0, c0)
        _cmp(y[:, r0:r1, a0:a1, ycoff:ycoff + 64].float(), torch.relu(want).float(), 2e-2, "c8 bf16 wide cols %d.." % c0)


def _convt_direct(x, specs, y, ycoff, act):
    """lwg_conv_transpose4_nhwc_f32 / _bf16 called directly (a channel slice ycoff); returns (error code, args, panel)."""
    a = ops.conv_args(x, specs[0], y, act=act)
    a.ycoff = ycoff
    if x.dtype == torch.bfloat16:
        panel = ops._w16up(specs)
        a.w = ops._ptr(panel, torch.bfloat16)
        return _lib.lib().lwg_conv_transpose4_nhwc_bf16(a, ops._stream()), a, panel
    panel = ops._w32up(specs)
    a.w = ops._ptr(panel)
    return _lib.lib().lwg_conv_transpose4_nhwc_f32(a, ops._stream()), a, panel


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H,W", [(2, 131073), (5, 1001)])
def test_convt_direct_wide_ragged_channel_slice(dtype, H, W):
    """E1 + E5 for lwg_conv_transpose4_nhwc_f32 (the wide image as four parity launches, the small one as ONE grid) and lwg_conv_transpose4_nhwc_bf16:
    output channels 128..191 of a wider tensor (wide: 1.07 GB of output rows)."""
    Cin, N, ycoff = 128, 64, 128
    YC = (256 if dtype == torch.float32 else 512) if W > 10000 else 256
    w, b, specs = _convt_layer(Cin, N, 820)
    x = _gen_dev((1, H, W, Cin), 821, dtype)
    y, buf = _sentinel((1, 2 * H, 2 * W, YC), dtype)
    e, a, panel = _convt_direct(x, specs, y, ycoff, ops.ACT_RELU)
    assert e == 0
    if dtype == torch.float32:
        assert _lib.lib().lwg_conv_transpose4_is_one_grid(a) == (1 if W < 10000 else 0)
    torch.cuda.synchronize()
    assert _slice_ok(y, buf, ycoff, ycoff + N), _written_at(y[..., :ycoff])
    wq, tol = (w.to(torch.bfloat16).float(), 2e-2) if dtype == torch.bfloat16 else (w, 2e-5)
    for c0 in _wins([0, W], [2 * W - 64], 2 * W):
        want, (r0, r1, a0, a1) = _convt_ref(x.float(), wq, b, ops.ACT_RELU, 0, c0)
        _cmp(y[:, r0:r1, a0:a1, ycoff:ycoff + N].float(), want.float(), tol, "convT direct %s cols %d.." % (dtype, c0))


def _frames_equal_one_frame(run, xb, y, frames):
    """Each frame of the batched result y bitwise equal to its one-frame launch run(x1, y1)."""
    y1 = torch.empty_like(y[:1])
    for f in frames:
        run(xb[f:f + 1], y1)
        assert torch.equal(y1[0], y[f]), "frame %d of %d differs from its one-frame launch" % (f, y.shape[0])


@pytest.mark.parametrize("kind", ["convt_f32", "convt_bf16", "c8_bf16"])
def test_batch_slicing_boundary_other_entry_points(kind):
    """E6 for the other sliced entry points: lwg_conv_transpose4_nhwc_f32 (256-channel 128 x 128 frames: 16 MiB each), lwg_conv_transpose4_nhwc_bf16
    (128 channels: 4 MiB) and lwg_conv2d_nhwc_c8_bf16 (fp32 8-channel 512 x 512 frames, 3 x 3 / stride 2: 8 MiB).  One frame under the range: one launch;
    B * per = 0xC0000000: slices of (0xC0000000 - 1) / per frames, the last one ONE frame - every frame bitwise its one-frame launch."""
    if kind == "convt_f32":
        Hs, C, dtype, xdt = 128, 256, torch.float32, torch.float32
    elif kind == "convt_bf16":
        Hs, C, dtype, xdt = 128, 128, torch.bfloat16, torch.bfloat16
    else:
        Hs, C, dtype, xdt = 512, 8, torch.bfloat16, torch.float32
    per = Hs * Hs * C * (2 if xdt == torch.bfloat16 else 4)
    n = 0xC0000000 // per
    assert n * per == 0xC0000000
    if kind == "c8_bf16":
        w, b, spec = _conv_layer(8, 64, 830)
        spec = _spec_dev(packing.pack_conv(w, b, stride=2, pad=1))
        oshape = (Hs // 2, Hs // 2, 64)

        def run(xb, y):
            with _mode("fp32", BF16_C8=True):
                ops.conv2d(xb, spec, y, act=ops.ACT_RELU)
    else:
        w, b, specs = _convt_layer(C, 64, 831)
        oshape = (2 * Hs, 2 * Hs, 64)

        def run(xb, y):
            e, _, panel = _convt_direct(xb, specs, y, 0, ops.ACT_RELU)
            assert e == 0
            torch.cuda.synchronize()
    x = _gen_dev((n, Hs, Hs, C), 832, xdt)
    for B in (n - 1, n):
        xb = x[:B]
        a = ops.conv_args(xb, spec if kind == "c8_bf16" else specs[0], torch.empty((1,) + oshape, device=DEV, dtype=dtype))
        a.B = B
        a.M = B * a.OH * a.OW
        assert _lib.lib().lwg_conv_slice_count(a) == (1 if B < n else 2)
        y = torch.empty((B,) + oshape, device=DEV, dtype=dtype)
        run(xb, y)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(y[-1].float()).all())
        _frames_equal_one_frame(run, xb, y, range(B) if B == n else (0, B // 2, B - 1))
        if kind != "c8_bf16":
            wq, tol = (w.to(torch.bfloat16).float(), 2e-2) if dtype == torch.bfloat16 else (w, 2e-5)
            want, (r0, r1, c0, c1) = _convt_ref(xb[B - 1:B].float(), wq, b, ops.ACT_RELU, 2 * Hs - 64, 2 * Hs - 64)
            _cmp(y[B - 1:B, r0:r1, c0:c1].float(), want.float(), tol, "%s last frame of %d" % (kind, B))
        del y
    del x
    torch.cuda.empty_cache()


def _up4_head_ref(x, w, bsv, w5, bg, r0, c0, h=32, wd=32):
    """fp64 ReLU(ConvTranspose2d(4, 2, 1)) -> bf16 -> 5 x 5 regressors -> tanh / sigmoid -> compositing at output rows r0 .., columns c0 .. (clipped)."""
    H, W = x.shape[1], x.shape[2]
    r1, c1 = min(2 * H, r0 + h), min(2 * W, c0 + wd)
    tr0, tr1, tc0, tc1 = r0 - 2, r1 + 2, c0 - 2, c1 + 2
    cr0, cr1, cc0, cc1 = max(0, tr0), min(2 * H, tr1), max(0, tc0), min(2 * W, tc1)
    t, _ = _convt_ref(x.float(), w, bsv, ops.ACT_RELU, cr0, cc0, cr1 - cr0, cc1 - cc0)
    t = t.permute(0, 3, 1, 2).to(torch.bfloat16).double()
    t = F.pad(t, (cc0 - tc0, tc1 - cc1, cr0 - tr0, tr1 - cr1))
    s5 = F.conv2d(t, w5, padding=0)
    img, m = torch.tanh(s5[:, :3]), torch.sigmoid(s5[:, 3:4])
    return m * bg[:, :, r0:r1, c0:c1].cpu().double() + (1 - m) * img, m, (r0, r1, c0, c1)


def test_up4_head_compose_wide_and_slicing():
    """E1 and E6 for lwg_up4_head_compose_bf16: two input rows of 131073 pixels (tiles mostly right of the image), against fp64 with the bf16-rounded
    operands and intermediate (the bound of tests/gpu_checks.check_bf16_up4_head); then 128 x 128 frames (4 MiB each) in batches one frame under and
    exactly at the 32-bit range (the last slice one frame) - every frame bitwise its one-frame launch."""
    w = _rand((128, 64, 4, 4), 840, 1.0 / np.sqrt(128 * 4))
    bsv = _rand((64,), 841, 0.1)
    w_img, w_att = _rand((3, 64, 5, 5), 842, 0.05), _rand((1, 64, 5, 5), 843, 0.05)
    specs = [_spec_dev(s_) for s_ in packing.pack_conv_transpose(w, bsv)]
    head16 = packing.pack_head_bf16(w_img, w_att).to(DEV)
    wq, w5 = w.to(torch.bfloat16).float(), torch.cat([w_img, w_att]).to(torch.bfloat16).double()
    H, W = 2, 131073
    x = _gen_dev((1, H, W, 128), 844, torch.bfloat16)
    bg = _gen_dev((1, 3, 2 * H, 2 * W), 845, scale=0.5)
    assert ops.up4_head_eligible(x, specs, ops.ACT_RELU)
    pred, mask, _ = ops.up4_head_compose_bf16(x, specs, head16, bg, want_pred=True, want_mask=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(pred).all()) and bool(torch.isfinite(mask).all())
    for c0 in _wins([0, W], [2 * W - 32], 2 * W, 32):
        pr, mr, (r0, r1, a0, a1) = _up4_head_ref(x, wq, bsv, w5, bg, 0, c0)
        _cmp(pred[:, :, r0:r1, a0:a1], pr.float(), 2e-2, "up4 head pred cols %d.." % c0)
        _cmp(mask[:, :, r0:r1, a0:a1], mr.float(), 2e-2, "up4 head mask cols %d.." % c0)
    del x, bg, pred, mask
    Hs = 128
    n = (0xC0000000) // (Hs * Hs * 256)
    x = _gen_dev((n, Hs, Hs, 128), 846, torch.bfloat16)
    bg = _gen_dev((1, 3, 2 * Hs, 2 * Hs), 847, scale=0.5)
    for B in (n - 1, n):
        xb = x[:B]
        pred, mask, _ = ops.up4_head_compose_bf16(xb, specs, head16, bg, want_pred=True, want_mask=True)
        frames = range(B) if B == n else (0, B // 2, B - 1)
        for f in frames:
            p1, m1, _ = ops.up4_head_compose_bf16(xb[f:f + 1], specs, head16, bg, want_pred=True, want_mask=True)
            assert torch.equal(p1[0], pred[f]) and torch.equal(m1[0], mask[f]), "up4 head: frame %d of %d differs from its one-frame launch" % (f, B)
        del pred, mask
    del x
    torch.cuda.empty_cache()
