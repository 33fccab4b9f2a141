"""The F(2x4, 2x2) transposed-convolution kernel (csrc/convt_winograd24.hip, lwg_conv_transpose4_winograd24_f32) on the GPU: the matrix of
gpu_checks.check_winograd_up4 / check_winograd_determinism / check_winograd_adversarial for the new kernel (small shapes reach it through
ops.WINO_UP4_24_MIN_HW = 0)."""
import contextlib

import numpy as np
import pytest
import torch

from ipercore_amd import _lib, ops
from ipercore_amd.networks import packing
from tests.gpu_checks import ADV_KINDS, DEV, _adversarial_operands, _cmp, _rand, _spec_dev

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _f24(on=True):
    """The "winograd" mode with the F(2x4, 2x2) kernel on every eligible transposed convolution (on) or on none (off)."""
    prev = ops.WINO_UP4_24, ops.WINO_UP4_24_MIN_HW
    ops.WINO_UP4_24, ops.WINO_UP4_24_MIN_HW = on, 0
    try:
        with ops.conv_precision("winograd"):
            yield
    finally:
        ops.WINO_UP4_24, ops.WINO_UP4_24_MIN_HW = prev


def _layer(Cin, N, seed):
    w = _rand((Cin, N, 4, 4), seed, 1.0 / np.sqrt(Cin * 4))
    b = _rand((N,), seed + 1, 0.1)
    return w, b, [_spec_dev(s_) for s_ in packing.pack_conv_transpose(w, b)]


_ACT = {ops.ACT_RELU: torch.relu, ops.ACT_TANH: torch.tanh, ops.ACT_NONE: lambda t: t}


@pytest.mark.parametrize("tag,B,H,W,Cin,N,act", [
    ("ragged_relu", 2, 24, 40, 64, 64, ops.ACT_RELU), ("odd_none", 1, 17, 31, 128, 64, ops.ACT_NONE), ("deep", 3, 16, 16, 256, 256, ops.ACT_RELU),
    ("last_layer", 2, 48, 64, 128, 64, ops.ACT_TANH), ("tiny", 1, 3, 5, 32, 64, ops.ACT_RELU), ("n96", 1, 20, 12, 64, 96, ops.ACT_NONE)])
def test_winograd24_matrix(tag, B, H, W, Cin, N, act):
    """fp64 reference at 2e-5; q4 = the NHWC values moved; an output channel slice of a wider tensor; a frame alone = the frame in its batch; not
    the direct kernel's bits, not the F(2x2, 2x2) kernel's; training callers keep the direct form; the hook kind stays "winograd_up4"."""
    w, b, specs = _layer(Cin, N, 500)
    x = _rand((B, H, W, Cin), 502)
    want = torch.nn.functional.conv_transpose2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), stride=2, padding=1)
    want = _ACT[act](want).permute(0, 2, 3, 1).float()
    xd = x.to(DEV)
    nan = lambda *sh: torch.full(sh, float("nan"), device=DEV)     # noqa: E731
    y24, y1, yq, yt, y22 = nan(B, 2 * H, 2 * W, N), nan(1, 2 * H, 2 * W, N), nan(B, N // 4, 2 * H, 2 * W, 4), nan(B, 2 * H, 2 * W, N), nan(B, 2 * H, 2 * W, N)
    ys = torch.zeros(B, 2 * H, 2 * W, N + 32, device=DEV)
    yd = nan(B, 2 * H, 2 * W, N)
    direct = N % 64 == 0                                                          # (the direct kernel needs N % 64 == 0)
    if direct:
        ops.conv_transpose2d(xd, specs, yd, act=act)
    seen = []
    prev_hook, ops.CONV_HOOK = ops.CONV_HOOK, (lambda begin, M, spec, epi=0, info=None: seen.append(info["kind"]) if not begin else None)
    try:
        with _f24():
            ops.conv_transpose2d(xd, specs, y24, act=act)
            ops.conv_transpose2d(xd[-1:].contiguous(), specs, y1, act=act)
            ops.conv_transpose2d(xd, specs, yq, act=act, q4=True)
            if direct:
                ops.conv_transpose2d(xd, specs, yt, act=act, splitk=True)      # a training caller: the direct form
            a = ops.conv_args(xd, specs[0], ys, act=act)
            a.ycoff, a.w = 16, ops._ptr(ops._wwino_t24(specs))
            _lib.check(_lib.lib().lwg_conv_transpose4_winograd24_f32(a, ops._stream()), "lwg_conv_transpose4_winograd24_f32")
    finally:
        ops.CONV_HOOK = prev_hook
    with _f24(False):
        ops.conv_transpose2d(xd, specs, y22, act=act)                           # the F(2x2, 2x2) kernel
    torch.cuda.synchronize()
    assert seen[:3] == ["winograd_up4"] * 3 and "winograd_up4" not in seen[3:], seen
    _cmp(y24, want, 2e-5, "F(2x4, 2x2) convT " + tag)
    if direct:
        assert not torch.equal(y24, yd) and torch.equal(yt, yd), tag
    assert not torch.equal(y24, y22), tag + ": the F(2x2, 2x2) kernel's bits (did the new kernel run?)"
    _cmp(y22, want, 2e-5, "F(2x2, 2x2) convT " + tag)
    assert torch.equal(y24[-1:], y1), tag + ": a frame's result depends on its launch batch"
    assert torch.equal(yq.permute(0, 2, 3, 1, 4).reshape(B, 2 * H, 2 * W, N), y24), tag + ": channel-quad-plane output differs from NHWC"
    assert torch.equal(ys[..., 16:16 + N], y24) and float(ys[..., :16].abs().max()) == 0.0 and float(ys[..., 16 + N:].abs().max()) == 0.0, tag


def test_winograd24_contract():
    """What the kernel does not take is refused before any launch."""
    _, _, specs = _layer(64, 64, 510)
    xd = _rand((1, 8, 8, 64), 512).to(DEV)
    y = torch.empty(1, 16, 16, 64, device=DEV)
    a = ops.conv_args(xd, specs[0], y, act=ops.ACT_RELU)
    a.w = ops._ptr(ops._wwino_t24(specs))
    for field, val in (("C0", 40), ("N", 48), ("ycoff", 2), ("epi", ops.EPI_RESIDUAL), ("ntaps", 9), ("omul", 1), ("act", ops.ACT_RELU_MASK)):
        keep = getattr(a, field)
        setattr(a, field, val)
        assert _lib.lib().lwg_conv_transpose4_winograd24_f32(a, None) == 1, field
        setattr(a, field, keep)
    assert _lib.lib().lwg_conv_transpose4_winograd24_f32(a, None) == 0
    torch.cuda.synchronize()


def test_winograd24_determinism():
    """The clip's launch sizes (several blocks per persistent workgroup, the XCD-aware block order), default dispatch: six repeats bit for bit, the
    batch's last frame = the frame alone."""
    reps = 6
    with ops.conv_precision("winograd"):
        for tag, B, H, Cin, Cout, q4 in (("up_64_256_256", 64, 64, 256, 256, False), ("up_128_256_128", 16, 128, 256, 128, False),
                                         ("up_256_128_64_q4", 4, 256, 128, 64, True)):
            assert ops._up4_24(torch.empty(1, H, H, 1)), tag
            _, _, specs = _layer(Cin, Cout, 520)
            x = _rand((B, H, H, Cin), 522).to(DEV)
            shape = (B, Cout // 4, 2 * H, 2 * H, 4) if q4 else (B, 2 * H, 2 * H, Cout)
            ys = []
            for _ in range(reps):
                y = torch.empty(*shape, device=DEV)
                ops.conv_transpose2d(x, specs, y, act=ops.ACT_RELU, q4=q4)
                ys.append(y)
            y1 = torch.empty(1, *shape[1:], device=DEV)
            ops.conv_transpose2d(x[-1:].contiguous(), specs, y1, act=ops.ACT_RELU, q4=q4)
            torch.cuda.synchronize()
            nd = sum(0 if torch.equal(ys[0], o) else 1 for o in ys[1:])
            assert nd == 0 and torch.equal(ys[0][-1:], y1), (tag, nd)
            assert torch.isfinite(ys[0]).all(), tag
            del ys


def test_winograd24_adversarial():
    """check_winograd_adversarial's transposed cases for the new kernel: relative L2 error against fp64 <= 4x the direct kernel's on the six
    adversarial operand kinds at Cin = 64 and 256 (ratios printed)."""
    rel = lambda y, ref: ((y.double().cpu() - ref).norm() / ref.norm()).item()      # noqa: E731
    ratios = {}
    for (B, H, W, Cin, N) in ((2, 32, 48, 64, 64), (1, 32, 32, 256, 256)):
        for kind in ADV_KINDS:
            w, x = _adversarial_operands(kind, Cin, (Cin, N, 4, 4), (B, H // 2, W // 2, Cin), 410 + Cin, cin_dim=0, fan=4 * Cin)
            b = _rand((N,), 411, 0.1)
            want = torch.nn.functional.conv_transpose2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), stride=2, padding=1).permute(0, 2, 3, 1)
            specs = [_spec_dev(s_) for s_ in packing.pack_conv_transpose(w, b)]
            xd = x.to(DEV)
            yd, yw, y22 = (torch.empty(B, H, W, N, device=DEV) for _ in range(3))
            ops.conv_transpose2d(xd, specs, yd)
            with _f24():
                ops.conv_transpose2d(xd, specs, yw)
            with _f24(False):
                ops.conv_transpose2d(xd, specs, y22)
            torch.cuda.synchronize()
            assert torch.isfinite(yw).all() and not torch.equal(yw, yd) and not torch.equal(yw, y22), kind
            ed, ew, e22 = rel(yd, want), rel(yw, want), rel(y22, want)
            ratios[f"{Cin}_{kind}"] = (round(ew / ed, 3), round(e22 / ed, 3))
            assert ew <= 4.0 * ed, (Cin, kind, ed, ew)
    print("F(2x4,2x2) / F(2x2,2x2) error over direct:", ratios)
