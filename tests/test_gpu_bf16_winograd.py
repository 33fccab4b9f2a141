"""The bf16 F(2x2, 3x3) Winograd convolution (csrc/conv_winograd_bf16.hip, ops.conv_precision("bf16_winograd")) on the GPU: every launch kind of
its contract against an fp64 CPU convolution of the same bf16-rounded operands, beside the "bf16"-mode kernel on those operands; batch invariance,
run-to-run determinism, the launches the mode must leave alone, the host contract, and the whole per-frame path."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ipercore_amd import _lib, ops
from ipercore_amd.networks import packing
from tests import parity_utils as pu
from tests.gpu_checks import ADV_KINDS, DEV, _adversarial_operands, _psnr, _spec_dev

pytestmark = pytest.mark.gpu

MAX_REL = 2.4e-2      # of the reference's maximum: twice _bf16_kernel_case's 1.2e-2 (the emulated error ratio is <= 1.9x)
RATIO = 3.0           # relative L2 against fp64, in units of the "bf16"-mode kernel's on the same operands (tests/bf16wino_emu.py)


def r16(t):
    return t.to(torch.bfloat16).float()


def _nchw(t):
    return t.double().permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


class _Hook:
    def __init__(self):
        self.kinds = []

    def __call__(self, begin, M, spec, epi, info):
        if not begin:
            self.kinds.append(info["kind"])


def _launch(mode, x0, sp, yshape, x1=None, **kw):
    """One ops.conv2d call in ``mode`` on a NaN-filled bf16 output -> (y, hook kinds)."""
    y = torch.full(yshape, float("nan"), device=DEV, dtype=torch.bfloat16)
    hook, prev = _Hook(), ops.CONV_HOOK
    ops.CONV_HOOK = hook
    try:
        with ops.conv_precision(mode):
            ops.conv2d(x0, sp, y, x1=x1, **kw)
    finally:
        ops.CONV_HOOK = prev
    torch.cuda.synchronize()
    return y, hook.kinds


def _rel_l2(y, want):
    return ((y.double().cpu() - want).pow(2).sum().sqrt() / want.pow(2).sum().sqrt()).item()


def _build(B, H, W, C0, C1, N, kind, seed, act=ops.ACT_RELU, operands=None):
    """Operands as gpu_checks._bf16_kernel_case builds them (bf16-rounded, fp64 CPU reference on the same values)."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *sh, sc=1.0: r16(torch.randn(*sh, generator=g) * sc)                    # noqa: E731
    Cin = C0 + C1
    if operands is None:
        xin = rnd(B, H, W, Cin)
        w = rnd(N, Cin, 3, 3, sc=(Cin * 9) ** -0.5)
    else:
        w, xin = operands
        w, xin = r16(w), r16(xin)
    x0c, x1c = xin[..., :C0].contiguous(), (xin[..., C0:].contiguous() if C1 else None)
    kw = {}
    if kind == "spade":
        wb = rnd(N, Cin, 3, 3, sc=(Cin * 9) ** -0.5)
        bg_, bb_ = 0.1 * torch.randn(N, generator=g), 0.1 * torch.randn(N, generator=g)
        sp = _spec_dev(packing.pack_spade_gamma_beta(w, bg_, wb, bb_))
        xn, mean, rstd = rnd(B, H, W, N), torch.randn(B, N, generator=g) * 0.1, torch.randn(B, N, generator=g) * 0.1 + 1.0
        kw = dict(epi=ops.EPI_SPADE, xn=xn.to(DEV).to(torch.bfloat16), mean=mean.to(DEV), rstd=rstd.to(DEV))
        gamma = F.conv2d(_nchw(xin), w.double(), bg_.double(), padding=1)
        beta = F.conv2d(_nchw(xin), wb.double(), bb_.double(), padding=1)
        want = _nhwc((_nchw(xn) - mean.double()[:, :, None, None]) * rstd.double()[:, :, None, None] * (1 + gamma) + beta)
    else:
        bias = 0.1 * torch.randn(N, generator=g)
        sp = _spec_dev(packing.pack_conv(w, bias, stride=1))
        conv = F.conv2d(_nchw(xin), w.double(), bias.double(), padding=1)
        if kind == "res":
            res = rnd(B, H, W, N)
            kw = dict(epi=ops.EPI_RESIDUAL, res=res.to(DEV).to(torch.bfloat16))
            want = _nhwc(conv + _nchw(res))
        else:
            kw = dict(act=act)
            want = _nhwc(F.relu(conv) if act == ops.ACT_RELU else conv)
    x0 = x0c.to(DEV).to(torch.bfloat16)
    x1 = None if x1c is None else x1c.to(DEV).to(torch.bfloat16)
    return x0, x1, sp, kw, want, (B, H, W, N)


def _check(name, x0, x1, sp, kw, want, yshape, batch_invariance=True, max_rel=MAX_REL):
    got, kinds = _launch("bf16_winograd", x0, sp, yshape, x1=x1, **kw)
    base, kinds16 = _launch("bf16", x0, sp, yshape, x1=x1, **kw)
    assert torch.isfinite(got).all(), (name, "non-finite output: an element was not written")
    wmax = want.abs().max().item()
    m = {"max_rel": (got.float().cpu().double() - want).abs().max().item() / wmax, "rel_l2": _rel_l2(got, want), "rel_l2_bf16": _rel_l2(base, want)}
    m["ratio"] = m["rel_l2"] / m["rel_l2_bf16"]
    print(name, m)
    assert max_rel is None or m["max_rel"] <= max_rel, (name, m)
    assert m["ratio"] <= RATIO, (name, m)
    assert not torch.equal(got, base), (name, "the new mode produced the bf16-mode kernel's bits: the Winograd kernel did not run")
    assert kinds == ["bf16_winograd"] and kinds16 == ["bf16"], (name, kinds, kinds16)
    if batch_invariance:
        kw1 = {k: (v[-1:].contiguous() if torch.is_tensor(v) else v) for k, v in kw.items()}
        alone, _ = _launch("bf16_winograd", x0[-1:].contiguous(), sp, (1,) + tuple(yshape[1:]), x1=None if x1 is None else x1[-1:].contiguous(), **kw1)
        assert torch.equal(alone, got[-1:]), (name, "the last frame alone differs from that frame in its batch")
    return m


CASES = [
    ("ragged relu", 2, 20, 36, 64, 0, 128, "conv"),
    ("odd sizes", 1, 17, 31, 128, 0, 64, "conv"),
    ("tiny one partial block", 1, 3, 5, 64, 0, 64, "conv"),
    ("deep", 3, 16, 16, 256, 0, 256, "conv"),
    ("concat", 1, 24, 24, 128, 256, 256, "conv"),
    ("residual", 2, 8, 16, 256, 0, 256, "res"),
    ("spade 64 channels", 2, 16, 16, 128, 0, 64, "spade"),
    ("spade 256 channels", 1, 16, 16, 128, 0, 256, "spade"),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0].replace(" ", "_") for c in CASES])
def test_matrix(case):
    name, B, H, W, C0, C1, N, kind = case
    _check(name, *_build(B, H, W, C0, C1, N, kind, 7000 + CASES.index(case)))


@pytest.mark.parametrize("act", [ops.ACT_NONE, ops.ACT_TANH, ops.ACT_SIGMOID], ids=["none", "tanh", "sigmoid"])
def test_activations(act):
    """The run-time activation codes of the epilogue (the matrix runs ReLU) against the same function in fp64."""
    x0, x1, sp, kw, want, yshape = _build(1, 9, 13, 64, 0, 64, "conv", 7100 + act, act=ops.ACT_NONE)
    want = {ops.ACT_NONE: want, ops.ACT_TANH: want.tanh(), ops.ACT_SIGMOID: want.sigmoid()}[act]
    _check(f"act {act}", x0, x1, sp, dict(act=act), want, yshape)


def test_adversarial():
    """gpu_checks.ADV_KINDS at 2 x 32 x 32, 256 -> 256: the same ratio bound on offset / ill-scaled / heavy-tailed operands."""
    ratios = {}
    for i, kind in enumerate(ADV_KINDS):
        ops_ = _adversarial_operands(kind, 256, (256, 256, 3, 3), (2, 32, 32, 256), 7200 + i)
        m = _check("adv " + kind, *_build(2, 32, 32, 256, 0, 256, "conv", 7300 + i, act=ops.ACT_NONE, operands=ops_), batch_invariance=False, max_rel=None)
        ratios[kind] = round(m["ratio"], 3)
    print("bf16_winograd adversarial ratios", ratios)


def test_determinism():
    """The clip's launch geometry scaled down, 4 x 96 x 96 x 128 -> 128: 288 blocks on 256 compute units, so some persistent workgroups walk two blocks -
    three launches, bitwise equal results.  A plain repeat."""
    x0, x1, sp, kw, want, yshape = _build(4, 96, 96, 128, 0, 128, "conv", 7400)
    ys = [_launch("bf16_winograd", x0, sp, yshape, **kw)[0] for _ in range(3)]
    assert torch.isfinite(ys[0]).all()
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])
    assert (ys[0].float().cpu().double() - want).abs().max().item() <= MAX_REL * want.abs().max().item()


def test_ineligible_launches_unchanged():
    """1x1, strided 3x3 and a transposed convolution's parity launch: in the new mode bit for bit the "bf16"-mode result, hook kind "bf16"."""
    g = torch.Generator().manual_seed(7500)
    rnd = lambda *sh, sc=1.0: r16(torch.randn(*sh, generator=g) * sc)                    # noqa: E731
    x = rnd(2, 16, 16, 64).to(DEV).to(torch.bfloat16)
    launches = [("1x1", _spec_dev(packing.pack_conv(rnd(64, 64, 1, 1, sc=0.1), 0.1 * torch.randn(64, generator=g), stride=1)), (2, 16, 16, 64)),
                ("3x3 s2", _spec_dev(packing.pack_conv(rnd(128, 64, 3, 3, sc=0.04), 0.1 * torch.randn(128, generator=g), stride=2)), (2, 8, 8, 128)),
                ("convT parity", _spec_dev(packing.pack_conv_transpose(rnd(64, 64, 4, 4, sc=0.06), 0.1 * torch.randn(64, generator=g))[3]), (2, 32, 32, 64))]
    for name, sp, yshape in launches:
        a, ka = _launch("bf16_winograd", x, sp, yshape, act=ops.ACT_RELU)
        b, kb = _launch("bf16", x, sp, yshape, act=ops.ACT_RELU)
        mask = torch.isfinite(b)                      # a parity launch writes one pixel in four
        assert mask.any() and torch.equal(torch.isfinite(a), mask), name
        assert torch.equal(a[mask], b[mask]), (name, "an ineligible launch changed in the new mode")
        assert ka == ["bf16"] and kb == ["bf16"], (name, ka, kb)


def test_host_contract():
    """Cin = 96, N = 32 and fp32 tensors are refused with hipErrorInvalidValue before any launch: the output stays NaN."""
    lib = _lib.lib()
    dummy = torch.zeros(1 << 20, device=DEV, dtype=torch.bfloat16)

    def refused(cin, n, dt):
        x = torch.zeros(1, 8, 8, cin, device=DEV, dtype=dt)
        y = torch.full((1, 8, 8, n), float("nan"), device=DEV, dtype=dt)
        sp = _spec_dev(packing.pack_conv(torch.zeros(n, cin, 3, 3), torch.zeros(n), stride=1))
        a = ops.conv_args(x, sp, y)
        a.w = dummy.data_ptr()
        for i, (dy, dx) in enumerate(ops._WINO_TAPS):
            a.dy[i], a.dx[i] = dy, dx
        err = lib.lwg_conv2d_winograd_bf16(a, None)
        torch.cuda.synchronize()
        return err, bool(torch.isnan(y).all())
    assert refused(96, 64, torch.bfloat16) == (1, True)
    assert refused(64, 32, torch.bfloat16) == (1, True)
    assert refused(64, 64, torch.float32) == (1, True)
    # the same description inside the contract is taken (the refusals above are not an artefact of the hand-built argument block)
    x = torch.zeros(1, 8, 8, 64, device=DEV, dtype=torch.bfloat16)
    y = torch.full((1, 8, 8, 64), float("nan"), device=DEV, dtype=torch.bfloat16)
    a = ops.conv_args(x, _spec_dev(packing.pack_conv(torch.zeros(64, 64, 3, 3), torch.zeros(64), stride=1)), y)
    a.w = dummy.data_ptr()
    for i, (dy, dx) in enumerate(ops._WINO_TAPS):
        a.dy[i], a.dx[i] = dy, dx
    assert lib.lwg_conv2d_winograd_bf16(a, None) == 0
    torch.cuda.synchronize()
    assert (y == 0).all()


def test_pipeline():
    """The whole per-frame path at 256 x 256 (check_split_products' case): >= 40 dB PSNR against the fp32 path, frames that differ from
    "bf16" mode's, and nothing left behind after switching back."""
    case = pu.build_case(image_size=256, num_filters=[64, 128, 256], n_res=6, bg_filters=[64, 128, 128, 256], n_frames=2, ns=2)
    im = pu.make_imitator(case, frame_batch=2)
    prev = im.generator.conv_precision
    ref = pu.run_hip(case, imitator=im).clone()
    frames = {}
    for mode in ("bf16", "bf16_winograd"):
        im.generator.conv_precision = mode
        im.set_source(case.src_smpl, case.uv_img, case.bg_img, src_img=case.src_img)
        frames[mode] = pu.run_hip(case, imitator=im).clone()
    im.generator.conv_precision = prev
    im.set_source(case.src_smpl, case.uv_img, case.bg_img, src_img=case.src_img)
    again = pu.run_hip(case, imitator=im)
    torch.cuda.synchronize()
    psnr = {mode: min(_psnr(frames[mode][t], ref[t]) for t in range(ref.shape[0])) for mode in frames}
    print("bf16_winograd pipeline 256: PSNR vs the fp32 path", psnr, "dB lost against bf16 mode:", psnr["bf16"] - psnr["bf16_winograd"])
    assert torch.isfinite(frames["bf16_winograd"]).all()
    assert psnr["bf16_winograd"] >= 40.0, psnr
    assert not torch.equal(frames["bf16_winograd"], frames["bf16"]), "the new mode rendered bf16 mode's frames bit for bit"
    assert torch.equal(again, ref), "frames after switching back differ from the first fp32-path run: the mode left something behind"


@pytest.mark.parametrize("shape", [(1, 17, 31, 128, 64), (2, 16, 16, 256, 128)], ids=["17x31_128_64", "16x16_256_128"])
def test_kernel_matches_emulation(shape):
    """The kernel against tests/bf16wino_emu.emulate_winograd, the CPU emulation of its documented rounding points, on the same operands.  The two
    differ only in the order of the fp32 accumulation: before the final rounding that is at most 16 Cin 2^-24 = 1.2e-4 .. 2.4e-4 of the accumulated
    magnitude (typically its square root), well under half a bf16 ulp (2^-9), so an output is either bit-equal or one bf16 ulp (2^-7 relative, plus
    the accumulation bound near zero) away, and only the few elements whose fp32 value lies that close to a rounding boundary differ at all: at most
    5 % here.  A kernel that rounds V, U or the output at another point differs in about half of its elements."""
    from tests.bf16wino_emu import emulate_winograd
    B, H, W, Cin, N = shape
    g = torch.Generator().manual_seed(7600 + Cin)
    x = r16(torch.randn(B, H, W, Cin, generator=g))
    w = torch.randn(N, Cin, 3, 3, generator=g) * (Cin * 9) ** -0.5
    sp = _spec_dev(packing.pack_conv(w, None, stride=1))
    got, kinds = _launch("bf16_winograd", x.to(DEV).to(torch.bfloat16), sp, (B, H, W, N), act=ops.ACT_NONE)
    emu = emulate_winograd(x, w)
    got = got.float().cpu()
    d = (got - emu).abs()
    differing = (d > 0).float().mean().item()
    print("kernel vs emulation", shape, {"differing": differing, "max_abs": d.max().item(), "emu_max": emu.abs().max().item()})
    assert kinds == ["bf16_winograd"] and torch.isfinite(got).all()
    assert (d <= 2.0 ** -7 * emu.abs() + 2.4e-4 * emu.abs().max()).all(), d.max().item()
    assert differing <= 0.05, differing
