"""The bf16 convolution engine on exact inputs at every tile seam: the five kernels of csrc/conv_igemm_bf16.hip and lwg_conv2d_winograd_bf16 against
torch's conv2d / conv_transpose2d on the CPU, bit for bit (tests/bf16conv_cases.py: operands on which no intermediate of the kernels rounds in any
summation order, and references that are bf16 frames - asserted there on the reference).  Every comparison is ``torch.equal`` over every element of a
NaN-prefilled output; no tolerance appears in this file.  Every case asserts the entry point it ran (ops.conv2d_route / conv_transpose2d_route and
CONV_HOOK's kind) and, through ``bf16_form`` with the device's CU count, the tile form its section is about: a changed threshold fails the test
instead of turning it into a test of another kernel.  The shapes whose form depends on the CU count are computed from it.

Kernel form -> the tests that reach it (each asserts the set of forms its cases took):
  lwg_conv_bf16_hr2_kernel<3,3,2> / <3,3,1>   test_hr2_size_cross[64] / [128] (the 7 x 7 size cross), test_hr2_chunks_concat_widths_epilogues_slices
                                              (1..6 chunks, three concats, N 64..256, residual, SPADE YC 64 / 128, 16 sentinel channels), ties, impulses
  lwg_conv_bf16_hr2_kernel<2,2,1|2>           test_hr2_parity_launches (Cin 256 and 192: omul = 2, the four parities through ops.conv_transpose2d),
                                              test_up4_fused_transposed_conv (its BF16_UP4 = False half)
  lwg_conv_bf16_hr2_kernel<3,3,1,ACC>         test_hr2_accumulator_frame (dense family, outputs beyond 256, fp32 frame in hrl_acc_offset's order)
  lwg_conv_bf16_up4_kernel<1|2,1|2>           test_up4_fused_transposed_conv (also bitwise equal to the four parity launches)
  lwg_conv_bf16_kernel<4,1,1,2>, <2,2,2,2>    test_general_kernel_small_forms (stride 2, 1 x 1 with N != Cin, concat, forced SPADE form, B = 2),
                                              test_general_kernel_on_the_lds_route (BF16_HR = BF16_PW = False: 3 x 3 plain / residual / SPADE, parities)
  lwg_conv_bf16_kernel<2,4,4,2>               test_general_kernel_cu_dependent_forms[0] / [1] (M = 256 CUs + 37); [2]: <2,2,2,2> on a plain epilogue
  lwg_conv_bf16_pw_kernel<1,2,2|2,4,2|4,8,2>  test_pointwise_small; test_pointwise_persistent_loop[C] (M = (4 CUs + 1) BM + 5: three tiles per workgroup)
  lwg_conv_c8_bf16_kernel                     test_first_layer_small (1, 9 and a hand-built 10 taps, strides 1 and 2), test_first_layer_second_pass
                                              (M = 2048 * 256 + 257 as 245 x 2141, and 727 x 727 = 2048 * 256 + 4241)
  lwg_conv_winograd_bf16_kernel               test_winograd_size_cross, test_winograd_chunks_concat_widths_epilogues_slices
Not here: a coded impulse and a tie case for the Winograd kernel (G w G^T of a coded weight, and B^T d B of the tie inputs, are not bf16 values);
tanh and sigmoid (not exact)."""
import contextlib

import pytest
import torch

from ipercore_amd import ops
from ipercore_amd.networks import packing
from tests import bf16conv_cases as bc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
ACT = {"none": ops.ACT_NONE, "relu": ops.ACT_RELU}
EPI = {"plain": ops.EPI_NONE, "res": ops.EPI_RESIDUAL, "spade": ops.EPI_SPADE}


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


class _Hook:
    def __init__(self):
        self.kinds = []

    def __call__(self, begin, M, spec, epi, info):
        if not begin:
            self.kinds.append(info["kind"])


@contextlib.contextmanager
def _route_of(case):
    """The lab switches and the precision mode of a case's route, and a CONV_HOOK that records what ran; everything restored on exit."""
    saved = (ops.BF16_HR, ops.BF16_PW, ops.BF16_C8, ops.BF16_UP4, ops.CONV_HOOK)
    hook = _Hook()
    try:
        ops.BF16_HR = ops.BF16_PW = case.route != "lds"
        ops.BF16_C8 = True
        ops.BF16_UP4 = case.route != "parity"
        ops.CONV_HOOK = hook
        with ops.conv_precision("bf16_winograd" if case.route == "wino" else "bf16"):
            yield hook
    finally:
        ops.BF16_HR, ops.BF16_PW, ops.BF16_C8, ops.BF16_UP4, ops.CONV_HOOK = saved


def _specs(case, o, dev=DEV):
    """The packed convolution(s) of a case on the device (a transposed convolution: its four parity specs)."""
    if case.kind == "convT":
        return [packing.spec_to(s, dev) for s in packing.pack_conv_transpose(o["w"], o["bias"])]
    if case.epi == "spade":
        return packing.spec_to(packing.pack_spade_gamma_beta(o["wg"], o["bg"], o["wb"], o["bb"]), dev)
    if case.k == 10:            # packing has no 10-tap convolution: the GEMM panel by hand, K order tap * 8 + c (the small-Cin order)
        taps = bc.taps_of(case)
        wk = torch.stack([o["w"][:, :, dy + 1, dx + 2].t() for dy, dx in taps]).reshape(len(taps) * 8, case.N)
        return packing.spec_to(ops.ConvSpec(packing._panel(wk), o["bias"], case.N, 8, taps, stride=case.stride), dev)
    return packing.spec_to(packing.pack_conv(o["w"], o["bias"], stride=case.stride, pad=0 if case.k == 1 else 1), dev)


def _framed(case, t, dtype=BF, dev=DEV):
    """An output-shaped operand (the residual) laid out as the output is: in the channel slice of a frame of N + pad channels."""
    if not case.pad:
        return t.to(dev, dtype)
    full = torch.zeros(t.shape[:3] + (t.shape[3] + case.pad,), dtype=dtype, device=dev)
    full[..., 8:8 + t.shape[3]] = t.to(dev, dtype)
    return full


def _launch(case, cus, fused=True):
    """Run the case on the device -> the output frame (bf16, N + pad channels, NaN-prefilled), having asserted its entry point and its form."""
    o = bc.operands(case)
    form = bc.bf16_form(case._replace(route="parity") if not fused else case, cus)
    xdt = torch.float32 if case.kind == "first" else BF
    x0 = o["x0"].to(DEV, xdt)
    x1 = None if o["x1"] is None else o["x1"].to(DEV, xdt)
    oh, ow = bc.out_hw(case)
    ycoff = 8 if case.pad else 0
    y = torch.full((case.B, oh, ow, bc.out_channels(case) + case.pad), float("nan"), dtype=BF, device=DEV)
    sp = _specs(case, o)
    with _route_of(case._replace(route="parity") if not fused else case) as hook:
        if case.kind == "convT":
            route = ops.conv_transpose2d_route(x0, sp, y, ACT[case.act])
            if form.entry == "lwg_conv_transpose4_nhwc_bf16":
                assert route.entry == form.entry and route.kind == "up4", (case.name, route)
                if case.pad:        # conv_transpose2d writes whole tensors: the sliced launch through the same argument block and panel
                    a = ops.conv_args(x0, sp[0], y, act=ACT[case.act], ycoff=ycoff)
                    ops._fused_transpose_launch(a, sp[0], ops._w16up(sp), route.entry, route.kind, route.sliced)
                else:
                    ops.conv_transpose2d(x0, sp, y, ACT[case.act])
                assert hook.kinds == ["up4"], (case.name, hook.kinds)
            else:
                assert route.entry is None, (case.name, route)
                for s in sp:
                    r = ops.conv2d_route(x0, s, y, act=ACT[case.act], ycoff=ycoff)
                    assert r.entry == form.entry and r.kind == "bf16", (case.name, r)
                    ops.conv2d(x0, s, y, act=ACT[case.act], ycoff=ycoff)
                assert hook.kinds == ["bf16"] * 4, (case.name, hook.kinds)
        else:
            kw = dict(x1=x1, epi=EPI[case.epi], act=ACT[case.act], ycoff=ycoff)
            if case.epi == "res":
                kw["res"] = _framed(case, o["res"])
            if case.epi == "spade":
                kw.update(xn=o["xn"].to(DEV, BF), mean=o["mean"].to(DEV), rstd=o["rstd"].to(DEV))
            r = ops.conv2d_route(x0, sp, y, **kw)
            assert r.entry == form.entry, (case.name, r, form)
            ops.conv2d(x0, sp, y, **kw)
            assert hook.kinds == [r.kind] and r.kind == {"lwg_conv2d_winograd_bf16": "bf16_winograd", "lwg_conv2d_nhwc_c8_bf16": "direct"}.get(r.entry, "bf16"), \
                (case.name, hook.kinds, r)
    torch.cuda.synchronize()
    return y, form


def _say(case, got, want):
    """Where two frames differ (for the assertion message)."""
    bad = (got != want) | torch.isnan(got)
    idx = bad.nonzero()
    first = [(tuple(int(v) for v in i), float(got[tuple(i)]), float(want[tuple(i)])) for i in idx[:6]]
    chans = sorted({int(i[3]) for i in idx})
    return "%s: %d of %d outputs differ; pixels (b, y, x) %s ...; channels %s ...; first (index, got, want): %s" % (
        case.name, int(bad.sum()), bad.numel(), sorted({tuple(int(v) for v in i[:3]) for i in idx})[:8], chans[:8], first)


def _check(case, cus, ref_dtype=torch.float64, fused=True):
    y, form = _launch(case, cus, fused)
    want = bc.expected_bf16(case, ref_dtype)
    n = bc.out_channels(case)
    got = y.cpu()
    if case.pad:
        bits = got.view(torch.int16)
        nan = torch.full((1,), float("nan"), dtype=BF).view(torch.int16).item()
        assert bool((bits[..., :8] == nan).all()) and bool((bits[..., 8 + n:] == nan).all()), case.name + ": a sentinel channel outside the slice was written"
        got = got[..., 8:8 + n]
    assert got.shape == want.shape, (case.name, got.shape, want.shape)
    assert torch.equal(got.float(), want.float()), _say(case, got.float(), want.float())
    return y, form


def _run(cases, cus, kernels, ref_dtype=torch.float64):
    seen = set()
    for case in cases:
        seen.add(_check(case, cus, ref_dtype)[1].kernel)
    assert seen == set(kernels), seen


# ------------------------------------------------------------------------------------------------------------------------------ 1. hr2
@pytest.mark.parametrize("N", (64, 128))
def test_hr2_size_cross(N):
    _run(bc.hr2_cross(N), _cus(), {"lwg_conv_bf16_hr2_kernel<3,3,%d>" % (2 if N == 64 else 1)})


def test_hr2_chunks_concat_widths_epilogues_slices():
    cases = bc.hr2_axes()
    _run(cases, _cus(), {"lwg_conv_bf16_hr2_kernel<3,3,1>", "lwg_conv_bf16_hr2_kernel<3,3,2>"})
    assert {bc.bf16_form(c, _cus()).info["chunks"] for c in cases} == {1, 2, 3, 4, 5, 6}


def test_hr2_parity_launches():
    _run(bc.hr2_parity(), _cus(), {"lwg_conv_bf16_hr2_kernel<2,2,1>", "lwg_conv_bf16_hr2_kernel<2,2,2>"})


def test_hr2_accumulator_frame():
    """lwg_conv2d_nhwc_bf16_hr_acc: the fp32 accumulators (no bias, no rounding) are the convolution itself, in the frame's documented order - the
    plain panel's columns, each 32-column tile stored [khalf][r] (bc.acc_frame_columns)."""
    (case,) = bc.hr2_acc()
    assert bc.bf16_form(case, _cus()).entry == "lwg_conv2d_nhwc_bf16_hr_acc"
    o = bc.operands(case)
    sp = _specs(case, o)
    got = ops.conv2d_acc_frame(o["x0"].to(DEV, BF), sp, spade=False)
    torch.cuda.synchronize()
    want = bc.reference(case).float()[..., bc.acc_frame_columns(case.N)].contiguous()
    assert float(want.abs().max()) > 256 and got.dtype == torch.float32
    assert torch.equal(got.cpu(), want), _say(case, got.cpu(), want)


# ------------------------------------------------------------------------------------------------------------------------------ 2. up4
def test_up4_fused_transposed_conv():
    cus = _cus()
    seen = set()
    for case in bc.up4_cases():
        y, form = _check(case, cus)
        seen.add(form.kernel)
        y4, form4 = _check(case, cus, fused=False)               # the four parity launches (BF16_UP4 = False): the same bits
        assert form4.entry == "lwg_conv2d_nhwc_bf16_hr" and torch.equal(y.view(torch.int16), y4.view(torch.int16)), case.name
    assert ops.BF16_UP4 is True
    assert seen == {"lwg_conv_bf16_up4_kernel<%d,%d>" % (n, w) for n in (1, 2) for w in (1, 2)}


# ------------------------------------------------------------------------------------------------------------------------------ 3. general
def test_general_kernel_small_forms():
    _run(bc.general_small(), _cus(), {"lwg_conv_bf16_kernel<4,1,1,2>", "lwg_conv_bf16_kernel<2,2,2,2>"})


def test_general_kernel_on_the_lds_route():
    _run(bc.general_lds_route(), _cus(), {"lwg_conv_bf16_kernel<4,1,1,2>", "lwg_conv_bf16_kernel<2,2,2,2>"})
    assert (ops.BF16_HR, ops.BF16_PW) == (True, True)


@pytest.mark.parametrize("which", (0, 1, 2))
def test_general_kernel_cu_dependent_forms(which):
    """The 8-wave 256 x 256 form (one tile per CU and a ragged one) and the 128 x 128 form on a plain epilogue (two tiles per CU)."""
    cus = _cus()
    case = bc.general_big(cus)[which]
    kernel = "lwg_conv_bf16_kernel<2,4,4,2>" if which < 2 else "lwg_conv_bf16_kernel<2,2,2,2>"
    _run([case], cus, {kernel}, torch.float32)
    f = bc.bf16_form(case, cus)
    assert f.info["tiles_m"] == (cus + 1 if which < 2 else 2 * cus + 1)


# ------------------------------------------------------------------------------------------------------------------------------ 4. pointwise
def test_pointwise_small():
    cases = bc.pw_small()
    _run(cases, _cus(), {"lwg_conv_bf16_pw_kernel<1,2,2>", "lwg_conv_bf16_pw_kernel<2,4,2>", "lwg_conv_bf16_pw_kernel<4,8,2>"})


@pytest.mark.parametrize("C", sorted(bc.PW_BM))
def test_pointwise_persistent_loop(C):
    cus = _cus()
    case = bc.pw_persistent(cus, C)
    f = bc.bf16_form(case, cus)
    assert f.info["walk"] == 3 and f.info["tiles"] > 2 * f.info["slots"] and bc.rows(case) % f.tile[0] == 5
    _run([case], cus, {f.kernel}, torch.float32)


# ------------------------------------------------------------------------------------------------------------------------------ 5. first layer
def test_first_layer_small():
    _run(bc.c8_small(), _cus(), {"lwg_conv_c8_bf16_kernel"})


@pytest.mark.parametrize("which", (0, 1))
def test_first_layer_second_pass(which):
    case = bc.c8_second_pass()[which]
    assert bc.bf16_form(case, _cus()).info == {"grid": 2048, "passes": 2}
    _run([case], _cus(), {"lwg_conv_c8_bf16_kernel"}, torch.float32)


# ------------------------------------------------------------------------------------------------------------------------------ 6. Winograd
def test_winograd_size_cross():
    _run(bc.wino_cross(), _cus(), {"lwg_conv_winograd_bf16_kernel"})


def test_winograd_chunks_concat_widths_epilogues_slices():
    _run(bc.wino_axes(), _cus(), {"lwg_conv_winograd_bf16_kernel"})


# ------------------------------------------------------------------------------------------------------------------------------ ties, impulses
def test_final_rounding_is_to_nearest_even():
    """257, 259, -257, -259, 385 -> 256, 260, -256, -260, 384 on every store path: store_dt's packed path, the SPADE uintx2 path, the first layer's."""
    cus = _cus()
    for case in bc.tie_cases():
        y, _ = _check(case, cus)
        picks = tuple(float(y[0, cy, cx, bc.TIE_ROW + (t < 0)]) for (cy, cx), t in zip(bc.TIE_AT, bc.TIE_TARGETS))
        assert picks == tuple(float(v) for v in bc.TIE_ROUNDED), (case.name, picks)


def test_coded_impulses():
    """One impulse per image on each side of a block corner, a distinct bf16 code per weight: every output is the one weight it should have read."""
    cus = _cus()
    kernels = set()
    for case in bc.impulse_cases():
        try:
            kernels.add(_check(case, cus)[1].kernel.split("<")[0])
        except AssertionError as e:          # name the weights the wrong outputs did read
            y, _ = _launch(case, cus)
            want = bc.expected_bf16(case).float()
            bad = (y.cpu().float() != want).nonzero()[:4]
            read = [(tuple(int(v) for v in i), bc.impulse_decode(case, float(y[tuple(i)]))[:3], bc.impulse_decode(case, float(want[tuple(i)]))[:3]) for i in bad]
            raise AssertionError("%s\n(index, weight read, weight expected): %s" % (e, read))
    assert kernels == {"lwg_conv_bf16_hr2_kernel", "lwg_conv_bf16_up4_kernel", "lwg_conv_bf16_kernel", "lwg_conv_bf16_pw_kernel", "lwg_conv_c8_bf16_kernel"}
