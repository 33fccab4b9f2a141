"""The loss / optimizer kernels of the training step (csrc/train_ops.hip) one by one on the cases of tests/train_ops_cases.py: the fused Adam update
(device-t and host-t forms), the activation backward, the per-channel PReLU, MaxPool2d(2, 2), the device-side head crop and the panel pack / unpack.
References, bounds and their derivations live in tests/train_ops_cases.py; tests/test_train_ops_primitives_cpu.py shows on the CPU that every bound
holds with slack for an fp32 restatement of the kernel and refuses the planted errors.

Kernels that write an output buffer are called through the C ABI on a NaN-filled buffer (an element nobody wrote shows up), and their ops.* wrapper must
return the same bits; in-place kernels (Adam, unpack_wgrad, the crop's backward into a zeroed dx) go through ops.*.  Every test prints its metrics -
for the toleranced comparisons the worst observed |error| / bound - as one JSON line."""
import ctypes
import json

import pytest
import torch

from ipercore_amd import _lib, ops
from tests import emu_ops
from tests import train_ops_cases as tc
from tests.gpu_checks import DEV

pytestmark = pytest.mark.gpu


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _report(what, metrics):
    print("train_ops_primitives " + json.dumps({what: metrics}))


def _same_bits(got, want):
    return torch.equal(tc.bits(got.cpu()), tc.bits(want))


# ------------------------------------------------------------------------------------------------------------------------------------ Adam
def _adam_one_step(state, g, t_dev, t):
    """ops.adam_step_dev on ``state`` (p, m, v on the device, updated in place) and ops.adam_step at the same t on a copy of the state before the step,
    each against the float64 step from that state -> (ratios of the device form, ratios of the host form, the two forms agree bit for bit)."""
    hyp = (tc.ADAM_LR,) + tc.ADAM_BETAS + (tc.ADAM_EPS,)
    p, m, v = state
    before = [a.clone() for a in state]
    host = [a.clone() for a in state]
    ops.adam_step_dev(p, g, m, v, *hyp, t_dev)
    ops.adam_step(host[0], g, host[1], host[2], *hyp, t)
    torch.cuda.synchronize()
    assert int(t_dev.item()) == t, f"t_dev is {int(t_dev.item())} after the step that should have made it {t}"
    ref = tc.adam_ref64(before[0].cpu(), g.cpu(), before[1].cpu(), before[2].cpu(), t)
    rd = tc.adam_ratios(p.cpu(), m.cpu(), v.cpu(), ref)
    same = all(torch.equal(a, b) for a, b in zip(state, host))
    rh = rd if same else tc.adam_ratios(host[0].cpu(), host[1].cpu(), host[2].cpu(), ref)
    return rd, rh, same


def _adam_assert(rd, rh, what):
    for form, r in (("device-t", rd), ("host-t", rh)):
        assert max(r.values()) <= 1.0, f"adam {what} {form}: worst |error| / bound {r}"


@pytest.mark.parametrize("n", tc.ADAM_SIZES)
def test_adam_six_steps_from_t0(n):
    """t_dev = 0, m = v = 0, six steps, each against one float64 step from the device's own state before it (so the fp32 rounding of carried state
    does not accumulate), with the hyperparameters as the C ABI rounds them (exact Python betas would differ by 6.4e-6 of the update at t = 1 with
    carried state: the ABI's, not the kernel's).  The device-t and host-t forms agree bit for bit at every t <= 6; t_dev advances by exactly 1."""
    p, g0, m, v = tc.adam_inputs(n, True)
    state = [a.to(DEV) for a in (p, m, v)]
    t_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    worst = {}
    for s in range(tc.ADAM_FIRST_STEPS):
        g = tc.adam_step_gradient(g0, s).to(DEV)
        rd, rh, same = _adam_one_step(state, g, t_dev, s + 1)
        assert same, f"adam n={n}: the device-t and host-t forms differ at t = {s + 1}"
        _adam_assert(rd, rh, f"n={n} t={s + 1}")
        worst = {k: max(worst.get(k, 0.0), r) for k, r in rd.items()}
    _report(f"adam_n{n}_t1to6", {"worst_error_over_bound": worst, "device_equals_host": True})


@pytest.mark.parametrize("preset", tc.ADAM_PRESETS)
@pytest.mark.parametrize("n", tc.ADAM_SIZES)
def test_adam_one_step_at_large_t(n, preset):
    """t_dev preset to 999 / 99 999, carried m and v, one step.  Both forms meet the bounds, and - since both run lwg_adam_kernel, which forms the
    bias corrections with the device's powf - agree bit for bit here too."""
    p, g, m, v = tc.adam_inputs(n, False, preset)
    state = [a.to(DEV) for a in (p, m, v)]
    t_dev = torch.full((1,), preset, dtype=torch.int32, device=DEV)
    rd, rh, same = _adam_one_step(state, g.to(DEV), t_dev, preset + 1)
    _report(f"adam_n{n}_t{preset + 1}", {"worst_error_over_bound_device_t": rd, "worst_error_over_bound_host_t": rh, "device_equals_host": same})
    _adam_assert(rd, rh, f"n={n} t={preset + 1}")
    assert same, f"adam n={n}: the device-t and host-t forms differ at t = {preset + 1}"


# --------------------------------------------------------------------------------------------------------------------- activation backward
@pytest.mark.parametrize("n", tc.ACT_SIZES)
@pytest.mark.parametrize("name", tc.ACT_CODES)
def test_act_bwd(name, n):
    """NONE / RELU / LRELU: the bits of dy, dy * (y > 0), dy * where(y > 0, 1, 0.2f) (at y = +-0: 0 and 0.2 dy, ATen's rule).  TANH / SIGMOID: float64
    dy (1 - y^2) / dy y (1 - y) within 2^-22 |dy|, the planted saturated outputs included."""
    act = tc.ACT_CODES[name]
    dy, y = tc.act_inputs(n, act)
    dyd, yd, out = dy.to(DEV), y.to(DEV), _nan(n)
    _lib.check(_lib.lib().lwg_act_bwd_f32(dyd.data_ptr(), yd.data_ptr(), n, act, out.data_ptr(), ops._stream()), "lwg_act_bwd_f32")
    wrapped = ops.act_bwd(dyd, yd, act)
    torch.cuda.synchronize()
    assert torch.equal(tc.bits(wrapped), tc.bits(out))
    got = out.cpu()
    if act in (tc.ACT_NONE, tc.ACT_RELU, tc.ACT_LRELU):
        assert torch.equal(tc.bits(got), tc.bits(tc.act_bwd_f32(dy, y, act))), f"act_bwd {name} n={n}"
        _report(f"act_bwd_{name}_n{n}", "bitwise")
        return
    ref, bound = tc.act_bwd_ref64(dy, y, act)
    ratio = tc.worst_ratio((got.double() - ref).abs(), bound)
    _report(f"act_bwd_{name}_n{n}", {"worst_error_over_bound": ratio})
    assert ratio <= 1.0, f"act_bwd {name} n={n}: worst |error| / bound {ratio}"


# ----------------------------------------------------------------------------------------------------------------------------------- PReLU
@pytest.mark.parametrize("rows,C", tc.PRELU_CASES)
def test_prelu_forward_residual_and_backward(rows, C):
    """Forward: == the fp32 where(x > 0, x, slope x).  Forward + residual: float64 within 2^-23 (|PReLU(x)| + |res|).  Backward: the bits of the fp32
    where(x > 0, dy, slope dy) - ATen's rule, slope dy at x = +-0, planted in every channel."""
    x, slope, res, dy = tc.prelu_inputs(rows, C)
    L = _lib.lib()
    xd, sd, rd, dyd = (t.to(DEV) for t in (x, slope, res, dy))
    y, yr, dx = _nan(rows, C), _nan(rows, C), _nan(rows, C)
    _lib.check(L.lwg_prelu_f32(xd.data_ptr(), sd.data_ptr(), None, rows, C, y.data_ptr(), ops._stream()), "lwg_prelu_f32")
    _lib.check(L.lwg_prelu_f32(xd.data_ptr(), sd.data_ptr(), rd.data_ptr(), rows, C, yr.data_ptr(), ops._stream()), "lwg_prelu_f32")
    _lib.check(L.lwg_prelu_bwd_f32(xd.data_ptr(), sd.data_ptr(), dyd.data_ptr(), rows, C, dx.data_ptr(), ops._stream()), "lwg_prelu_bwd_f32")
    wrapped = ops.prelu(xd, sd), ops.prelu(xd, sd, rd), ops.prelu_bwd(xd, sd, dyd)
    torch.cuda.synchronize()
    for w, direct in zip(wrapped, (y, yr, dx)):
        assert torch.equal(tc.bits(w), tc.bits(direct))
    assert torch.equal(y.cpu(), tc.prelu_f32(x, slope)), f"prelu ({rows}, {C}) forward"
    ref, bound = tc.prelu_res_ref64(x, slope, res)
    ratio = tc.worst_ratio((yr.cpu().double() - ref).abs(), bound)
    _report(f"prelu_{rows}x{C}", {"residual_worst_error_over_bound": ratio, "forward": "equal", "backward": "bitwise"})
    assert ratio <= 1.0, f"prelu ({rows}, {C}) forward + residual: worst |error| / bound {ratio}"
    assert torch.equal(tc.bits(dx.cpu()), tc.bits(tc.prelu_bwd_f32(x, slope, dy))), f"prelu ({rows}, {C}) backward"


# --------------------------------------------------------------------------------------------------------------------------------- MaxPool
POOL_RUNS = [(s, "ties") for s in tc.POOL_CASES] + [(tc.POOL_CASES[2], k) for k in tc.POOL_SPECIAL] + [(tc.POOL_CASES[3], k) for k in tc.POOL_SPECIAL]


@pytest.mark.parametrize("shape,kind", POOL_RUNS, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_maxpool2_forward_and_backward(shape, kind):
    """F.max_pool2d and its autograd on the CPU, bit for bit: every dx element is one dy or +0.  Values from {-1, 0, 0, 1}: most windows tie; the
    +-0 case: every window ties, the forward returns the bits of its first element and the gradient goes there (-0 == +0); the -inf case: an all
    -inf window gives -inf and routes to (0, 0)."""
    B, H, W, C = shape
    x, dy = tc.pool_inputs(*shape, kind=kind)
    y_ref, dx_ref = tc.pool_reference(x, dy)
    L = _lib.lib()
    xd, dyd = x.to(DEV), dy.to(DEV)
    y, dx = _nan(B, H // 2, W // 2, C), _nan(B, H, W, C)
    _lib.check(L.lwg_maxpool2_fwd_nhwc_f32(xd.data_ptr(), y.data_ptr(), B, H, W, C, ops._stream()), "lwg_maxpool2_fwd_nhwc_f32")
    _lib.check(L.lwg_maxpool2_bwd_nhwc_f32(xd.data_ptr(), dyd.data_ptr(), dx.data_ptr(), B, H, W, C, ops._stream()), "lwg_maxpool2_bwd_nhwc_f32")
    wy, wdx = ops.maxpool2_fwd(xd), ops.maxpool2_bwd(xd, dyd)
    torch.cuda.synchronize()
    assert torch.equal(tc.bits(wy), tc.bits(y)) and torch.equal(tc.bits(wdx), tc.bits(dx))
    what = f"maxpool2 {shape} {kind}"
    assert _same_bits(y, y_ref), what + " forward"
    assert _same_bits(dx, dx_ref), what + " backward"


# ------------------------------------------------------------------------------------------------------------------------------- head crop
@pytest.mark.parametrize("out_hw", tc.CROP_OUT, ids=lambda s: "%dx%d" % s)
def test_crop_resize_forward(out_hw):
    """emu_ops._crop_ref (the reference's slice + F.interpolate(align_corners=True), fp32 on the CPU) within check_face_loss's 2e-6; exact zeros for
    dropped samples in the NaN-filled output; valid exact; the same crops without the valid output."""
    x, box = tc.crop_inputs()
    N, C, H, W = tc.CROP_IMAGE
    OH, OW = out_hw
    ref, valid_ref = emu_ops._crop_ref(x, box, out_hw)
    assert valid_ref.tolist() == [float(v) for v in tc.CROP_VALID]
    L = _lib.lib()
    xd, bd = x.to(DEV), box.to(DEV)
    y, valid, y2 = _nan(N, C, OH, OW), _nan(N), _nan(N, C, OH, OW)
    _lib.check(L.lwg_crop_resize_bilinear_f32(xd.data_ptr(), bd.data_ptr(), y.data_ptr(), valid.data_ptr(), N, C, H, W, OH, OW, ops._stream()),
               "lwg_crop_resize_bilinear_f32")
    _lib.check(L.lwg_crop_resize_bilinear_f32(xd.data_ptr(), bd.data_ptr(), y2.data_ptr(), None, N, C, H, W, OH, OW, ops._stream()),
               "lwg_crop_resize_bilinear_f32")
    wy, wvalid = ops.crop_resize(xd, bd, out_hw)
    wy2, none = ops.crop_resize(xd, bd, out_hw, want_valid=False)
    torch.cuda.synchronize()
    assert none is None and torch.equal(tc.bits(wy), tc.bits(y)) and torch.equal(tc.bits(wy2), tc.bits(y)) and torch.equal(wvalid, valid)
    assert torch.equal(tc.bits(y2), tc.bits(y)), f"crop {out_hw}: the crops differ without the valid output"
    assert torch.equal(valid.cpu(), valid_ref), f"crop {out_hw}: valid {valid.cpu().tolist()}"
    got = y.cpu()
    assert not torch.isnan(got).any(), f"crop {out_hw}: {int(torch.isnan(got).sum())} output elements were never written"
    err = float((got - ref).abs().max())
    _report("crop_forward_%dx%d" % out_hw, {"max_abs_error": err, "tolerance": tc.CROP_FWD_TOL})
    assert err <= tc.CROP_FWD_TOL, f"crop {out_hw}: max |error| {err:.3e}"
    assert (got[valid_ref == 0] == 0).all(), f"crop {out_hw}: a dropped sample is not exactly 0"


@pytest.mark.parametrize("out_hw", tc.CROP_OUT_BWD, ids=lambda s: "%dx%d" % s)
def test_crop_resize_backward(out_hw):
    """emu_ops.crop_resize_bwd within 2e-5 max(1, max |dx_ref| of the sample) per sample; exactly 0 for dropped samples and outside the clamped
    rectangle of kept ones."""
    x, box = tc.crop_inputs()
    N, C, H, W = tc.CROP_IMAGE
    dy = tc.crop_dy(out_hw)
    ref = emu_ops.crop_resize_bwd(dy, box, (H, W))
    got = ops.crop_resize_bwd(dy.to(DEV), box.to(DEV), (H, W))
    torch.cuda.synchronize()
    got = got.cpu()
    assert torch.isfinite(got).all()
    ratio = float(((got - ref).abs() / tc.crop_bwd_tol(ref)).max())
    _report("crop_backward_%dx%d" % out_hw, {"worst_error_over_tolerance": ratio})
    assert ratio <= 1.0, f"crop backward {out_hw}: worst |error| / tolerance {ratio}"
    outside = torch.ones(N, C, H, W, dtype=torch.bool)
    for i, b in enumerate(tc.CROP_BOXES):
        rect = tc.crop_rect(b, H, W)
        if rect is not None:
            x0, y0, cw, ch = rect
            outside[i, :, y0:y0 + ch, x0:x0 + cw] = False
    assert (got[outside] == 0).all(), f"crop backward {out_hw}: gradient outside the crop rectangle or in a dropped sample"


# ------------------------------------------------------------------------------------------------------------------ panel pack and unpack
def _kidx(kidx):
    return (ctypes.c_int * len(kidx))(*kidx)


@pytest.mark.parametrize("case", tc.PANEL_CASES, ids=tc.panel_id)
def test_pack_panel_single_launch_equals_the_emulation(case):
    """lwg_pack_panel_f32 into a NaN-filled panel: emu_ops.pack_panel element for element (the weight holds its own flat index), the zero padding
    of K rows, input channels and output columns written."""
    sh, tr, kidx, cin, cin_pad, nout, n_pad = case
    w = tc.index_weight(sh)
    want = emu_ops.pack_panel(w, tr, kidx, cin, cin_pad, nout, n_pad)
    wd, out = w.to(DEV), _nan(*want.shape)
    _lib.check(_lib.lib().lwg_pack_panel_f32(wd.data_ptr(), sh[0], sh[1], sh[2], sh[3], 1 if tr else 0, _kidx(kidx), len(kidx), cin, cin_pad, nout, n_pad,
                                             out.data_ptr(), ops._stream()), "lwg_pack_panel_f32")
    wrapped = ops.pack_panel(wd, tr, kidx, cin, cin_pad, nout, n_pad)
    torch.cuda.synchronize()
    assert torch.equal(wrapped, out)
    assert torch.equal(out.cpu(), want), f"pack_panel {tc.panel_id(case)}"


def test_pack_panels_one_launch_equals_the_emulation():
    """Every case in ONE descriptor table through ops.PanelCache (weights as views of one flat buffer that trains, as FlatAdam lays them out): the
    registered panels are NaN-filled, then refresh() = lwg_pack_panels_f32 must leave the emulation's panel in each."""
    shapes = list(dict.fromkeys(c[0] for c in tc.PANEL_CASES))
    sizes = [tc.index_weight(sh).numel() for sh in shapes]
    flat = torch.zeros(sum(sizes), device=DEV).requires_grad_(True)
    views, off = {}, 0
    for sh, nel in zip(shapes, sizes):
        views[sh] = flat.detach()[off:off + nel].view(*sh)
        views[sh].copy_(tc.index_weight(sh))
        off += nel
    cache = ops.PanelCache([flat])
    prev, ops.PANEL_CACHE = ops.PANEL_CACHE, cache
    try:
        panels = [ops.pack_panel(views[c[0]], *c[1:]) for c in tc.PANEL_CASES]       # first request: single launches, registered
        assert len(cache.rows) == len(tc.PANEL_CASES)
        for p_ in panels:
            p_.fill_(float("nan"))
        cache.refresh()
    finally:
        ops.PANEL_CACHE = prev
    torch.cuda.synchronize()
    for case, p_ in zip(tc.PANEL_CASES, panels):
        want = emu_ops.pack_panel(tc.index_weight(case[0]), *case[1:])
        assert torch.equal(p_.cpu(), want), f"pack_panels {tc.panel_id(case)}"


@pytest.mark.parametrize("case", tc.UNPACK_CASES, ids=tc.panel_id)
def test_unpack_wgrad_equals_the_emulation_and_keeps_the_sentinel(case):
    """dw prefilled with a sentinel, the tap sets (the four parity sets of a 4x4 transposed kernel) written one after another: after each launch dw is
    the emulation's, so the positions no tap has mapped to yet - and the rows and columns beyond (cin, nout) - still hold the sentinel."""
    sh, tr, tapsets, cin, cin_pad, nout, n_pad = case
    dwks, stages, written = tc.unpack_reference(case)
    dw = torch.full(sh, tc.SENTINEL, device=DEV)
    for j, (kidx, dwk, want) in enumerate(zip(tapsets, dwks, stages)):
        ops.unpack_wgrad(dwk.to(DEV), dw, tr, kidx, cin, cin_pad, nout)
        torch.cuda.synchronize()
        assert torch.equal(dw.cpu(), want), f"unpack_wgrad {tc.panel_id(case)} after tap set {j}"
    assert (dw.cpu()[~written] == tc.SENTINEL).all()
