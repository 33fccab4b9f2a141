"""tests/train_ops_cases.py held against itself, on the CPU: every reference against tests/emu_ops.py, every error bound against a numpy-float32
restatement of the kernel's arithmetic (so each bound is known to hold with slack before a GPU sees it), and against planted errors - the step
count off by one in Adam, >= for > in the PReLU backward, a pool row stride built on H, a head crop without its last block - which the same
assertions as tests/test_gpu_train_ops_primitives.py must refuse."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import emu_ops
from tests import train_ops_cases as tc

SMALL_ADAM = tuple(n for n in tc.ADAM_SIZES if n < 10 ** 6)


# ------------------------------------------------------------------------------------------------------------------------------------ Adam
def test_adam_inputs_are_what_the_cases_promise():
    for n in SMALL_ADAM:
        p, g, m, v = tc.adam_inputs(n, True)
        assert int((g == 0).sum()) == min(8, n // 2) and g[-1] == 0 and not m.any() and not v.any()
        p, g, m, v = tc.adam_inputs(n, False)
        assert m.abs().max() > 0 and v.min() >= 0 and v.max() <= 0.01
    p, g, m, v = tc.adam_inputs(1028, False)
    mag = g[g != 0].abs().log10()
    assert mag.min() < -5.5 and mag.max() > 0.5                    # the scales 1e-6 .. 10 are all there
    assert tc.ADAM_SIZES[-1] == 4 * (8192 * 256 + 1)


@pytest.mark.parametrize("t", tc.ADAM_CPU_TS)
def test_adam_bounds_hold_for_the_fp32_restatement(t):
    worst = {"m": 0.0, "v": 0.0, "p": 0.0}
    for n in SMALL_ADAM:
        p, g, m, v = tc.adam_inputs(n, t == 1, t)
        ref = tc.adam_ref64(p, g, m, v, t)
        pp, mm, vv = tc.adam_f32(p, g, m, v, t)
        for k, r in tc.adam_ratios(pp, mm, vv, ref).items():
            worst[k] = max(worst[k], r)
    print(f"adam t={t}: worst |error| / bound of the fp32 restatement {worst}")
    assert worst["m"] <= 0.75 and worst["v"] <= 0.75 and worst["p"] <= 0.75, worst       # slack: a quarter of each bound is unused


def test_adam_reference_is_torch_optim_adam():
    """The float64 reference (with exact Python hyperparameters) is torch.optim.Adam in float64, step by step."""
    n = 1000
    p, g, m, v = tc.adam_inputs(n, True)
    pr = p.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([pr], lr=tc.ADAM_LR, betas=tc.ADAM_BETAS, eps=tc.ADAM_EPS)
    pc, mc, vc = p.double(), m.double(), v.double()
    for s in range(4):
        gs = tc.adam_step_gradient(g, s)
        pr.grad = gs.double().clone()
        opt.step()
        b1, b2 = tc.ADAM_BETAS
        mc = b1 * mc + (1 - b1) * gs.double()
        vc = b2 * vc + (1 - b2) * gs.double() ** 2
        pc = pc - tc.ADAM_LR / (1 - b1 ** (s + 1)) * mc / ((vc / (1 - b2 ** (s + 1))).sqrt() + tc.ADAM_EPS)
        assert (pc - pr.detach()).abs().max() <= 1e-12
    # the ABI rounds the hyperparameters to fp32: float(np.float32(0.999)) = 0.99900001287, so 1 - b2 is 1.29e-5 smaller than 1e-3.  With carried
    # state at t = 1 (v_old b2 / (1 - b2) dominates the denominator) that moves the update by 6.4e-6 of itself (6.7e-6 with lr and b1; more where
    # m nearly cancels).  At t = 1 the bound's powf term hides that; at t = 1000 it is more than the bound allows - and the ABI's doing, not the
    # kernel's: the reference rounds them the same way
    p, g, m, v = tc.adam_inputs(n, False)
    ref, exact = tc.adam_ref64(p, g, m, v, 1), tc.adam_ref64(p, g, m, v, 1, abi=False)
    upd = (exact["p"] - p.double()).abs()
    moved = ((ref["p"] - exact["p"]).abs() / upd)[upd > 0]
    assert 6e-6 < moved.median() < 7e-6, moved.median()
    ref, exact = tc.adam_ref64(p, g, m, v, 1000), tc.adam_ref64(p, g, m, v, 1000, abi=False)
    assert ((ref["p"] - exact["p"]).abs() / ref["p_bound"]).max() > 2


def test_adam_emulation_agrees_with_the_reference():
    """emu_ops.adam_step (torch fp32 ops, Python hyperparameters) stays within the tolerance gpu_checks.check_train_ops gives it; m and v to 2e-5
    of themselves (1 - b2 as the ABI rounds it is 1.3e-5 off the Python value)."""
    p, g, m, v = tc.adam_inputs(1000, False)
    ref = tc.adam_ref64(p, g, m, v, 7)
    pe, me, ve = p.clone(), m.clone(), v.clone()
    emu_ops.adam_step(pe, g, me, ve, tc.ADAM_LR, *tc.ADAM_BETAS, tc.ADAM_EPS, 7)
    assert (pe.double() - ref["p"]).abs().max() <= 1e-5 * p.abs().max()
    assert ((me.double() - ref["m"]).abs() <= 2e-5 * ref["m"].abs() + 1e-7).all() and ((ve.double() - ref["v"]).abs() <= 2e-5 * ref["v"]).all()


@pytest.mark.parametrize("off", (-1, 1))
def test_adam_bound_refuses_a_step_count_off_by_one_at_t_1000(off):
    """t = 999 or 1001 in place of 1000 changes the update by 2.9e-4 of itself (the sqrt(1 - b2^t) factor).  Not EVERY element with |p| < 4 can
    violate the bound: where m nearly cancels the update is next to 0 and 2.9e-4 of it disappears under the 2^-23 |p| term.  Such an element has
    2.8e-4 |update| <= 2^-23 * 4 + (the r_t term, ~1e-6 |update|-sized), i.e. |update| < 2e-3.  So: every element that does not violate has an
    update under 2e-3, every element with an update over 4e-3 violates, and the violators are 1003 of the 1028 elements (97.6 %) for both signs."""
    p, g, m, v = tc.adam_inputs(1028, False, 1000)
    ref = tc.adam_ref64(p, g, m, v, 1000)
    wrong = tc.adam_ref64(p, g, m, v, 1000 + off)
    upd = (ref["p"] - p.double()).abs()
    rel = ((wrong["p"] - ref["p"]).abs() / upd)[upd > 0]
    assert 2.8e-4 < rel.min() and rel.max() < 3.0e-4, (rel.min(), rel.max())
    sel = p.abs() < 4
    viol = (wrong["p"] - ref["p"]).abs() > ref["p_bound"]
    assert sel.sum() > 1000
    assert viol[sel & (upd > 4e-3)].all()                     # 2.8e-4 * 4e-3 = 1.1e-6 > 2^-23 * 4 + r_t * (update-sized term)
    assert (upd[sel & ~viol] < 2e-3).all(), upd[sel & ~viol].max()
    assert viol[sel].float().mean() > 0.97, (int(viol[sel].sum()), int(sel.sum()))
    assert tc.adam_ratios(wrong["p"], ref["m"], ref["v"], ref)["p"] > 10


def test_adam_bound_refuses_a_missing_bias_correction():
    p, g, m, v = tc.adam_inputs(1028, True)
    ref = tc.adam_ref64(p, g, m, v, 1)
    # no correction at t = 1: the update is lr m / (sqrt(v) + eps) = 0.1 / sqrt(0.001) times too large
    bad = p.double() - tc.adam_abi(tc.ADAM_LR) * ref["m"] / (ref["v"].sqrt() + tc.adam_abi(tc.ADAM_EPS))
    assert tc.adam_ratios(bad, ref["m"], ref["v"], ref)["p"] > 1e3


# --------------------------------------------------------------------------------------------------------------------- activation backward
@pytest.mark.parametrize("name", tc.ACT_CODES)
def test_act_bwd_cases_references_and_bound(name):
    act = tc.ACT_CODES[name]
    for n in (4, 1028):
        dy, y = tc.act_inputs(n, act)
        for val in tc.ACT_PLANTED[act]:
            want = min(16, n // len(tc.ACT_PLANTED[act]))
            hit = (y == val) & (torch.signbit(y) == bool(np.signbit(val)))
            assert int(hit.sum()) >= want, (name, n, val)
        kern, emu = tc.act_bwd_kernel_f32(dy, y, act), emu_ops.act_bwd(dy, y, act)
        if act in (tc.ACT_NONE, tc.ACT_RELU, tc.ACT_LRELU):
            want = tc.act_bwd_f32(dy, y, act)
            assert torch.equal(tc.bits(kern), tc.bits(want)) and torch.equal(emu, want)
            # ATen's rule at y = +-0: ReLU 0, LeakyReLU 0.2 dy
            a = y.clone().requires_grad_(True)
            {tc.ACT_NONE: lambda t: t * 1, tc.ACT_RELU: F.relu, tc.ACT_LRELU: lambda t: F.leaky_relu(t, 0.2)}[act](a).backward(dy)
            assert torch.equal(a.grad, want)
        else:
            ref, bound = tc.act_bwd_ref64(dy, y, act)
            ratio = tc.worst_ratio((kern.double() - ref).abs(), bound)
            print(f"act_bwd {name} n={n}: worst |error| / bound of the fp32 restatement {float(ratio):.3f}")
            assert ratio <= 0.75
            assert ((emu.double() - ref).abs() <= bound).all()
            sat = y.abs() == 1 if act == tc.ACT_TANH else (y == 0) | (y == 1)
            assert sat.any() and (kern[sat] == 0).all()
    # a swapped tanh / sigmoid derivative is refused
    dy, y = tc.act_inputs(1028, tc.ACT_TANH)
    ref, bound = tc.act_bwd_ref64(dy, y, tc.ACT_TANH)
    assert ((tc.act_bwd_kernel_f32(dy, y, tc.ACT_SIGMOID).double() - ref).abs() > bound).any()


# ----------------------------------------------------------------------------------------------------------------------------------- PReLU
@pytest.mark.parametrize("rows,C", tc.PRELU_CASES[:-1] + ((3000, 12),))
def test_prelu_references_follow_aten_and_refuse_the_old_rule(rows, C):
    x, slope, res, dy = tc.prelu_inputs(rows, C)
    assert all(s in slope.tolist() for s in tc.PRELU_SLOPES[:min(5, (C + 1) // 2)])
    zero = x == 0
    assert zero.any(dim=0).all()                                                    # every channel has a zero
    if rows >= 2:
        assert (zero & torch.signbit(x)).any(dim=0).all() and (zero & ~torch.signbit(x)).any(dim=0).all()
    # ATen: forward, and the backward's slope * dy at x = +-0
    xr = x.clone().requires_grad_(True)
    y = F.prelu(xr.t().reshape(1, C, rows), slope)                                  # channels in dimension 1
    y.backward(dy.t().reshape(1, C, rows))
    fwd, bwd = tc.prelu_f32(x, slope), tc.prelu_bwd_f32(x, slope, dy)
    assert torch.equal(y.detach().reshape(C, rows).t(), fwd)
    assert torch.equal(xr.grad, bwd)
    assert torch.equal(emu_ops.prelu(x, slope), fwd) and torch.equal(tc.bits(emu_ops.prelu_bwd(x, slope, dy)), tc.bits(bwd))
    # the planted error - the rule of lwg_prelu_kernel<true> and emu_ops.prelu_bwd before they followed ATen - differs exactly at the zeros
    # whose channel's slope is not 1 (N(0,1) dy: no zero gradient)
    old = tc.prelu_bwd_f32_ge(x, slope, dy)
    assert not torch.equal(old, bwd)
    assert torch.equal(old != bwd, zero & (slope != 1))
    # forward: value-identical under both rules (x = +-0 gives +-0 either way)
    assert torch.equal(torch.where(x >= 0, x, slope * x), fwd)
    # with the residual: two roundings in fp32 - 2^-24 |PReLU(x)| + 2^-24 |sum| - which the bound covers exactly: no slack where the residual is
    # small next to the PReLU term, half of it unused where the kernel fuses the two
    ref, bound = tc.prelu_res_ref64(x, slope, res)
    two = (fwd + res).double()
    ratio = tc.worst_ratio((two - ref).abs(), bound)
    print(f"prelu + residual ({rows}, {C}): worst |error| / bound of the fp32 restatement {ratio:.3f}")
    assert ratio <= 1.0
    assert torch.equal(emu_ops.prelu(x, slope, res), fwd + res)


def test_prelu_large_case_defeats_a_channel_from_the_loop_counter():
    rows, C = tc.PRELU_CASES[-1]
    n4, C4 = rows * C // 4, C // 4
    assert n4 > 8192 * 256 and (8192 * 256) % C4 != 0


# --------------------------------------------------------------------------------------------------------------------------------- MaxPool
@pytest.mark.parametrize("kind", ("ties",) + tc.POOL_SPECIAL)
@pytest.mark.parametrize("shape", tc.POOL_CASES[:-1], ids=lambda s: "x".join(map(str, s)))
def test_pool_restatement_is_aten_and_a_stride_on_H_is_refused(shape, kind):
    x, dy = tc.pool_inputs(*shape, kind=kind)
    y_ref, dx_ref = tc.pool_reference(x, dy)
    assert torch.equal(y_ref, emu_ops.maxpool2_fwd(x)) and torch.equal(tc.bits(dx_ref), tc.bits(emu_ops.maxpool2_bwd(x, dy)))
    y, dx = tc.pool_kernel_np(x, dy)
    assert torch.equal(tc.bits(y), tc.bits(y_ref))                   # the zero signs of the +-0 case included
    assert torch.equal(tc.bits(dx), tc.bits(dx_ref))                 # every element one dy or +0; none left NaN
    B, H, W, C = shape
    win = x.view(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B, H // 2, W // 2, C, 4)
    if kind == "ties" and x.numel() >= 480:
        assert ((win == win.amax(-1, keepdim=True)).sum(-1) > 1).float().mean() > 0.5          # most windows tie
    if kind == "neg_inf" and x.numel() >= 480:
        dead = (win == -float("inf")).all(-1)
        assert dead.any() and (y_ref[dead] == -float("inf")).all()
        first = dx_ref.view(B, H // 2, 2, W // 2, 2, C)[:, :, 0, :, 0, :]
        assert torch.equal(first[dead], dy[dead])                    # ATen: an all -inf window sends its gradient to (0, 0)
    if kind == "signed_zero":
        first = dx_ref.view(B, H // 2, 2, W // 2, 2, C)[:, :, 0, :, 0, :]
        assert torch.equal(first, dy)                                # -0 == +0: the first of the window wins
        assert torch.equal(tc.bits(y_ref), tc.bits(x.view(B, H // 2, 2, W // 2, 2, C)[:, :, 0, :, 0, :]))     # ... and ATen returns ITS bits
        if x.numel() >= 480:                                         # a maximum that prefers +0 (fmaxf on the GPU, np.maximum's order) is refused
            plus = torch.where(torch.signbit(win).all(-1), torch.tensor(-0.0), torch.tensor(0.0))
            assert not torch.equal(tc.bits(plus), tc.bits(y_ref))
    if H < W:                                                        # the planted stride stays inside the buffer only then
        yb, dxb = tc.pool_kernel_np(x, dy, row_stride_on="H")
        if kind == "ties":
            assert not torch.equal(yb, y_ref)
        assert not torch.equal(tc.bits(dxb), tc.bits(dx_ref))


def test_pool_large_case_wraps_the_grid():
    B, H, W, C = tc.POOL_CASES[-1]
    assert B * (H // 2) * (W // 2) * (C // 4) > 16384 * 256 and H != W


# ------------------------------------------------------------------------------------------------------------------------------- head crop
def test_crop_boxes_valid_flags_and_tail_blocks():
    x, box = tc.crop_inputs()
    N, C, H, W = tc.CROP_IMAGE
    assert [0 if tc.crop_rect(b, H, W) is None else 1 for b in tc.CROP_BOXES] == list(tc.CROP_VALID)
    assert emu_ops._crop_ref(x, box, (7, 5))[1].tolist() == [float(v) for v in tc.CROP_VALID]
    assert (112 * 96) % 256 == 0 and (17 * 31) % 256 == 15 and all((oh * ow) % 256 for oh, ow in tc.CROP_OUT[1:])
    rects = [tc.crop_rect(b, H, W) for b in tc.CROP_BOXES]
    assert (52, 36, 1, 1) in rects and (0, 0, W, H) in rects          # a one-pixel crop in the last row and column; the whole image


@pytest.mark.parametrize("out_hw", tc.CROP_OUT, ids=lambda s: "%dx%d" % s)
def test_crop_forward_restatement_within_tolerance_and_a_dropped_block_is_refused(out_hw):
    x, box = tc.crop_inputs()
    ref, valid_ref = emu_ops._crop_ref(x, box, out_hw)
    y, valid = tc.crop_kernel_np(x, box, out_hw)
    assert torch.equal(valid, valid_ref)
    err = float((y - ref).abs().max())
    print(f"crop forward {out_hw}: fp32 restatement against the fp32 reference {err:.2e} (tolerance {tc.CROP_FWD_TOL:.0e})")
    assert not torch.isnan(y).any() and err <= tc.CROP_FWD_TOL / 4
    dropped = valid_ref == 0
    assert (y[dropped] == 0).all() and (ref[dropped] == 0).all()
    # the planted error: one block fewer per (sample, channel).  At 112 x 96 = 42 * 256 it takes a full block, elsewhere the ragged tail
    blocks = (out_hw[0] * out_hw[1] + 255) // 256
    yb, _ = tc.crop_kernel_np(x, box, out_hw, blocks=blocks - 1)
    assert torch.isnan(yb).any() and not ((yb - ref).abs() <= tc.CROP_FWD_TOL).all()
    # ... and a guard-less launch grid that is exact only at 112 x 96: floor(pixels / 256) blocks
    yf, _ = tc.crop_kernel_np(x, box, out_hw, blocks=(out_hw[0] * out_hw[1]) // 256)
    assert torch.isnan(yf).any() == (out_hw != (112, 96))


@pytest.mark.parametrize("out_hw", tc.CROP_OUT_BWD, ids=lambda s: "%dx%d" % s)
def test_crop_backward_references_agree_and_restatement_within_tolerance(out_hw):
    x, box = tc.crop_inputs()
    N, C, H, W = tc.CROP_IMAGE
    dy = tc.crop_dy(out_hw)
    ref = emu_ops.crop_resize_bwd(dy, box, (H, W))
    assert torch.equal(ref, tc.crop_bwd_ref(dy, box, (H, W)))
    tol = tc.crop_bwd_tol(ref)
    ref64 = tc.crop_bwd_ref(dy, box, (H, W), dtype=torch.float64)
    r64 = float(((ref.double() - ref64).abs() / tol).max())
    got = tc.crop_bwd_kernel_np(dy, box, (H, W))
    rk = float(((got - ref).abs() / tol).max())
    print(f"crop backward {out_hw}: fp32 against float64 reference {r64:.3f} of the tolerance, fp32 restatement against the fp32 reference {rk:.3f}")
    assert r64 <= 0.25 and rk <= 0.25
    outside = torch.ones(N, C, H, W, dtype=torch.bool)
    for i, b in enumerate(tc.CROP_BOXES):
        rect = tc.crop_rect(b, H, W)
        if rect is not None:
            x0, y0, cw, ch = rect
            outside[i, :, y0:y0 + ch, x0:x0 + cw] = False
    assert (ref[outside] == 0).all() and (got[outside] == 0).all()
    # a transposed interpolation that forgets the box origin is refused
    shifted = torch.roll(got, shifts=(1, 1), dims=(2, 3))
    assert not ((shifted - ref).abs() <= tol).all()


# ------------------------------------------------------------------------------------------------------------------ panel pack and unpack
@pytest.mark.parametrize("case", tc.PANEL_CASES, ids=tc.panel_id)
def test_pack_restatements_equal_the_emulation(case):
    sh, tr, kidx, cin, cin_pad, nout, n_pad = case
    w = tc.index_weight(sh)
    want = emu_ops.pack_panel(w, tr, kidx, cin, cin_pad, nout, n_pad)
    Kp = (len(kidx) * cin_pad + 31) // 32 * 32
    assert want.shape == (Kp // 4, n_pad, 4)
    assert torch.equal(tc.pack_kernel_np(w, tr, kidx, cin, cin_pad, nout, n_pad), want)
    if cin_pad % 32 == 0:
        assert torch.equal(tc.pack_kernel_np(w, tr, kidx, cin, cin_pad, nout, n_pad, chunked_form=True), want)
    # every weight element the request covers appears exactly once, everything else is zero padding
    vals = want[want != 0]
    assert len(vals.unique()) == len(vals) and len(vals) >= len(kidx) * cin * nout - 1          # (flat index 0 is a zero itself)
    # the other orientation is another panel
    if sh[0] >= max(cin, nout) and sh[1] >= max(cin, nout):
        assert not torch.equal(emu_ops.pack_panel(w, not tr, kidx, cin, cin_pad, nout, n_pad), want)


def test_panel_cases_cover_the_paths():
    pads = [c[4] for c in tc.PANEL_CASES]
    assert any(p % 32 for p in pads) and any(p % 32 == 0 for p in pads)
    assert any(len(c[2]) * c[4] % 32 for c in tc.PANEL_CASES)                     # K padded up to a multiple of 32 (196 -> 224, 8 -> 32)
    assert any(c[1] and c[3] < c[4] for c in tc.PANEL_CASES) and any(c[5] < c[6] for c in tc.PANEL_CASES) and any(len(c[2]) == 1 for c in tc.PANEL_CASES)


@pytest.mark.parametrize("case", tc.UNPACK_CASES, ids=tc.panel_id)
def test_unpack_restatement_equals_the_emulation_and_keeps_the_sentinel(case):
    sh, tr, tapsets, cin, cin_pad, nout, n_pad = case
    dwks, stages, written = tc.unpack_reference(case)
    assert written.any() and not written.all()
    assert (stages[-1][~written] == tc.SENTINEL).all() and (stages[-1][written] != tc.SENTINEL).all()
    dw = torch.full(sh, tc.SENTINEL)
    for kidx, dwk, want in zip(tapsets, dwks, stages):
        tc.unpack_kernel_np(dwk, dw, tr, kidx, cin, cin_pad, nout)
        assert torch.equal(dw, want)
    # pack and unpack are inverse on the covered positions
    w = tc.index_weight(sh)
    back = torch.full(sh, tc.SENTINEL)
    for kidx in tapsets:
        panel = emu_ops.pack_panel(w, tr, kidx, cin, cin_pad, nout, n_pad)
        rows = len(kidx) * cin_pad
        emu_ops.unpack_wgrad(panel.permute(0, 2, 1).reshape(-1, n_pad)[:rows].contiguous(), back, tr, kidx, cin, cin_pad, nout)
    assert torch.equal(back[written], w[written]) and (back[~written] == tc.SENTINEL).all()
