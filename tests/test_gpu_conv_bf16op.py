"""The opt-in bf16-operand forward / data-gradient convolution (csrc/conv_igemm_bf16op.hip, ops.conv_precision("bf16_operands")) on
the GPU: the kernel against the two derived bounds of tests/convbf16op_emu.py (accumulation: against the fp64 convolution of the bf16-rounded
operands; rounding: against the fp64 convolution of the operands as given), its parity forms, ReLU mask and split-K form, then every layer above it -
ops.conv2d's routing, ConvFn, the trainer's eager and captured steps."""
import functools

import pytest
import torch
import torch.nn.functional as F

from ipercore_amd import _lib, ops
from ipercore_amd.networks import packing, training
from tests import convbf16op_emu as emu
from tests import gpu_checks as gc
from tests.gpu_checks import DEV, _rand
from tests.test_gpu_wgrad_bf16 import TR, _Kinds, _trainer_setup

pytestmark = pytest.mark.gpu
MODE = "bf16_operands"
NAN = float("nan")


def _ids(v):
    return "x".join(map(str, v[0])) + "_k%ds%d" % v[1][:2] if isinstance(v, tuple) and isinstance(v[0], tuple) else str(v)


@functools.lru_cache(maxsize=None)
def _case(case, kind="randn"):
    """Operands of one case (CPU, fp32, unchanged by their users), computed once."""
    return emu.case(case[0], case[1], kind)


@functools.lru_cache(maxsize=None)
def _refs(case, kind, with_bias, act, masked=False):
    """-> (fp64 reference, fp64 rounded reference, (accumulation bound, rounding bound), mask or None) of one case, computed once."""
    x, w, bias, res = _case(case, kind)
    k, stride, pad = case[1]
    b = bias if with_bias else None
    kw = dict(k=k, stride=stride, pad=pad, act=emu.ACT_RELU_MASK if masked else act, res=res if masked else None)
    return emu.reference(x, w, b, **kw), emu.rounded_reference(x, w, b, **kw), emu.bounds(x, w, b, k, stride, pad), (res > 0) if masked else None


def _launch(case, with_bias=True, act=ops.ACT_NONE, masked=False, splitk=False, kind="randn", mode=MODE):
    """One ops.conv2d of a case in a mode -> (the output slice, the whole y, hook kinds, the plan's slices)."""
    (B, H, W, C0, C1, N), (k, stride, pad), sl = case
    x, w, bias, res = _case(case, kind)
    spec = gc._spec_dev(packing.pack_conv(w, bias if with_bias else None, stride=stride, pad=pad))
    xd = x.to(DEV)
    x0 = xd[..., :C0].contiguous()
    x1 = xd[..., C0:].contiguous() if C1 else None
    OH, OW = emu.out_hw(H, W, k, stride, pad)
    YC, ycoff = sl or (N, 0)
    y = torch.full((B, OH, OW, YC), NAN, device=DEV)
    kw = dict(x1=x1, ycoff=ycoff)
    if masked:
        kw.update(epi=ops.EPI_RESIDUAL, act=ops.ACT_RELU_MASK, res=res.to(DEV))
    else:
        kw.update(act=act)
    a = ops.conv_args(x0, spec, y, **kw)
    slices = int(_lib.lib().lwg_conv2d_bf16op_ws_floats(a) // (a.M * a.N))
    with ops.conv_precision(mode), _Kinds() as hook:
        ops.conv2d(x0, spec, y, splitk=splitk, **kw)
    torch.cuda.synchronize()
    return y[..., ycoff:ycoff + N], y, hook.kinds, slices


def _check(tag, got, refs):
    """Finite and inside both derived bounds, element by element (the ReLU mask: where res > 0, exact zeros elsewhere).  Prints before it asserts."""
    ref, rref, bnds, where = refs
    ok, fa, fr = emu.inside(got, ref, rref, bnds, where)
    print(f"conv_bf16op {tag}: err / accumulation bound {fa:.3e}, err / rounding bound {fr:.3e}, "
          f"rel L2 vs fp64 {float((got.double().cpu() - ref).norm() / ref.norm()):.3e}")
    assert torch.isfinite(got).all(), tag
    assert ok, (tag, fa, fr)
    if where is not None:
        assert bool((got.cpu()[~where] == 0).all()), tag


@pytest.mark.parametrize("case", emu.MATRIX, ids=_ids)
def test_kernel_inside_both_bounds(case):
    for with_bias in (True, False):
        for act in (ops.ACT_NONE, ops.ACT_RELU):
            got, y, kinds, _ = _launch(case, with_bias, act)
            assert kinds == ["bf16op"], kinds
            _check(f"{case} bias={with_bias} act={act}", got, _refs(case, "randn", with_bias, act))
            if case[2] is not None:                                      # a slice of a wider y: the other channels stay untouched
                YC, ycoff = case[2]
                rest = torch.cat([y[..., :ycoff], y[..., ycoff + case[0][5]:]], dim=3)
                assert rest.shape[3] == YC - case[0][5] and bool(torch.isnan(rest).all())


def test_transposed_conv_parity_launches():
    """nn.ConvTranspose2d(4, 2, 1), (1, 8, 8, 64) -> (1, 16, 16, 64): conv_transpose2d needs no branch of its own, its four parity specs fall through to
    conv2d; against fp64 conv_transpose2d with bounds built the same way."""
    w, x = _rand((64, 64, 4, 4), 50, 0.05), _rand((1, 8, 8, 64), 51)
    specs = [gc._spec_dev(s) for s in packing.pack_conv_transpose(w, None)]
    y = torch.full((1, 16, 16, 64), NAN, device=DEV)
    with ops.conv_precision(MODE), _Kinds() as hook:
        ops.conv_transpose2d(x.to(DEV), specs, y)
    torch.cuda.synchronize()
    assert hook.kinds == ["bf16op"] * 4, hook.kinds
    _check("conv_transpose 4x4 s2", y, (emu.convt_reference(x, w), emu.convt_rounded_reference(x, w), emu.convt_bounds(x, w), None))


def test_stride2_data_gradient_parity_launches():
    """The four-parity data gradient of Conv2d(4, 2, 1) at H = W = 9 (odd: the parities have 5 / 4 rows) through the out_hw callable, against its
    adjoint in fp64: conv_transpose2d of dy with the same weight, output_padding 1."""
    H = W = 9
    w, dy = _rand((64, 64, 4, 4), 54, 0.05), _rand((2, 4, 4, 64), 55)
    dspecs = [gc._spec_dev(s) for s in packing.pack_dgrad_conv(w, 2, 1, n_pad=64, cin_pad=64)]
    dx = torch.full((2, H, W, 64), NAN, device=DEV)
    with ops.conv_precision(MODE), _Kinds() as hook:
        ops.conv_transpose2d(dy.to(DEV), dspecs, dx, splitk=True, out_hw=lambda s_: ((H - s_.ooy + 1) // 2, (W - s_.oox + 1) // 2))
    torch.cuda.synchronize()
    assert hook.kinds == ["bf16op"] * 4, hook.kinds
    _check("dgrad 4x4 s2 H=W=9", dx, (emu.convt_reference(dy, w, 1), emu.convt_rounded_reference(dy, w, 1), emu.convt_bounds(dy, w, 1), None))


def test_relu_mask_data_gradient():
    got, _, kinds, _ = _launch(emu.MASK_SHAPE, with_bias=False, masked=True)
    assert kinds == ["bf16op"]
    _check("relu mask, whole", got, _refs(emu.MASK_SHAPE, "randn", False, ops.ACT_NONE, True))


@pytest.mark.parametrize("case", emu.SPLITK, ids=_ids)
def test_split_k(case):
    """The one-sample shapes: the plan splits them; plain and with the ReLU mask, each result inside both bounds, and within twice the accumulation
    bound of the whole launch (two summation orders of the same products)."""
    for masked in (False, True):
        refs = _refs(case, "randn", not masked, ops.ACT_NONE, masked)
        whole, _, kw_, slices = _launch(case, not masked, masked=masked, splitk=False)
        split, _, ks_, _ = _launch(case, not masked, masked=masked, splitk=True)
        assert slices > 1, slices
        assert kw_ == ks_ == ["bf16op"]
        _check(f"{case} whole masked={masked}", whole, refs)
        _check(f"{case} split in {slices} masked={masked}", split, refs)
        d, acc = (split.double() - whole.double()).abs().cpu(), refs[2][0]
        print(f"conv_bf16op {case} split vs whole: max diff / accumulation bound {float((d / acc.clamp_min(1e-300)).max()):.3e}, equal {torch.equal(split, whole)}")
        assert bool((d <= 2 * acc).all())


@pytest.mark.parametrize("kind", emu.KINDS)
def test_operand_kinds(kind):
    got, _, _, _ = _launch(emu.KINDS_SHAPE, kind=kind)
    _check(kind, got, _refs(emu.KINDS_SHAPE, kind, True, ops.ACT_NONE))


def test_deterministic():
    """The same launch description gives the same bits: a whole and a split-K launch (slabs added in slice order, no float atomics), each twice from
    fresh outputs."""
    for case, splitk in ((emu.KINDS_SHAPE, False), (emu.SPLITK[0], True)):
        a, b = _launch(case, splitk=splitk)[0], _launch(case, splitk=splitk)[0]
        assert torch.isfinite(a).all() and torch.equal(a, b), case


def _ineligible_cases():
    """name -> callable() -> output of a launch the mode does not take."""
    def cin8():
        spec = gc._spec_dev(packing.pack_conv(_rand((64, 6, 3, 3), 30, 0.05), _rand((64,), 33, 0.1), stride=1, pad=1, cin_pad=8))
        x = _rand((2, 8, 8, 8), 31).to(DEV)
        return lambda: ops.conv2d(x, spec, torch.full((2, 8, 8, 64), NAN, device=DEV), act=ops.ACT_RELU)

    def spade():
        B, H, W, C = 1, 8, 8, 64
        spec = gc._spec_dev(packing.pack_spade_gamma_beta(_rand((C, 64, 3, 3), 110, 0.03), _rand((C,), 111, 0.1), _rand((C, 64, 3, 3), 112, 0.03),
                                                         _rand((C,), 113, 0.1)))
        actv, xn = _rand((B, H, W, 64), 114).to(DEV), (_rand((B, H, W, C), 115, 2.0) + 0.5).to(DEV)
        mean, rstd = xn.reshape(B, -1, C).mean(1), 1 / torch.sqrt(xn.reshape(B, -1, C).var(1, unbiased=False) + 1e-5)
        return lambda: ops.conv2d(actv, spec, torch.full((B, H, W, C), NAN, device=DEV), epi=ops.EPI_SPADE, xn=xn, mean=mean, rstd=rstd)

    def q4():
        spec = gc._spec_dev(packing.pack_conv(_rand((64, 64, 3, 3), 103, 0.05), _rand((64,), 104, 0.1), stride=1, pad=1))
        x = _rand((1, 8, 8, 64), 105).to(DEV)
        return lambda: ops.conv2d(x, spec, torch.full((1, 16, 8, 8, 4), NAN, device=DEV), act=ops.ACT_RELU, q4=True)

    def convt_q4():
        # a transposed convolution the mode refuses (channel-quad planes): the "fp32" mode's form - one grid for a launch this small, hook kind
        # "up4" -, not four parity launches
        specs = [gc._spec_dev(s) for s in packing.pack_conv_transpose(_rand((64, 64, 4, 4), 120, 0.05), _rand((64,), 121, 0.1))]
        x = _rand((1, 8, 8, 64), 122).to(DEV)
        return lambda: ops.conv_transpose2d(x, specs, torch.full((1, 16, 16, 16, 4), NAN, device=DEV), act=ops.ACT_RELU, q4=True)

    def convt_small_group():
        # ops._bf16op_use_parity4: (1, 64, 64, 256) -> 128 as a training caller runs it - one grid in "fp32", and the mode's plan would split each
        # parity launch (eight kernels: measured 1.40 of the one-grid form's time) - keeps the one-grid form
        specs = [gc._spec_dev(s) for s in packing.pack_conv_transpose(_rand((256, 128, 4, 4), 130, 0.03), _rand((128,), 131, 0.1))]
        x = _rand((1, 64, 64, 256), 132).to(DEV)
        assert not ops._bf16op_use_parity4(specs, x, torch.empty(1, 128, 128, 128, device=DEV), ops.ACT_RELU, True)
        return lambda: ops.conv_transpose2d(x, specs, torch.full((1, 128, 128, 128), NAN, device=DEV), act=ops.ACT_RELU, splitk=True)

    return {"cin8": cin8(), "spade": spade(), "q4": q4(), "conv_transpose_q4": convt_q4(), "conv_transpose_small_group": convt_small_group()}


def test_ineligible_launches_keep_the_fp32_route():
    for name, fn in _ineligible_cases().items():
        with ops.conv_precision("fp32"), _Kinds() as h0:
            want = fn()
        with ops.conv_precision(MODE), _Kinds() as h1:
            got = fn()
        torch.cuda.synchronize()
        assert torch.isfinite(want).all() and torch.equal(got, want), name
        assert h1.kinds == h0.kinds and "bf16op" not in h1.kinds, (name, h0.kinds, h1.kinds)
        assert not name.startswith("conv_transpose") or h0.kinds == ["up4"], h0.kinds


def test_the_mode_leaves_nothing_behind():
    """A default-mode conv2d before and after a block in the mode: bitwise equal, the same kernel family, ops.CONV_PRECISION back."""
    case = emu.MATRIX[2]
    prev = ops.CONV_PRECISION
    for mode in (prev, "winograd"):
        before, _, k0, _ = _launch(case, act=ops.ACT_RELU, mode=mode)
        inside, _, k1, _ = _launch(case, act=ops.ACT_RELU)
        _launch(emu.SPLITK[0], splitk=True)
        after, _, k2, _ = _launch(case, act=ops.ACT_RELU, mode=mode)
        assert ops.CONV_PRECISION == prev and ops._MODE_WINO4
        assert k1 == ["bf16op"] and k0 == k2 and "bf16op" not in k0, (k0, k1, k2)
        assert torch.equal(before, after) and not torch.equal(before, inside)


def test_convfn_under_the_mode():
    """One 3x3 layer with bias, 64 -> 64 at 16 x 16, forward then backward: y and dx (plain and with the ReLU mask on the forward input) inside both
    bounds; dw and db - the weight gradient is not this mode's - unchanged from the "fp32" mode for the same dy."""
    x = _rand((2, 16, 16, 64), 60)
    w, b = _rand((64, 64, 3, 3), 61, 0.05), _rand((64,), 62, 0.1)
    up = _rand((2, 16, 16, 64), 63)
    wt = w.permute(1, 0, 2, 3).flip(2, 3).contiguous()              # dx = conv(dy, wt): the stride-1 convolution's adjoint

    def run(mode, mask_dx):
        xd = x.to(DEV).requires_grad_(True)
        wd, bd = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
        with ops.conv_precision(mode), _Kinds() as hook:
            y = training.conv(xd, wd, bd, stride=1, pad=1, mask_dx=mask_dx)
            y.backward(up.to(DEV))
        torch.cuda.synchronize()
        return y.detach(), xd.grad, wd.grad, bd.grad, hook.kinds

    for mask_dx in (False, True):
        y0, gx0, gw0, gb0, k0 = run("fp32", mask_dx)
        y1, gx1, gw1, gb1, k1 = run(MODE, mask_dx)
        assert k1.count("bf16op") == 2 and "bf16op" not in k0 and len(k0) == len(k1), (k0, k1)
        _check(f"ConvFn y mask_dx={mask_dx}", y1, (emu.reference(x, w, b), emu.rounded_reference(x, w, b), emu.bounds(x, w, b), None))
        kw = dict(act=emu.ACT_RELU_MASK, res=x) if mask_dx else {}
        _check(f"ConvFn dx mask_dx={mask_dx}", gx1, (emu.reference(up, wt, None, **kw), emu.rounded_reference(up, wt, None, **kw), emu.bounds(up, wt, None),
                                                     (x > 0) if mask_dx else None))
        assert torch.equal(gw1, gw0) and torch.equal(gb1, gb0)
        assert not torch.equal(y1, y0) and not torch.equal(gx1, gx0)


# ---- the trainer at 64 x 64 (tests/test_gpu_wgrad_bf16.py's TR: S = 64, ns = 2, nf = [64, 64, 128], nres = 2, bgf = [64, 64, 128], L1 loss set)
def _new_trainer(conv, use_graph, wgrad="direct"):
    from ipercore_amd.networks import NetworksFactory
    from ipercore_amd.trainers import LWGTrainer, PatchGlobalDiscriminator, TrainOpts
    inp, sdn = _trainer_setup()
    G = NetworksFactory.get_by_name("AttLWB-SPADE", cfg=gc.pu.gen_cfg(TR["nf"], TR["nres"], TR["bgf"]), temporal=False)
    G.load_state_dict({k: torch.tensor(v) for k, v in sdn.items()}, strict=True)
    G.to(DEV).train()
    torch.manual_seed(0)
    D = PatchGlobalDiscriminator().to(DEV)
    opts = TrainOpts.l1_transfer()
    opts.use_graph, opts.wgrad_precision = use_graph, wgrad
    if conv is not None:
        opts.conv_precision = conv
    tr = LWGTrainer(G, D, opts=opts)
    tr.set_input({k: v.clone() for k, v in inp.items()})
    return tr


def test_trainer_captured_against_eager():
    """Two LWGTrainer steps at 64^2 with TrainOpts.conv_precision = "bf16_operands", captured against eager, held to what
    gpu_checks._graph_vs_eager_steps holds the other modes to; the new kernel ran, no Winograd launch did, and the switch is back after every step."""
    N, runs, prev = 2, {}, ops.CONV_PRECISION
    for mode in ("eager", "graph"):
        tr = _new_trainer(MODE, mode == "graph")
        with _Kinds() as hook:
            hist = []
            for _ in range(N):
                hist.append(tr.optimize_parameters())
                assert ops.CONV_PRECISION == prev
        torch.cuda.synchronize()
        assert "bf16op" in hook.kinds and not [k for k in hook.kinds if k.startswith("winograd")], (mode, sorted(set(hook.kinds)))
        runs[mode] = dict(losses=[(float(a), float(b)) for a, b in hist], flatG=tr.optimizer_G.flat.clone(), flatD=tr.optimizer_D.flat.clone(),
                          tG=int(tr.optimizer_G.t_dev.item()), tD=int(tr.optimizer_D.t_dev.item()), step_mode=tr.step_mode)
    e, gr = runs["eager"], runs["graph"]
    assert "hipGraph" in gr["step_mode"], gr["step_mode"]
    assert e["tG"] == gr["tG"] == N and e["tD"] == gr["tD"] == N
    lr = 1e-4
    for (a0, b0), (a1, b1) in zip(e["losses"], gr["losses"]):
        assert abs(a0 - a1) <= 2e-3 * max(1.0, abs(a0)) and abs(b0 - b1) <= 2e-3 * max(1.0, abs(b0)), (e["losses"], gr["losses"])
    for k in ("flatG", "flatD"):
        d = (e[k] - gr[k]).abs()
        print(f"conv_bf16op trainer graph vs eager {k}: max {d.max().item():.3e} mean {d.mean().item():.3e}")
        assert d.max().item() <= 2 * N * lr and d.mean().item() <= 0.1 * lr, (k, d.max().item(), d.mean().item())


class _EligibleLaunches:
    """Wraps ops.conv2d: every launch the mode takes is recorded with its operands and its result cloned."""

    def __init__(self):
        self.calls = []

    def __enter__(self):
        self.orig = orig = ops.conv2d
        cl = lambda t: None if t is None else t.detach().clone()      # noqa: E731

        def spy(x0, spec, y, x1=None, epi=ops.EPI_NONE, act=ops.ACT_NONE, res=None, xn=None, mean=None, rstd=None, out_hw=None, ycoff=0,
                splitk=False, q4=False, lists=None):
            take = ops.CONV_PRECISION == MODE and ops._bf16op_use(spec, x0, y, x1, epi, act, q4, ycoff)
            # (the panel and the bias are cloned too: views of live parameters, which the optimizer moves at the end of the step)
            args = (cl(x0), spec, cl(x1), epi, act, cl(res), out_hw, ycoff, cl(spec.w), cl(spec.bias)) if take else None
            out = orig(x0, spec, y, x1=x1, epi=epi, act=act, res=res, xn=xn, mean=mean, rstd=rstd, out_hw=out_hw, ycoff=ycoff, splitk=splitk, q4=q4,
                       lists=lists)
            if take:
                self.calls.append(args + (cl(y),))
            return out

        ops.conv2d = spy
        return self

    def __exit__(self, *exc):
        ops.conv2d = self.orig


def _spec_conv64(x, wk, spec, OH, OW):
    """fp64 convolution of x (B, H, W, Cin) by the taps of a spec with weights wk (ntaps, Cin, N), on the device -> (B, OH, OW, N)."""
    B, H, W, _ = x.shape
    s = spec.stride
    lo_y, lo_x = max(0, -min(spec.dy)), max(0, -min(spec.dx))
    hi_y, hi_x = max(0, (OH - 1) * s + max(spec.dy) - (H - 1)), max(0, (OW - 1) * s + max(spec.dx) - (W - 1))
    xp = F.pad(x, (0, 0, lo_x, hi_x, lo_y, hi_y))
    acc = torch.zeros(B, OH, OW, wk.shape[2], dtype=torch.float64, device=x.device)
    for t in range(spec.ntaps):
        y0, x0 = lo_y + spec.dy[t], lo_x + spec.dx[t]
        acc += xp[:, y0:y0 + (OH - 1) * s + 1:s, x0:x0 + (OW - 1) * s + 1:s, :] @ wk[t]
    return acc


def _check_recorded(call):
    """One recorded launch against fp64 on its own operands (the fp32 panel unpacked: k = ((c / 32) ntaps + tap) 32 + c % 32) -> the two ratios."""
    x0, spec, x1, epi, act, res, out_hw, ycoff, panel, sbias, y = call
    assert act in (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_RELU_MASK), act
    x = (x0 if x1 is None else torch.cat([x0, x1], dim=3)).double()
    nt, cin, N = spec.ntaps, spec.Cin, spec.N
    wk = panel.permute(0, 2, 1).reshape(cin // 32, nt, 32, N).permute(1, 0, 2, 3).reshape(nt, cin, N).double()
    OH, OW = (y.shape[1] // spec.omul, y.shape[2] // spec.omul) if out_hw is None else out_hw
    got = y[:, spec.ooy::spec.omul, spec.oox::spec.omul, ycoff:ycoff + N][:, :OH, :OW].double()
    r = None if res is None else res[:, spec.ooy::spec.omul, spec.oox::spec.omul, ycoff:ycoff + N][:, :OH, :OW].double()
    bias = 0 if sbias is None else sbias.double()
    rd = lambda t: t.float().bfloat16().double()          # noqa: E731
    masked = act == ops.ACT_RELU_MASK

    def ep(acc):
        if masked:
            return torch.where(r > 0, acc, torch.zeros_like(acc))
        acc = acc if r is None else acc + r
        return acc.relu() if act == ops.ACT_RELU else acc

    ref, rref = ep(_spec_conv64(x, wk, spec, OH, OW) + bias), ep(_spec_conv64(rd(x), rd(wk), spec, OH, OW) + bias)
    ab = 0 if sbias is None else sbias.double().abs()
    extra = 0 if (r is None or masked) else r.abs()
    S, S_hat = _spec_conv64(x.abs(), wk.abs(), spec, OH, OW) + ab + extra, _spec_conv64(rd(x).abs(), rd(wk).abs(), spec, OH, OW) + ab + extra
    acc, rnd = emu.bounds_of(nt * cin + 1 + (r is not None and not masked), S_hat, S)
    ea, er = (got - rref).abs(), (got - ref).abs()
    if masked:
        assert bool((got[r <= 0] == 0).all())
        ea, er, acc, rnd = ea[r > 0], er[r > 0], acc[r > 0], rnd[r > 0]
    assert torch.isfinite(got).all()
    fa, fr = float((ea / acc.clamp_min(1e-300)).max()), float((er / rnd.clamp_min(1e-300)).max())
    assert bool((ea <= acc).all()) and bool((er <= rnd).all()), (tuple(y.shape), nt, cin, N, epi, act, fa, fr)
    return fa, fr


def test_every_eligible_launch_of_a_step_inside_both_bounds():
    """Every launch of one eager step in the mode that the new kernel takes, recorded with its operands, held to both bounds against fp64 on those
    operands; the hook shows the new kernel and no Winograd launch."""
    tr = _new_trainer(MODE, False)
    with _Kinds() as hook, _EligibleLaunches() as rec:
        lg, ld = tr.optimize_parameters()
    torch.cuda.synchronize()
    assert torch.isfinite(lg) and torch.isfinite(ld)
    assert hook.kinds.count("bf16op") == len(rec.calls) >= 20, (hook.kinds.count("bf16op"), len(rec.calls))
    assert not [k for k in hook.kinds if k.startswith("winograd")], sorted(set(hook.kinds))
    worst = [0.0, 0.0]
    for call in rec.calls:
        fa, fr = _check_recorded(call)
        worst = [max(worst[0], fa), max(worst[1], fr)]
    forms = {(c[1].ntaps, c[1].stride, c[1].omul, c[3], c[4]) for c in rec.calls}
    print(f"conv_bf16op trainer launches: {len(rec.calls)} eligible in {len(forms)} forms (ntaps, stride, omul, epi, act), worst err / accumulation bound "
          f"{worst[0]:.3e}, err / rounding bound {worst[1]:.3e}")


def test_one_captured_trainer_switches_modes():
    """winograd -> bf16_operands -> winograd on ONE captured trainer: the convolution kernels are frozen into the graph, so each switch re-captures the
    step (the hook sees the launches of a capture, and none of a replay) and the step stays a hipGraph.  Its last capture launches exactly the kernel
    families a fresh default trainer's capture launches."""
    tr = _new_trainer("winograd", True)

    def step(t, mode):
        t.opts.conv_precision = mode
        with _Kinds() as hook:
            lg, ld = t.optimize_parameters()
        torch.cuda.synchronize()
        assert torch.isfinite(lg) and torch.isfinite(ld)
        assert "hipGraph" in t.step_mode, t.step_mode
        return hook.kinds

    k = step(tr, "winograd")                             # (at 64^2 the default mode's launches are too small for its Winograd kernels: "direct")
    assert k and "bf16op" not in k, sorted(set(k))
    k = step(tr, MODE)
    assert "bf16op" in k and not [q for q in k if q.startswith("winograd")], sorted(set(k))
    pc = getattr(tr, "_panel_cache", None)               # the other mode's derived panels do not ride along in the per-step refresh
    assert pc is None or (not pc.wino and not pc.wino4), (len(pc.wino), len(pc.wino4))
    assert step(tr, MODE) == []                          # a replay: no launch goes through the hook
    last = step(tr, "winograd")
    assert last and "bf16op" not in last, sorted(set(last))
    assert step(tr, "winograd") == []
    assert int(tr.optimizer_G.t_dev.item()) == 5 and int(tr.optimizer_D.t_dev.item()) == 5
    assert torch.isfinite(tr.optimizer_G.flat).all() and torch.isfinite(tr.optimizer_D.flat).all()
    fresh = _new_trainer(None, True)                     # default TrainOpts.conv_precision
    assert fresh.opts.conv_precision == "winograd"
    assert step(fresh, "winograd") == last


def test_with_the_bf16_weight_gradient():
    """The whole recipe, ("bf16_operands", "bf16"): a captured step runs, both kernels in it, finite losses."""
    tr = _new_trainer(MODE, True, wgrad="bf16")
    with _Kinds() as hook:
        losses = [tr.optimize_parameters() for _ in range(2)]
    torch.cuda.synchronize()
    assert "bf16op" in hook.kinds and "wgrad_bf16" in hook.kinds
    assert all(torch.isfinite(a) and torch.isfinite(b) for a, b in losses), losses
    assert ops.CONV_PRECISION != MODE and ops.WGRAD_PRECISION == "direct"
