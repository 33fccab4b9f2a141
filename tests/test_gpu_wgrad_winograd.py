"""The opt-in F(2x2, 3x3) Winograd weight gradient (csrc/conv_wgrad_winograd.hip, ops.wgrad_precision("winograd")) on the GPU:
the kernel against torch.nn.grad.conv2d_weight in fp64 with the direct kernel (lwg_conv2d_wgrad_unpacked_f32) on the same operands as the
yardstick, then every layer above it - packing.wgrad_conv, ConvFn, the generator's training gradients, the trainer's eager and captured steps."""
import functools

import pytest
import torch

from ipercore_amd import ops
from ipercore_amd.networks import packing, training
from tests import gpu_checks as gc
from tests import wgradwino_emu as emu
from tests.gpu_checks import DEV, _rand

pytestmark = pytest.mark.gpu

BIG = (1, 128, 128, 128, 0, 128)          # 4096 tiles: many slabs
MATRIX = [
    ((1, 8, 8, 64, 0, 64), None),         # one block
    ((3, 9, 7, 64, 0, 64), None),         # odd H and W; 20 tiles per image: chunks straddle images
    ((1, 3, 5, 64, 0, 64), None),         # smaller than one chunk
    ((2, 16, 32, 64, 0, 128), None),      # two column blocks
    ((1, 32, 32, 64, 0, 192), None),      # N is not a multiple of 128
    ((1, 16, 16, 128, 256, 256), None),   # two inputs
    (BIG, None),
    ((1, 16, 16, 64, 0, 64), (60, 61)),   # padded channels dropped
]


class _Kinds:
    """ops.CONV_HOOK recorder: the kinds of the closing calls."""

    def __init__(self):
        self.kinds = []

    def __call__(self, begin, M, spec, epi=0, info=None):
        if not begin:
            self.kinds.append(info["kind"])

    def __enter__(self):
        self.prev, ops.CONV_HOOK = ops.CONV_HOOK, self
        return self

    def __exit__(self, *exc):
        ops.CONV_HOOK = self.prev


def _rel(got, ref):
    return float((got.double().cpu() - ref).norm() / ref.norm())


def _spec(cin, nout, cp, npad, seed=5):
    return gc._spec_dev(packing.pack_conv(_rand((nout, cin, 3, 3), seed, 0.05), None, stride=1, pad=1, cin_pad=cp, n_pad=npad))


@functools.lru_cache(maxsize=None)
def _case(shape, drop=None, kind="randn"):
    """Operands (CPU, fp32, unchanged by their users) and the fp64 reference of one case, computed once."""
    B, H, W, C0, C1, N = shape
    C = C0 + C1
    x, dy = _operands(kind, (B, H, W, C), (B, H, W, N), 900 + H + C + N)
    cin, nout = drop or (C, N)
    ref = emu.reference(x[..., :cin], dy[..., :nout])
    return x, dy, ref, cin, nout


def _operands(kind, sx, sy, seed):
    x, dy = _rand(sx, seed), _rand(sy, seed + 1)
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
        chi2 = sum(_rand(sy, seed + 2 + i).pow(2) for i in range(3))          # Student-t, 3 degrees of freedom: z / sqrt(chi2_3 / 3)
        dy = dy / torch.sqrt(chi2 / 3.0)
    else:
        assert kind == "randn", kind
    return x.contiguous(), dy.contiguous()


def _run_both(shape, x, dy, cin, nout):
    """-> (Winograd dw, direct dw, hook kinds of the Winograd launch), both (nout, cin, 3, 3) pre-filled with NaN."""
    B, H, W, C0, C1, N = shape
    spec = _spec(cin, nout, C0 + C1, N)
    xd, dyd = x.to(DEV), dy.to(DEV)
    x0 = xd[..., :C0].contiguous()
    x1 = xd[..., C0:].contiguous() if C1 else None
    assert ops._wgrad_wino_use(x0, spec, dyd, x1)
    dww = torch.full((nout, cin, 3, 3), float("nan"), device=DEV)
    dwd = torch.full((nout, cin, 3, 3), float("nan"), device=DEV)
    with _Kinds() as hook:
        ops.conv2d_wgrad_winograd(x0, spec, dyd, dww, cin, nout, x1=x1)
    ops.conv2d_wgrad_unpacked(x0, spec, dyd, dwd, False, range(9), cin, nout, x1=x1)
    torch.cuda.synchronize()
    return dww, dwd, hook.kinds


def _check_ratio(tag, dww, dwd, ref):
    """Finite, not the direct kernel's bits, relative L2 against fp64 <= 4x the direct kernel's (check_winograd_adversarial's bound for the forward
    F(2x2, 3x3) kernel; the fp32 CPU emulation sits at 0.55 - 1.06x)."""
    assert torch.isfinite(dww).all(), tag
    assert torch.isfinite(dwd).all(), tag
    ew, ed = _rel(dww, ref), _rel(dwd, ref)
    print(f"wgrad_winograd {tag}: rel L2 vs fp64 winograd {ew:.3e} direct {ed:.3e} ratio {ew / ed:.2f}")
    assert not torch.equal(dww, dwd), tag
    assert ew <= 4.0 * ed, (tag, ew, ed)


@pytest.mark.parametrize("shape,drop", MATRIX, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "")
def test_kernel_against_fp64_and_direct(shape, drop):
    x, dy, ref, cin, nout = _case(shape, drop)
    dww, dwd, kinds = _run_both(shape, x, dy, cin, nout)
    assert kinds == ["wgrad_winograd"], kinds
    _check_ratio(str(shape), dww, dwd, ref)


@pytest.mark.parametrize("kind", ["dc10", "dc100", "post_relu", "chan_scales", "dy_1e-3", "student_t_dy"])
def test_adversarial_operands(kind):
    shape = (2, 32, 32, 128, 0, 128)
    x, dy, ref, cin, nout = _case(shape, None, kind)
    dww, dwd, _ = _run_both(shape, x, dy, cin, nout)
    _check_ratio(kind, dww, dwd, ref)


def test_deterministic():
    """Slabs are added in slab order, no float atomics: three launches of the 4096-tile case are bitwise equal."""
    x, dy, _, cin, nout = _case(BIG)
    outs = [_run_both(BIG, x, dy, cin, nout)[0] for _ in range(3)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@pytest.mark.parametrize("shape", [(3, 9, 7, 64, 0, 64), (2, 16, 32, 64, 0, 128)])
def test_kernel_against_fp32_emulation(shape):
    """The kernel and tests/wgradwino_emu.py in fp32 form the same products V_t Z_t (V and Z: two nested two-term sums, <= 2 roundings each whatever the
    grouping) and differ in the order the T tiles' products are added.  Any summation order of T fp32 terms is within (T - 1) u sum|terms| of the
    exact sum (u = 2^-24, Higham's gamma_n to first order), the operand roundings add <= 4 u per product on each side: the two evaluations of
    dU[xi, nu][c][n] differ by at most 2 (T + 8) u S, S = sum_t |V_t| |Z_t| (evaluated in fp64), and through |G^T| . |G| (the output transform,
    <= 2 more roundings per stage: the + 8 covers them) element by element.  T = 60 and 256 here.  Derived, not tuned."""
    B, H, W, C0, C1, N = shape
    x, dy, _, cin, nout = _case(shape)
    dww, _, _ = _run_both(shape, x, dy, cin, nout)
    want = emu.wgrad(x, dy, chunk=8)
    assert want.dtype == torch.float32
    V, Z = emu.transforms(x.double(), dy.double())
    T = V.shape[0]
    S = torch.einsum("txnc,txnm->xncm", V.abs(), Z.abs())
    g = torch.tensor(emu.G, dtype=torch.float64).abs()
    bound = 2.0 * (T + 8) * 2.0 ** -24 * torch.einsum("xk,xncm,nl->mckl", g, S, g)
    err = (dww.double().cpu() - want.double()).abs()
    print(f"wgrad_winograd vs fp32 emulation {shape}: max err / bound {float((err / bound).max()):.3e}, T = {T}")
    assert bool((err <= bound).all()), float((err / bound).max())


def _ineligible_cases():
    """name -> callable() -> weight gradient through packing.wgrad_conv / wgrad_conv_transpose / wgrad_thin; none is a launch of the new kernel."""
    def conv(cin, n, k, stride, pad, hw, cin_pad=None, seed=30):
        w = _rand((n, cin, k, k), seed, 0.05).to(DEV)
        spec = gc._spec_dev(packing.pack_conv(w, None, stride=stride, pad=pad, cin_pad=cin_pad))
        x = _rand((2, hw, hw, spec.Cin), seed + 1).to(DEV)
        oh = (hw + 2 * pad - k) // stride + 1
        dy = _rand((2, oh, oh, spec.N), seed + 2).to(DEV)
        return lambda: packing.wgrad_conv(x, spec, dy, None, k, k, cin, n)

    def thin():
        w = _rand((3, 64, 5, 5), 40, 0.05).to(DEV)
        x, dy = _rand((1, 16, 16, 64), 41).to(DEV), _rand((1, 16, 16, 4), 42).to(DEV)
        return lambda: training.thin_backward(x, w, dy, 2, False, True)[1]

    def convt():
        w = _rand((64, 64, 4, 4), 50, 0.05).to(DEV)
        specs = [gc._spec_dev(s) for s in packing.pack_conv_transpose(w, None)]
        adj = gc._spec_dev(packing.pack_dgrad_conv_transpose(w, n_pad=64)[0])
        x, dy = _rand((1, 8, 8, 64), 51).to(DEV), _rand((1, 16, 16, 64), 52).to(DEV)
        return lambda: packing.wgrad_conv_transpose(x, specs, dy, 64, 64, adj_spec=adj)

    return {"1x1": conv(64, 64, 1, 1, 0, 8), "3x3_stride2": conv(64, 64, 3, 2, 1, 8), "4x4_stride2": conv(64, 64, 4, 2, 1, 8),
            "first_layer_6_to_64": conv(6, 64, 3, 1, 1, 8, cin_pad=8), "thin_5x5": thin(), "conv_transpose": convt()}


def test_ineligible_launches_keep_the_default_path():
    for name, fn in _ineligible_cases().items():
        with _Kinds() as h0:
            want = fn()
        with ops.wgrad_precision("winograd"), _Kinds() as h1:
            got = fn()
        torch.cuda.synchronize()
        assert torch.isfinite(want).all() and torch.equal(got, want), name
        assert h1.kinds == h0.kinds and "wgrad_winograd" not in h1.kinds, (name, h0.kinds, h1.kinds)


def test_convfn_weight_and_bias_gradients():
    """One 3x3 layer with bias, (2, 16, 16, 64 -> 128), forward then backward with the switch on: weight.grad within the ratio bound, bias.grad
    (ops.colsum instead of the fused column sums) equal to the default mode's to 1e-6 relative."""
    x = _rand((2, 16, 16, 64), 60)
    w, b = _rand((128, 64, 3, 3), 61, 0.05), _rand((128,), 62, 0.1)
    up = _rand((2, 16, 16, 128), 63)
    ref = emu.reference(x, up)

    def run(mode):
        wd, bd = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
        with ops.wgrad_precision(mode), _Kinds() as hook:
            y = training.conv(x.to(DEV), wd, bd, stride=1, pad=1)
            y.backward(up.to(DEV))
        torch.cuda.synchronize()
        return wd.grad, bd.grad, hook.kinds

    gw0, gb0, k0 = run("direct")
    gw1, gb1, k1 = run("winograd")
    assert "wgrad_winograd" in k1 and "wgrad_winograd" not in k0, (k0, k1)
    _check_ratio("ConvFn 64->128", gw1, gw0, ref)
    assert float((gb1 - gb0).norm() / gb0.norm()) <= 1e-6
    assert _rel(gb1, up.double().sum(dim=(0, 1, 2))) <= 1e-6


def test_generator_training_grads_with_the_switch_on():
    """gpu_checks._generator_training_grads at its smallest configuration inside ops.wgrad_precision("winograd"): the helper's own bounds against the
    oracle hold unchanged, and the new kernel really ran."""
    with ops.wgrad_precision("winograd"), _Kinds() as hook:
        m = gc._generator_training_grads(64, [64, 64, 128], 2, [64, 64, 128], precisions=("winograd",), wino_min_grid=0)
    assert "wgrad_winograd" in hook.kinds
    print("wgrad_winograd generator grads:", m["worst_rel_grad_err"], m["worst_param"])


TR = dict(S=64, ns=2, nf=[64, 64, 128], nres=2, bgf=[64, 64, 128])      # gpu_checks.check_graph_vs_eager_steps' configuration


def _trainer_inputs(S, ns, nf, nres, bgf):
    from ipercore_amd import synthetic
    u = lambda shape, seed, name: torch.tensor(synthetic.uniform_image(shape, seed, name), device=DEV)      # noqa: E731
    bg_in, src_in, tsf_in, Tst = gc._training_inputs(S, ns, nf, nres, bgf, False)
    return {"input_G_bg": bg_in.to(DEV), "input_G_src": src_in.to(DEV), "input_G_tsf": tsf_in.to(DEV), "Tst": Tst.to(DEV),
            "real_src": u((1, ns, 3, S, S), 700, "real_src"), "real_tsf": u((1, 1, 3, S, S), 701, "real_tsf"),
            "real_bg": u((1, 3, S, S), 702, "real_bg"), "body_mask": (u((1, ns + 1, 1, S, S), 703, "mask") > 0).float()}


@functools.lru_cache(maxsize=None)
def _trainer_setup():
    """(inputs, generator state dict) shared by the trainer tests; their users clone / copy, never write."""
    from ipercore_amd import synthetic
    from ipercore_amd.networks import generator_param_shapes
    return (_trainer_inputs(**TR), synthetic.fill_state_dict(generator_param_shapes(TR["nf"], TR["nres"], TR["bgf"]), seed=7))


def _trainer(wgrad, use_graph, inp, sdn, nf, nres, bgf):
    from ipercore_amd.networks import NetworksFactory
    from ipercore_amd.trainers import LWGTrainer, PatchGlobalDiscriminator, TrainOpts
    G = NetworksFactory.get_by_name("AttLWB-SPADE", cfg=gc.pu.gen_cfg(nf, nres, bgf), temporal=False)
    G.load_state_dict({k: torch.tensor(v) for k, v in sdn.items()}, strict=True)
    G.to(DEV).train()
    torch.manual_seed(0)
    D = PatchGlobalDiscriminator().to(DEV)
    opts = TrainOpts.l1_transfer()
    opts.use_graph, opts.wgrad_precision = use_graph, wgrad
    tr = LWGTrainer(G, D, opts=opts)
    tr.set_input({k: v.clone() for k, v in inp.items()})
    return tr


def _new_trainer(wgrad, use_graph):
    inp, sdn = _trainer_setup()
    return _trainer(wgrad, use_graph, inp, sdn, TR["nf"], TR["nres"], TR["bgf"])


class _EligibleLaunches:
    """Records (arguments, result) of every packing.wgrad_conv call whose launch the Winograd mode would take (ops._wgrad_wino_use)."""

    def __init__(self):
        self.calls = []

    def __enter__(self):
        self.orig = orig = packing.wgrad_conv

        def spy(x0, spec, dy, x1, kh, kw, cin, n, db=None):
            dw = orig(x0, spec, dy, x1, kh, kw, cin, n, db=db)
            if kh == 3 and kw == 3 and ops._wgrad_wino_use(x0, spec, dy, x1):
                self.calls.append(((x0.clone(), spec, dy.clone(), None if x1 is None else x1.clone(), kh, kw, cin, n), db is not None, dw.clone(),
                                   None if db is None else db.clone()))
            return dw

        packing.wgrad_conv = spy
        return self

    def __exit__(self, *exc):
        packing.wgrad_conv = self.orig


def test_trainer_captured_against_eager():
    """Two LWGTrainer steps at 64^2 with TrainOpts.wgrad_precision = "winograd", captured against eager, held to the bounds of
    gpu_checks._graph_vs_eager_steps (a local copy: the helper takes no options); the new kernel ran and the switch is back at "direct" after
    every step."""
    N, runs = 2, {}
    for mode in ("eager", "graph"):
        tr = _new_trainer("winograd", mode == "graph")
        with _Kinds() as hook:
            hist = [tr.optimize_parameters() for _ in range(N)]
        torch.cuda.synchronize()
        assert ops.WGRAD_PRECISION == "direct"
        assert "wgrad_winograd" in hook.kinds, mode
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
        assert d.max().item() <= 2 * N * lr and d.mean().item() <= 0.1 * lr, (k, d.max().item(), d.mean().item())


def test_the_mode_leaves_nothing_behind():
    """A fresh default trainer's first step before the mode ran against one after it (a captured and an eager Winograd trainer step in between).
    Everything of the step that is a deterministic function of its inputs is held to bitwise equality: both losses, the discriminator's weights,
    the sequence of hook kinds (none of the new kernel), ops.WGRAD_PRECISION - and the weight gradient and fused bias gradient of EVERY launch the
    mode takes over: the launches of the "before" step are recorded with their operands and run again after the mode, through packing.wgrad_conv
    in the default mode, on those operands.  The generator's updated weights are not compared run against run: most of its gradients pass
    through the fp32 atomics of the attention / warp backward, and two default first steps do not reproduce them bitwise with the mode never
    entered (profiles/wgrad_winograd_default_repro.txt) - that comparison would test the atomics, not the mode."""
    def first_default_step(record):
        tr = _new_trainer("direct", False)
        with _Kinds() as hook, record:
            lg, ld = tr.optimize_parameters()
        torch.cuda.synchronize()
        return float(lg), float(ld), tr.optimizer_D.flat.clone(), hook.kinds

    rec = _EligibleLaunches()
    before = first_default_step(rec)
    assert rec.calls and "wgrad_winograd" not in before[3], (len(rec.calls), before[3])
    for graph in (True, False):
        tr = _new_trainer("winograd", graph)
        with _Kinds() as hook:
            tr.optimize_parameters()
        torch.cuda.synchronize()
        assert "wgrad_winograd" in hook.kinds
    assert ops.WGRAD_PRECISION == "direct"
    after = first_default_step(_EligibleLaunches())
    assert after[3] == before[3], (before[3], after[3])
    assert (before[0], before[1]) == (after[0], after[1]), (before[:2], after[:2])
    assert torch.equal(before[2], after[2])
    for args, fused, dw, db in rec.calls:
        db1 = torch.full_like(db, float("nan")) if fused else None
        with _Kinds() as hook:
            dw1 = packing.wgrad_conv(*args, db=db1)
        torch.cuda.synchronize()
        assert "wgrad_winograd" not in hook.kinds, hook.kinds          # the direct weight gradient goes through no hook
        assert torch.equal(dw1, dw), (tuple(dw.shape), float((dw1 - dw).abs().max()))
        assert not fused or torch.equal(db1, db)


def test_one_captured_trainer_switches_modes():
    """direct -> winograd -> direct on ONE captured trainer: the weight-gradient kernels are frozen into the graph, so each switch re-captures the
    step (the hook sees the launches of a capture, and none of a replay) with the kernels of the new mode, and the step stays a hipGraph."""
    tr = _new_trainer("direct", True)

    def step(mode):
        tr.opts.wgrad_precision = mode
        with _Kinds() as hook:
            lg, ld = tr.optimize_parameters()
        torch.cuda.synchronize()
        assert torch.isfinite(lg) and torch.isfinite(ld) and ops.WGRAD_PRECISION == "direct"
        assert "hipGraph" in tr.step_mode, tr.step_mode
        return hook.kinds

    k = step("direct")
    assert k and "wgrad_winograd" not in k, k
    k = step("winograd")
    assert "wgrad_winograd" in k, k
    assert step("winograd") == []                    # a replay: no launch goes through the hook
    k = step("direct")
    assert k and "wgrad_winograd" not in k, k
    assert step("direct") == []
    assert int(tr.optimizer_G.t_dev.item()) == 5 and int(tr.optimizer_D.t_dev.item()) == 5
    assert torch.isfinite(tr.optimizer_G.flat).all()
