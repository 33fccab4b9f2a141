"""The opt-in bf16-operand weight gradient (csrc/conv_wgrad_bf16.hip, ops.wgrad_mode("bf16")) on the GPU: the kernel against the
two derived bounds of tests/wgradbf16_emu.py (accumulation: against the fp64 gradient of the bf16-rounded operands; rounding: against the fp64
gradient of the operands as given) with the direct kernel (lwg_conv2d_wgrad_unpacked_f32) on the same operands next to it, then every layer above
it - packing.wgrad_conv / wgrad_conv_transpose, ConvFn, the trainer's eager and captured steps."""
import functools

import pytest
import torch

from ipercore_amd import ops
from ipercore_amd.networks import packing, training
from tests import gpu_checks as gc
from tests import wgradbf16_emu as emu
from tests.gpu_checks import DEV, _rand

pytestmark = pytest.mark.gpu


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


def _ids(v):
    return "x".join(map(str, v[0])) + "_k%ds%d" % v[1][:2] if isinstance(v, tuple) and isinstance(v[0], tuple) else str(v)


@functools.lru_cache(maxsize=None)
def _case(case, kind="randn"):
    """Operands (CPU, fp32, unchanged by their users), the fp64 references and the two bounds of one case, computed once."""
    shape, geom, drop = case
    x, dy, cin, nout = emu.case(shape, geom, drop, kind)
    xs, dys = x[..., :cin], dy[..., :nout]
    return x, dy, cin, nout, emu.reference(xs, dys, *geom), emu.rounded_reference(xs, dys, *geom), emu.bounds(xs, dys, *geom)


def _run_both(case, x, dy, cin, nout, want_db=False):
    """-> (bf16 dw, direct dw, hook kinds of the bf16 launch, bf16 db), the gradients (nout, cin, k, k) pre-filled with NaN."""
    (B, H, W, C0, C1, N), (k, stride, pad), _ = case
    w = _rand((nout, cin, k, k), 5, 0.05)
    spec = gc._spec_dev(packing.pack_conv(w, None, stride=stride, pad=pad, cin_pad=C0 + C1, n_pad=N))
    xd, dyd = x.to(DEV), dy.to(DEV)
    x0 = xd[..., :C0].contiguous()
    x1 = xd[..., C0:].contiguous() if C1 else None
    assert ops._wgrad_bf16_use(x0, spec, dyd, x1)
    dwb = torch.full((nout, cin, k, k), float("nan"), device=DEV)
    dwd = torch.full((nout, cin, k, k), float("nan"), device=DEV)
    db = torch.full((nout,), float("nan"), device=DEV) if want_db else None
    with _Kinds() as hook:
        ops.conv2d_wgrad_bf16(x0, spec, dyd, dwb, False, range(k * k), cin, nout, x1=x1, db=db)
    ops.conv2d_wgrad_unpacked(x0, spec, dyd, dwd, False, range(k * k), cin, nout, x1=x1)
    torch.cuda.synchronize()
    return dwb, dwd, hook.kinds, db


def _check_bounds(tag, got, ref, rref, bnds, direct=None):
    """Finite and inside both derived bounds, element by element; not the direct kernel's bits.  Prints the figures before it asserts."""
    acc, rnd = bnds
    g = got.double().cpu()
    ea, er = (g - rref).abs(), (g - ref).abs()
    fa, fr = float((ea / acc.clamp_min(1e-300)).max()), float((er / rnd.clamp_min(1e-300)).max())
    line = f"wgrad_bf16 {tag}: err / accumulation bound {fa:.3e}, err / rounding bound {fr:.3e}, rel L2 vs fp64 bf16 {_rel(got, ref):.3e}"
    if direct is not None:
        line += f" direct {_rel(direct, ref):.3e}, bf16 vs direct {_rel(got, direct.double().cpu()):.3e}"
    print(line)
    assert torch.isfinite(got).all(), tag
    if direct is not None:
        assert torch.isfinite(direct).all() and not torch.equal(got, direct), tag
    assert bool((ea <= acc).all()), (tag, fa)
    assert bool((er <= rnd).all()), (tag, fr)


@pytest.mark.parametrize("case", emu.MATRIX, ids=_ids)
def test_kernel_inside_both_bounds(case):
    x, dy, cin, nout, ref, rref, bnds = _case(case)
    dwb, dwd, kinds, _ = _run_both(case, x, dy, cin, nout)
    assert kinds == ["wgrad_bf16"], kinds
    _check_bounds(str(case), dwb, ref, rref, bnds, direct=dwd)


def _convt_operands():
    w = _rand((64, 64, 4, 4), 50, 0.05).to(DEV)
    specs = [gc._spec_dev(s) for s in packing.pack_conv_transpose(w, None)]
    adj = gc._spec_dev(packing.pack_dgrad_conv_transpose(w, n_pad=64)[0])
    return specs, adj, _rand((1, 8, 8, 64), 51), _rand((1, 16, 16, 64), 52)


def test_transposed_conv_adjoint_form():
    """nn.ConvTranspose2d(4, 2, 1), x (1, 8, 8, 64), dy (1, 16, 16, 64), through packing.wgrad_conv_transpose(adj_spec=...): the same entry point with
    the roles swapped and a permuted kidx, against conv_transpose2d's own weight gradient in fp64."""
    specs, adj, x, dy = _convt_operands()
    xd, dyd = x.to(DEV), dy.to(DEV)
    want = packing.wgrad_conv_transpose(xd, specs, dyd, 64, 64, adj_spec=adj)
    with ops.wgrad_mode("bf16"), _Kinds() as hook:
        got = packing.wgrad_conv_transpose(xd, specs, dyd, 64, 64, adj_spec=adj)
    torch.cuda.synchronize()
    assert hook.kinds == ["wgrad_bf16"], hook.kinds
    assert tuple(got.shape) == (64, 64, 4, 4)
    _check_bounds("conv_transpose 4x4 s2", got, emu.convt_weight(x, dy), emu.convt_weight(emu.rounded(x), emu.rounded(dy)), emu.convt_bounds(x, dy),
                  direct=want)


@pytest.mark.parametrize("kind", emu.KINDS)
def test_operand_kinds(kind):
    case = emu.KINDS_SHAPE
    x, dy, cin, nout, ref, rref, bnds = _case(case, kind)
    dwb, dwd, _, _ = _run_both(case, x, dy, cin, nout)
    _check_bounds(kind, dwb, ref, rref, bnds, direct=dwd)


def test_deterministic():
    """Slabs are added in slab order, no float atomics: three launches of the many-slab case are bitwise equal."""
    x, dy, cin, nout = _case(emu.BIG)[:4]
    outs = [_run_both(emu.BIG, x, dy, cin, nout)[0] for _ in range(3)]
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_fused_bias_gradient():
    """db rides along as in the direct kernel - fp32 column sums of dy as loaded, before rounding: relative L2 against fp64 <= 1e-6 at
    (2, 16, 16, 64 -> 128), the criterion of the ConvFn test of the column-sum kernel."""
    case = ((2, 16, 16, 64, 0, 128), (3, 1, 1), None)
    x, dy, cin, nout, ref, rref, bnds = _case(case)
    dwb, _, kinds, db = _run_both(case, x, dy, cin, nout, want_db=True)
    assert kinds == ["wgrad_bf16"]
    e = _rel(db, dy.double().sum(dim=(0, 1, 2)))
    print(f"wgrad_bf16 fused db: rel L2 vs fp64 {e:.3e}")
    assert torch.isfinite(db).all() and e <= 1e-6
    _check_bounds("with db", dwb, ref, rref, bnds)


def _ineligible_cases():
    """name -> callable() -> weight gradient through packing / training; none is a launch of the new kernel."""
    def first_layer():
        w = _rand((64, 6, 3, 3), 30, 0.05).to(DEV)
        spec = gc._spec_dev(packing.pack_conv(w, None, stride=1, pad=1, cin_pad=8))
        x, dy = _rand((2, 8, 8, 8), 31).to(DEV), _rand((2, 8, 8, 64), 32).to(DEV)
        return lambda: packing.wgrad_conv(x, spec, dy, None, 3, 3, 6, 64)

    def thin():
        w = _rand((3, 64, 5, 5), 40, 0.05).to(DEV)
        x, dy = _rand((1, 16, 16, 64), 41).to(DEV), _rand((1, 16, 16, 4), 42).to(DEV)
        return lambda: training.thin_backward(x, w, dy, 2, False, True)[1]

    def convt_four_parities():
        specs, _, x, dy = _convt_operands()
        xd, dyd = x.to(DEV), dy.to(DEV)
        return lambda: packing.wgrad_conv_transpose(xd, specs, dyd, 64, 64)

    return {"first_layer_6_to_64": first_layer(), "thin_5x5": thin(), "conv_transpose_four_parities": convt_four_parities()}


def test_ineligible_launches_keep_the_default_path():
    for name, fn in _ineligible_cases().items():
        with _Kinds() as h0:
            want = fn()
        with ops.wgrad_mode("bf16"), _Kinds() as h1:
            got = fn()
        torch.cuda.synchronize()
        assert torch.isfinite(want).all() and torch.equal(got, want), name
        assert h1.kinds == h0.kinds and "wgrad_bf16" not in h1.kinds, (name, h0.kinds, h1.kinds)


def test_convfn_weight_bias_and_data_gradients():
    """One 3x3 layer with bias, (2, 16, 16, 64 -> 128), forward then backward in the mode: weight.grad inside both bounds, bias.grad (still fused, fp32)
    to 1e-6 of the fp64 column sums, the output and the data gradient bitwise those of the default mode."""
    x = _rand((2, 16, 16, 64), 60)
    w, b = _rand((128, 64, 3, 3), 61, 0.05), _rand((128,), 62, 0.1)
    up = _rand((2, 16, 16, 128), 63)

    def run(mode):
        xd = x.to(DEV).requires_grad_(True)
        wd, bd = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
        with ops.wgrad_mode(mode), _Kinds() as hook:
            y = training.conv(xd, wd, bd, stride=1, pad=1)
            y.backward(up.to(DEV))
        torch.cuda.synchronize()
        return wd.grad, bd.grad, xd.grad, y.detach(), hook.kinds

    gw0, gb0, gx0, y0, k0 = run("direct")
    gw1, gb1, gx1, y1, k1 = run("bf16")
    assert "wgrad_bf16" in k1 and "wgrad_bf16" not in k0, (k0, k1)
    assert [k for k in k1 if k != "wgrad_bf16"] == k0, (k0, k1)            # no column-sum launch joins: the bias gradient stays fused
    _check_bounds("ConvFn 64->128", gw1, emu.reference(x, up), emu.rounded_reference(x, up), emu.bounds(x, up), direct=gw0)
    assert _rel(gb1, up.double().sum(dim=(0, 1, 2))) <= 1e-6
    assert torch.equal(y1, y0) and torch.equal(gx1, gx0)


TR = dict(S=64, ns=2, nf=[64, 64, 128], nres=2, bgf=[64, 64, 128])      # tests/test_gpu_wgrad_winograd.py's (gpu_checks.check_graph_vs_eager_steps')


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


def _new_trainer(wgrad, use_graph):
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
    tr = LWGTrainer(G, D, opts=opts)
    tr.set_input({k: v.clone() for k, v in inp.items()})
    return tr


class _EligibleLaunches:
    """Records (arguments, result) of every packing.wgrad_conv / wgrad_conv_transpose call whose launch the bf16 mode would take."""

    def __init__(self):
        self.calls = []

    def __enter__(self):
        self.orig = orig_c, orig_t = packing.wgrad_conv, packing.wgrad_conv_transpose
        cl = lambda t: None if t is None else t.clone()      # noqa: E731

        def spy_conv(x0, spec, dy, x1, kh, kw, cin, n, db=None):
            dw = orig_c(x0, spec, dy, x1, kh, kw, cin, n, db=db)
            if ops._wgrad_bf16_use(x0, spec, dy, x1):
                self.calls.append(("conv", (x0.clone(), spec, dy.clone(), cl(x1), kh, kw, cin, n), db is not None, dw.clone(), cl(db)))
            return dw

        def spy_convt(x0, specs, dy, cin, n, adj_spec=None):
            dw = orig_t(x0, specs, dy, cin, n, adj_spec=adj_spec)
            if adj_spec is not None and ops._wgrad_bf16_use(dy, adj_spec, x0):
                self.calls.append(("convt", (x0.clone(), specs, dy.clone(), cin, n, adj_spec), False, dw.clone(), None))
            return dw

        packing.wgrad_conv, packing.wgrad_conv_transpose = spy_conv, spy_convt
        return self

    def __exit__(self, *exc):
        packing.wgrad_conv, packing.wgrad_conv_transpose = self.orig

    @staticmethod
    def rerun(call, db):
        what, args = call[0], call[1]
        return packing.wgrad_conv(*args, db=db) if what == "conv" else packing.wgrad_conv_transpose(*args[:5], adj_spec=args[5])


def _first_step(mode, record=None):
    """A fresh eager trainer's first step -> (loss G, loss D, D's updated weights, hook kinds)."""
    tr = _new_trainer(mode, False)
    with _Kinds() as hook, (record or _EligibleLaunches()):
        lg, ld = tr.optimize_parameters()
    torch.cuda.synchronize()
    assert ops.WGRAD_PRECISION == "direct"
    return float(lg), float(ld), tr.optimizer_D.flat.clone(), hook.kinds


def test_trainer_captured_against_eager():
    """Two LWGTrainer steps at 64^2 with TrainOpts.wgrad_precision = "bf16", captured against eager, held to the bounds tests/test_gpu_wgrad_winograd.py
    holds its mode to (gpu_checks._graph_vs_eager_steps'); the new kernel ran and the switch is back at "direct" after every step."""
    N, runs = 2, {}
    for mode in ("eager", "graph"):
        tr = _new_trainer("bf16", mode == "graph")
        with _Kinds() as hook:
            hist = []
            for _ in range(N):
                hist.append(tr.optimize_parameters())
                assert ops.WGRAD_PRECISION == "direct"
        torch.cuda.synchronize()
        assert "wgrad_bf16" in hook.kinds, mode
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
        print(f"wgrad_bf16 trainer graph vs eager {k}: max {d.max().item():.3e} mean {d.mean().item():.3e}")
        assert d.max().item() <= 2 * N * lr and d.mean().item() <= 0.1 * lr, (k, d.max().item(), d.mean().item())


def test_first_step_losses_do_not_depend_on_the_mode():
    """The forward runs exactly as in "direct": the first step's two losses in the mode are the default trainer's, bitwise."""
    d, b = _first_step("direct"), _first_step("bf16")
    assert "wgrad_bf16" in b[3] and "wgrad_bf16" not in d[3]
    assert (d[0], d[1]) == (b[0], b[1]), (d[:2], b[:2])


def test_every_eligible_launch_of_a_step_inside_both_bounds():
    """Every launch of a default first step that the mode takes, recorded with its operands, run again through the new entry point (packing in the
    mode) and held to both bounds against fp64 on those operands."""
    rec = _EligibleLaunches()
    _first_step("direct", rec)
    assert len(rec.calls) >= 10 and "conv" in {c[0] for c in rec.calls}, [c[0] for c in rec.calls]
    worst = [0.0, 0.0]
    for call in rec.calls:
        what, args, fused = call[0], call[1], call[2]
        db = torch.full_like(call[4], float("nan")) if fused else None
        with ops.wgrad_mode("bf16"), _Kinds() as hook:
            got = _EligibleLaunches.rerun(call, db)
        torch.cuda.synchronize()
        assert hook.kinds == ["wgrad_bf16"], hook.kinds
        assert torch.isfinite(got).all()
        if what == "conv":
            x0, spec, dy, x1, kh, kw, cin, n = args
            x = (x0 if x1 is None else torch.cat([x0, x1], dim=3))[..., :cin].cpu()
            g = dy[..., :n].cpu()
            geom = (kh, spec.stride, -min(spec.dy))
            ref, rref, (acc, rnd) = emu.reference(x, g, *geom), emu.rounded_reference(x, g, *geom), emu.bounds(x, g, *geom)
            if fused:        # fp32 column sums of T terms, any order: within 2 (T + 8) 2^-24 sum |dy| of the exact sum (these sums cancel: no relative criterion)
                T = g.shape[0] * g.shape[1] * g.shape[2]
                edb = (db.double().cpu() - g.double().sum(dim=(0, 1, 2))).abs()
                assert bool((edb <= 2.0 * (T + 8) * emu.U_ACC * g.double().abs().sum(dim=(0, 1, 2))).all()), float(edb.max())
        else:
            x, g = args[0][..., :args[3]].cpu(), args[2][..., :args[4]].cpu()
            ref, rref, (acc, rnd) = emu.convt_weight(x, g), emu.convt_weight(emu.rounded(x), emu.rounded(g)), emu.convt_bounds(x, g)
        gd = got.double().cpu()
        ea, er = (gd - rref).abs(), (gd - ref).abs()
        worst = [max(worst[0], float((ea / acc.clamp_min(1e-300)).max())), max(worst[1], float((er / rnd.clamp_min(1e-300)).max()))]
        assert bool((ea <= acc).all()) and bool((er <= rnd).all()), (what, tuple(got.shape), worst)
    print(f"wgrad_bf16 trainer launches: {len(rec.calls)} eligible ({sum(c[0] == 'convt' for c in rec.calls)} transposed), worst err / accumulation bound {worst[0]:.3e}, err / rounding bound {worst[1]:.3e}")


def test_the_mode_leaves_nothing_behind():
    """A fresh default trainer's first step before the mode ran against one after it (a captured and an eager bf16 trainer step in between).
    Everything of the step that is a deterministic function of its inputs is held to bitwise equality: both losses, the discriminator's weights,
    the sequence of hook kinds (none of the new kernel), ops.WGRAD_PRECISION - and the weight gradient and fused bias gradient of EVERY launch the
    mode takes over, run again in the default mode on the recorded operands.  The generator's updated weights are not compared run against run:
    most of its gradients pass through the fp32 atomics of the attention / warp backward."""
    rec = _EligibleLaunches()
    before = _first_step("direct", rec)
    assert rec.calls and "wgrad_bf16" not in before[3], (len(rec.calls), before[3])
    for graph in (True, False):
        tr = _new_trainer("bf16", graph)
        with _Kinds() as hook:
            tr.optimize_parameters()
        torch.cuda.synchronize()
        assert "wgrad_bf16" in hook.kinds
    assert ops.WGRAD_PRECISION == "direct"
    after = _first_step("direct")
    assert after[3] == before[3], (before[3], after[3])
    assert (before[0], before[1]) == (after[0], after[1]), (before[:2], after[:2])
    assert torch.equal(before[2], after[2])
    for call in rec.calls:
        fused, dw, db = call[2:]
        db1 = torch.full_like(db, float("nan")) if fused else None
        with _Kinds() as hook:
            dw1 = _EligibleLaunches.rerun(call, db1)
        torch.cuda.synchronize()
        assert hook.kinds == [], hook.kinds                  # the direct weight gradient goes through no hook
        assert torch.equal(dw1, dw), (tuple(dw.shape), float((dw1 - dw).abs().max()))
        assert not fused or torch.equal(db1, db)


def test_one_captured_trainer_switches_modes():
    """direct -> bf16 -> direct on ONE captured trainer: the weight-gradient kernels are frozen into the graph, so each switch re-captures the step
    (the hook sees the launches of a capture, and none of a replay) with the kernels of the new mode, and the step stays a hipGraph."""
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
    assert k and "wgrad_bf16" not in k, k
    k = step("bf16")
    assert "wgrad_bf16" in k, k
    assert step("bf16") == []                        # a replay: no launch goes through the hook
    k = step("direct")
    assert k and "wgrad_bf16" not in k, k
    assert step("direct") == []
    assert int(tr.optimizer_G.t_dev.item()) == 5 and int(tr.optimizer_D.t_dev.item()) == 5
    assert torch.isfinite(tr.optimizer_G.flat).all() and torch.isfinite(tr.optimizer_D.flat).all()
