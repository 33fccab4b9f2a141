"""The opt-in F(4x4, 3x3) Winograd forward / data gradient of the training step (TrainOpts.conv_tiles = "4x4", ops.train_conv_tiles("4x4"))
on the GPU: the split-K form of csrc/conv_winograd4.hip against an fp64 convolution, the batched panel builder against the single launches, then every
layer above - ConvFn, the generator's training gradients, the trainer's eager and captured steps.  Shapes are (B, H, W, C0, C1, N)."""
import contextlib
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from ipercore_amd import _lib, ops
from ipercore_amd.networks import packing, training
from tests import gpu_checks as gc
from tests.gpu_checks import DEV, _rand

pytestmark = pytest.mark.gpu

# every case runs split over K (asserted through lwg_conv2d_winograd4_plan: a threshold change must not quietly make one a whole-K test)
SPLIT = {
    "one_tile": (1, 16, 32, 128, 0, 64),                 # 16 stages: 8 + 8
    "ragged_image_ragged_last_slice": (1, 17, 31, 160, 0, 128),      # 20 stages: 8 + 8 + 4
    "one_row": (1, 1, 33, 96, 0, 64),                    # 12 stages: 8 + 4
    "one_row_no_bias": (1, 1, 33, 96, 0, 64),
    "two_images_four_slices": (2, 8, 8, 256, 0, 256),
    "two_images_four_slices_no_bias": (2, 8, 8, 256, 0, 256),
    "two_inputs_boundary_at_the_inputs": (1, 32, 32, 64, 64, 64),
    "two_inputs_boundary_inside_an_input": (1, 19, 18, 72, 56, 64),
}
MASK = (2, 21, 19, 256, 0, 64)
ADV = (1, 32, 32, 256, 0, 256)


class _Hook:
    """ops.CONV_HOOK recorder: (kind, kernels) of the closing calls."""

    def __init__(self):
        self.infos = []

    def __call__(self, begin, M, spec, epi=0, info=None):
        if not begin:
            self.infos.append((info["kind"], info["kernels"]))

    @property
    def kinds(self):
        return [k for k, _ in self.infos]

    def __enter__(self):
        self.prev, ops.CONV_HOOK = ops.CONV_HOOK, self
        return self

    def __exit__(self, *exc):
        ops.CONV_HOOK = self.prev


@contextlib.contextmanager
def _every_launch():
    """The size thresholds of ops._wino4_plan / _wino_plan off: the small launches of these tests take the Winograd kernels in either mode."""
    prev = ops.WINO4_TRAIN_MIN_GRID, ops.WINO4_TRAIN_MIN_SLICE_CIN, ops.WINO_MIN_GRID
    ops.WINO4_TRAIN_MIN_GRID = ops.WINO4_TRAIN_MIN_SLICE_CIN = ops.WINO_MIN_GRID = 0
    try:
        yield
    finally:
        ops.WINO4_TRAIN_MIN_GRID, ops.WINO4_TRAIN_MIN_SLICE_CIN, ops.WINO_MIN_GRID = prev


def _rel(got, ref):
    return float((got.double().cpu() - ref.double()).norm() / ref.double().norm())


@functools.lru_cache(maxsize=None)
def _case(shape, bias=True, seed=940):
    """Operands (CPU, fp32, unchanged by their users) and the fp64 convolution of one case, computed once."""
    B, H, W, C0, C1, N = shape
    Cin = C0 + C1
    w = _rand((N, Cin, 3, 3), seed, (Cin * 9) ** -0.5)
    b = _rand((N,), seed + 1, 0.1) if bias else None
    x = _rand((B, H, W, Cin), seed + 2)
    want = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), None if b is None else b.double(), padding=1).permute(0, 2, 3, 1).contiguous()
    return w, b, x, want


def _slices(x0, spec, y, **kw):
    a = ops.conv_args(x0, spec, y, **kw)
    sl = ctypes.c_int(-1)
    assert _lib.lib().lwg_conv2d_winograd4_plan(a, 1, None, ctypes.byref(sl), None, None) == 0
    assert _lib.lib().lwg_conv2d_winograd4_ws_floats(a) == sl.value * a.M * a.N
    return sl.value


def _run(shape, w, b, x, tiles, direct=False, **kw):
    """One training launch (splitk=True) of the layer -> (y, hook infos, K slices of the F(4x4) plan); direct: the "fp32" engine instead."""
    B, H, W, C0, C1, N = shape
    spec = gc._spec_dev(packing.pack_conv(w, b, stride=1, pad=1))
    xd = x.to(DEV)
    x0 = xd[..., :C0].contiguous()
    x1 = xd[..., C0:].contiguous() if C1 else None
    y = torch.full((B, H, W, N), float("nan"), device=DEV)
    with _every_launch(), ops.conv_precision("fp32" if direct else "winograd"), ops.train_conv_tiles(tiles), _Hook() as hook:
        ops.conv2d(x0, spec, y, x1=x1, splitk=True, **kw)
    torch.cuda.synchronize()
    return y, hook.infos, _slices(x0, spec, y, x1=x1, **kw)


@pytest.mark.parametrize("tag", list(SPLIT))
def test_split_kernel_against_fp64(tag):
    """check_winograd4's own bounds (max error 1e-4 of the reference's scale, relative L2 <= 2e-5); neither the F(2x2, 3x3) nor the direct kernel's
    bits, and the hook reports the F(4x4) launch with its finishing kernel: the split kernel really ran."""
    shape = SPLIT[tag]
    w, b, x, want = _case(shape, bias="no_bias" not in tag)
    y4, infos, slices = _run(shape, w, b, x, "4x4")
    assert slices >= 2, (tag, slices)
    assert infos == [("winograd4", 2)], infos
    m = gc._cmp(y4, want.float(), 1e-4, "F(4x4,3x3) split-K " + tag)
    rel = _rel(y4, want)
    print(f"train_conv_tiles {tag} {shape}: {slices} slices, max abs {m['max_abs']:.3e}, rel L2 vs fp64 {rel:.3e}")
    assert rel <= 2e-5, (tag, rel)
    y2, infos2, _ = _run(shape, w, b, x, "2x2")
    assert infos2[0][0] == "winograd" and torch.isfinite(y2).all() and not torch.equal(y4, y2), (tag, infos2)
    if shape[4] == 0 or shape[3] % 32 == 0:                  # (the direct kernel's skip concatenation wants C0 % 32 == 0)
        yd, infosd, _ = _run(shape, w, b, x, "2x2", direct=True)
        assert infosd[0][0] == "direct" and not torch.equal(y4, yd), (tag, infosd)


def test_split_relu_mask_data_gradient():
    """y = res > 0 ? conv + bias : 0 through the slabs and the finishing kernel, against the direct kernel: zeros in the same places."""
    w, b, x, _ = _case(MASK, seed=950)
    res = _rand(MASK[:3] + (MASK[5],), 953).to(DEV)
    kw = dict(epi=ops.EPI_RESIDUAL, act=ops.ACT_RELU_MASK, res=res)
    y4, infos, slices = _run(MASK, w, b, x, "4x4", **kw)
    yd, _, _ = _run(MASK, w, b, x, "2x2", direct=True, **kw)
    assert slices >= 2 and infos == [("winograd4", 2)], (slices, infos)
    gc._cmp(y4, yd.cpu(), 1e-4, "F(4x4,3x3) split-K, ReLU-mask epilogue")
    assert not torch.equal(y4, yd) and torch.equal(y4 == 0, yd == 0)
    assert float((y4 == 0).float().mean()) > 0.3


@pytest.mark.parametrize("kind", gc.ADV_KINDS)
def test_split_adversarial_operands(kind):
    """Relative L2 error against fp64 at most 6x the direct kernel's on the same operands: the "f43" bound of gpu_checks._WINO_FORMS, against that
    check's own yardstick - the direct kernel as gpu_checks.check_winograd_adversarial launches it (ops.conv2d in the "fp32" engine, the K loop whole),
    on that check's operands for this shape.  (The direct kernel's split-K form, which a training launch of this shape would take, adds its slabs
    pairwise and is closer to fp64 than the whole loop - 2.2 - 3.1e-7 against 5.4e-7 - 1.2e-6; its figure is printed beside.  Measured ratios against
    the yardstick: 0.21 - 2.44; against the split-K form they would be 0.6 - 6.6, student_t_w at 6.05 and hot_channel at 6.6.)"""
    bar = dict((f, b) for f, _, b in gc._WINO_FORMS)["f43"]
    B, H, W, C, _, N = ADV
    w, x = gc._adversarial_operands(kind, C, (N, C, 3, 3), (B, H, W, C), 400 + C)
    b = _rand((N,), 401, 0.1)
    want = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), padding=1).permute(0, 2, 3, 1)
    y4, infos, slices = _run(ADV, w, b, x, "4x4")
    ys, _, _ = _run(ADV, w, b, x, "2x2", direct=True)
    yd = torch.empty(B, H, W, N, device=DEV)
    ops.conv2d(x.to(DEV), gc._spec_dev(packing.pack_conv(w, b, stride=1, pad=1)), yd)
    torch.cuda.synchronize()
    assert slices >= 2 and infos == [("winograd4", 2)], (slices, infos)
    assert torch.isfinite(y4).all() and not torch.equal(y4, yd)
    e4, ed, es = _rel(y4, want), _rel(yd, want), _rel(ys, want)
    print(f"train_conv_tiles adversarial {kind}: rel L2 vs fp64 split F(4x4) {e4:.3e} direct {ed:.3e} ratio {e4 / ed:.2f} (direct split-K {es:.3e})")
    assert e4 <= bar * ed, (kind, e4, ed)


def test_split_deterministic():
    """The slabs are added in slice order, no float atomics: the same split launch twice is bitwise equal."""
    shape = SPLIT["ragged_image_ragged_last_slice"]
    w, b, x, _ = _case(shape)
    a, _, slices = _run(shape, w, b, x, "4x4")
    c, _, _ = _run(shape, w, b, x, "4x4")
    assert slices >= 2 and torch.equal(a, c)


def test_batched_panels_equal_the_single_launches():
    """lwg_winograd4_panels_f32 on a device table of three records - a plain panel, one with a permuted tap order, a data-gradient (transposed) panel -
    is bitwise lwg_winograd4_panel_f32 per panel."""
    L = _lib.lib()
    w1, w2, w3 = _rand((64, 96, 3, 3), 960, 0.05), _rand((128, 64, 3, 3), 961, 0.05), _rand((96, 64, 3, 3), 962, 0.05)
    s1 = gc._spec_dev(packing.pack_conv(w1, None, stride=1, pad=1))
    s2 = gc._spec_dev(packing.pack_conv(w2, None, stride=1, pad=1))
    s2.dy, s2.dx = s2.dy[::-1], s2.dx[::-1]
    s3 = packing.pack_dgrad_conv(w3.to(DEV), stride=1, pad=1, n_pad=128, cin_pad=64)[0]       # Cin = 128 (dY's channels), N = 64
    specs = [s1, s2, s3]
    single, batched, rows = [], [], []
    for s in specs:
        cin, N, tap9 = ops._wino_panel_source(s)
        U = torch.full((4, cin // 8, 4, 2, 9 * N), float("nan"), device=DEV)
        ops._lib.check(L.lwg_winograd4_panel_f32(s.w.data_ptr(), U.data_ptr(), cin, N, tap9, ops._stream()), "lwg_winograd4_panel_f32")
        single.append(U)
        V = torch.full_like(U, float("nan"))
        batched.append(V)
        rows.append((s.w.data_ptr(), V.data_ptr(), cin, N, tuple(tap9)))
    assert rows[1][4] == tuple(reversed(rows[0][4])) and (rows[2][2], rows[2][3]) == (128, 64)
    descs = (_lib.LwgWinoDesc * len(rows))()
    first = 0
    for d, (wp, up, cin, N, tap9) in zip(descs, rows):
        d.wpanel, d.upk, d.Cin, d.N, d.first_block = wp, up, cin, N, first
        for i in range(9):
            d.tap9[i] = tap9[i]
        first += ((N + 63) // 64) * ((cin + 3) // 4)
    table = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(DEV)
    ops._lib.check(L.lwg_winograd4_panels_f32(table.data_ptr(), len(rows), first, ops._stream()), "lwg_winograd4_panels_f32")
    torch.cuda.synchronize()
    for U, V in zip(single, batched):
        assert torch.isfinite(U).all() and torch.equal(U, V)


def _convfn_case(tag):
    """(x0, x1, w, b, upstream gradient, ConvFn keywords, fp64 autograd results) of one layer."""
    if tag == "plain":
        C0, C1, N, kw = 128, 0, 64, dict(act=ops.ACT_RELU)
    elif tag == "mask_dx":
        C0, C1, N, kw = 128, 0, 128, dict(mask_dx=True)
    else:
        C0, C1, N, kw = 64, 64, 64, dict(act=ops.ACT_RELU)
    B, H, W = 1, 16, 32
    x = _rand((B, H, W, C0 + C1), 970)
    if tag == "mask_dx":
        x = x.relu()                                         # the input is a ReLU layer's output: its zeros are the mask
    w, b, up = _rand((N, C0 + C1, 3, 3), 971, ((C0 + C1) * 9) ** -0.5), _rand((N,), 972, 0.1), _rand((B, H, W, N), 973)
    xr, wr, br = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    y = F.conv2d(xr.permute(0, 3, 1, 2), wr, br, padding=1).permute(0, 2, 3, 1)
    if kw.get("act") == ops.ACT_RELU:
        y = y.relu()
    y.backward(up.double())
    dx = xr.grad * (x > 0) if tag == "mask_dx" else xr.grad
    return x, C0, C1, w, b, up, kw, (y.detach(), dx, wr.grad, br.grad)


@pytest.mark.parametrize("tag", ["plain", "mask_dx", "two_inputs"])
def test_convfn_forward_and_gradients(tag):
    """ConvFn under ops.train_conv_tiles("4x4"): y, dx, dw and db against fp64 autograd (the kernel-level bounds above on y and dx: 1e-4 of the
    scale, relative L2 2e-5; dw and db come from the unchanged weight-gradient kernels), the hook shows kind "winograd4" for the forward and the
    data-gradient launch - and none with the switch off, where the same calls keep the parent's kinds."""
    x, C0, C1, w, b, up, kw, (y_ref, dx_ref, dw_ref, db_ref) = _convfn_case(tag)

    def run(tiles):
        xd = x.to(DEV).requires_grad_(True)
        wd, bd = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
        with _every_launch(), ops.conv_precision("winograd"), ops.train_conv_tiles(tiles), _Hook() as hook:
            if C1:
                x0, x1 = xd[..., :C0], xd[..., C0:]
                y = training.conv(x0.contiguous(), wd, bd, x1=x1.contiguous(), stride=1, pad=1, **kw)
            else:
                y = training.conv(xd, wd, bd, stride=1, pad=1, **kw)
            y.backward(up.to(DEV))
        torch.cuda.synchronize()
        return y.detach(), xd.grad, wd.grad, bd.grad, hook.kinds

    y4, dx4, dw4, db4, k4 = run("4x4")
    y2, dx2, dw2, db2, k2 = run("2x2")
    assert k4.count("winograd4") == 2 and "winograd" not in k4, k4
    assert "winograd4" not in k2 and k2.count("winograd") == 2, k2
    for name, got, ref in (("y", y4, y_ref), ("dx", dx4, dx_ref)):
        gc._cmp(got, ref.float(), 1e-4, f"ConvFn {tag} {name}")
        assert _rel(got, ref) <= 2e-5, (tag, name, _rel(got, ref))
    assert not torch.equal(y4, y2) and not torch.equal(dx4, dx2)
    if tag == "mask_dx":
        assert torch.equal(dx4 == 0, dx2 == 0)
    for name, got, ref in (("dw", dw4, dw_ref), ("db", db4, db_ref)):
        assert _rel(got, ref) <= 2e-5, (tag, name, _rel(got, ref))


def test_convfn_on_the_shipped_plan():
    """One layer the shipped thresholds of ops._wino4_plan take, 2 x 64 x 64, 256 -> 256 (128 blocks of 32 channels, two slices of 128 input
    channels), through ConvFn with NO threshold touched: forward and data gradient run the split F(4x4) launch (kind "winograd4", two kernels
    each) and meet the kernel-level bounds against fp64 autograd; with the switch off the same call shows the F(2x2) kernel."""
    B, H, W, C, N = 2, 64, 64, 256, 256
    x, w, b, up = _rand((B, H, W, C), 980), _rand((N, C, 3, 3), 981, (C * 9) ** -0.5), _rand((N,), 982, 0.1), _rand((B, H, W, N), 983)
    xr, wr = x.double().requires_grad_(True), w.double()
    y_ref = F.conv2d(xr.permute(0, 3, 1, 2), wr, b.double(), padding=1).permute(0, 2, 3, 1)
    y_ref.backward(up.double())

    def run(tiles):
        xd = x.to(DEV).requires_grad_(True)
        wd, bd = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
        with ops.conv_precision("winograd"), ops.train_conv_tiles(tiles), _Hook() as hook:
            y = training.conv(xd, wd, bd, stride=1, pad=1)
            y.backward(up.to(DEV))
        torch.cuda.synchronize()
        return y.detach(), xd.grad, hook.infos

    y4, dx4, i4 = run("4x4")
    y2, dx2, i2 = run("2x2")
    assert i4 == [("winograd4", 2), ("winograd4", 2)], i4
    assert [k for k, _ in i2] == ["winograd", "winograd"], i2
    for name, got, ref in (("y", y4, y_ref.detach()), ("dx", dx4, xr.grad)):
        gc._cmp(got, ref.float(), 1e-4, f"ConvFn shipped plan {name}")
        assert _rel(got, ref) <= 2e-5, (name, _rel(got, ref))
    assert not torch.equal(y4, y2) and not torch.equal(dx4, dx2)


def test_generator_training_grads_with_the_switch_on():
    """gpu_checks._generator_training_grads at its smallest configuration inside ops.train_conv_tiles("4x4"): the helper's own bounds against the
    oracle hold unchanged, and the F(4x4) kernel really ran."""
    with _every_launch(), ops.train_conv_tiles("4x4"), _Hook() as hook:
        m = gc._generator_training_grads(64, [64, 64, 128], 2, [64, 64, 128], precisions=("winograd",), wino_min_grid=0)
    assert "winograd4" in hook.kinds
    print("train_conv_tiles generator grads:", m["worst_rel_grad_err"], m["worst_param"], hook.kinds.count("winograd4"), "F(4x4) launches")


TR = dict(S=64, ns=2, nf=[64, 64, 128], nres=2, bgf=[64, 64, 128])      # gpu_checks.check_graph_vs_eager_steps' configuration


@functools.lru_cache(maxsize=None)
def _trainer_setup():
    """(inputs, generator state dict) shared by the trainer tests; their users clone / copy, never write."""
    from ipercore_amd import synthetic
    from ipercore_amd.networks import generator_param_shapes
    S, ns, nf, nres, bgf = (TR[k] for k in ("S", "ns", "nf", "nres", "bgf"))
    u = lambda shape, seed, name: torch.tensor(synthetic.uniform_image(shape, seed, name), device=DEV)      # noqa: E731
    bg_in, src_in, tsf_in, Tst = gc._training_inputs(S, ns, nf, nres, bgf, False)
    inp = {"input_G_bg": bg_in.to(DEV), "input_G_src": src_in.to(DEV), "input_G_tsf": tsf_in.to(DEV), "Tst": Tst.to(DEV),
           "real_src": u((1, ns, 3, S, S), 700, "real_src"), "real_tsf": u((1, 1, 3, S, S), 701, "real_tsf"),
           "real_bg": u((1, 3, S, S), 702, "real_bg"), "body_mask": (u((1, ns + 1, 1, S, S), 703, "mask") > 0).float()}
    return inp, synthetic.fill_state_dict(generator_param_shapes(nf, nres, bgf), seed=7)


def _new_trainer(tiles, use_graph):
    from ipercore_amd.networks import NetworksFactory
    from ipercore_amd.trainers import LWGTrainer, PatchGlobalDiscriminator, TrainOpts
    inp, sdn = _trainer_setup()
    G = NetworksFactory.get_by_name("AttLWB-SPADE", cfg=gc.pu.gen_cfg(TR["nf"], TR["nres"], TR["bgf"]), temporal=False)
    G.load_state_dict({k: torch.tensor(v) for k, v in sdn.items()}, strict=True)
    G.to(DEV).train()
    torch.manual_seed(0)
    D = PatchGlobalDiscriminator().to(DEV)
    opts = TrainOpts.l1_transfer()
    opts.use_graph, opts.conv_tiles = use_graph, tiles
    tr = LWGTrainer(G, D, opts=opts)
    tr.set_input({k: v.clone() for k, v in inp.items()})
    return tr


def test_trainer_captured_against_eager():
    """Two LWGTrainer steps at 64^2 with TrainOpts.conv_tiles = "4x4", captured against eager, held to the bounds of
    test_gpu_wgrad_winograd.py::test_trainer_captured_against_eager (gpu_checks._graph_vs_eager_steps'); the F(4x4) kernel ran - on training and on
    frozen weights, through the panel cache's per-step refresh - and the switch is back at "2x2" after every step."""
    N, runs = 2, {}
    with _every_launch():
        for mode in ("eager", "graph"):
            tr = _new_trainer("4x4", mode == "graph")
            with _Hook() as hook:
                hist = [tr.optimize_parameters() for _ in range(N)]
            torch.cuda.synchronize()
            assert ops.TRAIN_CONV_TILES == "2x2"
            assert "winograd4" in hook.kinds, mode
            assert tr._panel_cache.wino4_rows and tr._panel_cache.wino4_table is not None, mode
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


def test_one_captured_trainer_switches_modes_and_leaves_nothing_behind():
    """2x2 -> 4x4 -> 2x2 on ONE captured trainer: the convolution kernels are frozen into the graph, so each switch re-captures the step (the hook
    sees the launches of a capture, and none of a replay) with the kernels of the new mode, and the step stays a hipGraph.  Around it, a fresh
    "2x2" trainer's first step before the mode ran against one after it: both losses, the discriminator's weights and the hook's kind sequence are
    bitwise equal.  (The generator's updated weights are not compared run against run: most of its gradients pass through the fp32 atomics of the
    attention / warp backward, which two default first steps do not reproduce bitwise with no mode ever entered - DESIGN 3.10b.)"""
    def first_default_step():
        tr = _new_trainer("2x2", False)
        with _Hook() as hook:
            lg, ld = tr.optimize_parameters()
        torch.cuda.synchronize()
        return float(lg), float(ld), tr.optimizer_D.flat.clone(), hook.kinds

    before = first_default_step()
    assert before[3] and "winograd4" not in before[3]
    tr = _new_trainer("2x2", True)

    def step(tiles):
        tr.opts.conv_tiles = tiles
        with _Hook() as hook:
            lg, ld = tr.optimize_parameters()
        torch.cuda.synchronize()
        assert torch.isfinite(lg) and torch.isfinite(ld) and ops.TRAIN_CONV_TILES == "2x2"
        assert "hipGraph" in tr.step_mode, tr.step_mode
        return hook.kinds

    k0 = step("2x2")
    assert k0 and "winograd4" not in k0, k0
    assert not tr._panel_cache.wino4_rows
    with _every_launch():
        k = step("4x4")
        assert "winograd4" in k, k
        assert tr._panel_cache.wino4_rows
        assert step("4x4") == []                     # a replay: no launch goes through the hook
    k = step("2x2")
    assert k == k0 and "winograd4" not in k, (k0, k)     # the re-captured "2x2" step of the trainer that ran "4x4": the parent's kind sequence ...
    assert not tr._panel_cache.wino4_rows and not tr._panel_cache.wino4                  # ... and no F(4x4) panel left in its per-step refresh
    assert step("2x2") == []
    assert int(tr.optimizer_G.t_dev.item()) == 5 and int(tr.optimizer_D.t_dev.item()) == 5
    assert torch.isfinite(tr.optimizer_G.flat).all()
    after = first_default_step()
    assert after[3] == before[3], (before[3], after[3])
    assert (before[0], before[1]) == (after[0], after[1]), (before[:2], after[:2])
    assert torch.equal(before[2], after[2])
