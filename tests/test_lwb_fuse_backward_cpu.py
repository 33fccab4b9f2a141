"""Training path of the AddLWB / AvgLWB / SoftGateAddLWB / SoftGateAvgLWB generators on the CPU: the contract of
``lwg_lwb_fuse_bwd_f32`` (tests/lwbfuse_emu.py) against fp64 autograd, the entry point's host-side rejections, the whole training
graph and one trainer step through the emulated C ABI against the oracle's autograd, and the oracle against gradients recorded from
the reference's own generator modules (tests/golden/golden_lwb_variant_grads_v1.npz)."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ipercore_amd import _lib, ops, synthetic
from ipercore_amd.networks import NetworksFactory, generator_param_shapes
from oracle import lwg_oracle as orc
from tests import emu_ops, lwbfuse_emu
from tests.test_generator_host import _as_device

KINDS = {"add": "AddLWB", "avg": "AvgLWB", "sg_add": "SoftGateAddLWB", "sg_avg": "SoftGateAvgLWB"}
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def scales(kind, ns):
    """(gated, scale_w, scale_o): the constants generator._attlwb / TrainableGenerator.fuselwb pass for each block."""
    return {"add": (False, 1.0, 1.0), "avg": (False, 1.0, 1.0 / (ns + 1)), "sg_add": (True, 1.0, 1.0), "sg_avg": (True, 1.0 / ns, 1.0)}[kind]


def adversarial_flows(B, ns, S, seed, dtype=torch.float64):
    """(B,ns,S,S,2) flows in grid_sample coordinates: in-range samples, a -2 background band (every tap outside), a band scaled past +-1
    (partial taps at the border) and values exactly +-1 (the tap pair straddling the last pixel's edge); the plain samples keep to the
    left half, so some source rows are reached by no flow."""
    g = torch.Generator().manual_seed(seed)
    T = torch.rand(B, ns, S, S, 2, generator=g, dtype=torch.float64) * 2 - 1
    T[..., 0] = T[..., 0] * 0.5 - 0.5                    # x in [-1, 0]: columns right of the middle stay out of the plain samples' reach
    q = max(1, S // 4)
    T[:, :, :q] = -2.0
    T[:, :, q:2 * q] *= 1.3
    T[:, :, 2 * q, ::2] = 1.0
    T[:, :, 2 * q, 1::2] = -1.0
    T[:, :, 2 * q + 1, ::3, 0] = 1.0
    T[:, :, 2 * q + 1, 1::3, 1] = -1.0
    return T.to(dtype)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("B,ns,h,S,batched", [(1, 2, 12, 12, 1), (2, 3, 6, 16, 1), (3, 2, 5, 12, 0), (2, 1, 8, 8, 0)])
def test_emulation_matches_fp64_autograd(kind, B, ns, h, S, batched):
    """tests/lwbfuse_emu (the per-tap contract the kernel is held to) against fp64 autograd through ``oracle.fuse_lwb``."""
    C = 8
    g = torch.Generator().manual_seed(100 + B * 7 + ns)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)                               # noqa: E731
    tsf = rnd(B, C, h, h).requires_grad_(True)
    src = rnd(B * ns if batched else ns, C, h, h).requires_grad_(True)
    sd = {"p.gate_conv.0.weight": (rnd(C, C, 3, 3) * 0.2).requires_grad_(True), "p.gate_conv.0.bias": (rnd(C) * 0.1).requires_grad_(True),
          "p.gate_conv.2.weight": (rnd(C, C, 3, 3) * 0.2).requires_grad_(True), "p.gate_conv.2.bias": (rnd(C) * 0.1).requires_grad_(True)}
    T = adversarial_flows(B, ns, S, seed=3 + h)
    dout = rnd(B, C, h, h)
    out_ref = orc.fuse_lwb(sd, "p", tsf, src if batched else src.repeat(B, 1, 1, 1), T, kind)
    out_ref.backward(dout)
    want_tsf, want_src = tsf.grad.clone(), src.grad.clone()
    want_w = {k: v.grad.clone() for k, v in sd.items() if v.grad is not None}
    # the same block with the fusion's backward from the emulation: the gate (a function of tsf_x) stays torch autograd
    gated, sw, so = scales(kind, ns)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()                                              # noqa: E731
    tsf2 = tsf.detach().clone().requires_grad_(True)
    sd2 = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    gate = torch.sigmoid(orc._conv(sd2, "p.gate_conv.2", F.relu(orc._conv(sd2, "p.gate_conv.0", tsf2)))) if gated else None
    d_tsf, d_src, d_gate = _as_device(lambda: lwbfuse_emu.lwb_fuse_bwd(
        nhwc(src.detach()), None if gate is None else nhwc(gate.detach()), T, nhwc(dout), src_batched=bool(batched), scale_w=sw, scale_o=so))
    assert (d_gate is None) == (not gated)
    got_tsf = d_tsf.permute(0, 3, 1, 2)
    if gated:
        gate.backward(d_gate.permute(0, 3, 1, 2))
        got_tsf = got_tsf + tsf2.grad
        for k, v in want_w.items():
            assert (sd2[k].grad - v).abs().max().item() <= 1e-10, k
    assert (got_tsf - want_tsf).abs().max().item() <= 1e-10
    assert (d_src.permute(0, 3, 1, 2) - want_src).abs().max().item() <= 1e-10
    # the forward the emulated ABI runs agrees with the oracle's block (same constants)
    out = emu_ops.lwb_fuse(nhwc(tsf.detach()), nhwc(src.detach()), T, torch.empty(B, h, h, C, dtype=torch.float64),
                           gate=None if gate is None else nhwc(gate.detach()), scale_w=sw, scale_o=so, src_batched=bool(batched))
    assert (out.permute(0, 3, 1, 2) - out_ref.detach()).abs().max().item() <= 1e-10


def test_fuse_backward_host_rejections():
    """Every host-side rejection of lwg_lwb_fuse_bwd_f32 returns 1 before any launch (no GPU is touched); ops.lwb_fuse_bwd refuses CPU tensors."""
    L = _lib.lib()
    buf = (ctypes.c_float * 4)()
    bad = ctypes.cast(buf, ctypes.c_void_p)
    f = L.lwg_lwb_fuse_bwd_f32
    ok = dict(src=bad, gate=None, T=bad, dout=bad, d_tsf=bad, d_src=bad, d_gate=None, B=1, ns=2, h=8, w=8, C=64, S=8)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["src"], a["gate"], a["T"], a["dout"], a["d_tsf"], a["d_src"], a["d_gate"], a["B"], a["ns"], a["h"], a["w"], a["C"], a["S"],
                 0, 1.0, 1.0, None)
    for name in ("T", "dout", "d_tsf", "d_src"):
        assert call(**{name: None}) == 1, name
    assert call(gate=bad, d_gate=None) == 1                      # a gate without d_gate
    assert call(gate=bad, d_gate=bad, src=None) == 1             # a gate without the sources its gradient gathers
    for C in (0, 16, 48, 96, 512):
        assert call(C=C) == 1, C
    for name in ("B", "ns", "h", "w", "S"):
        assert call(**{name: 0}) == 1 and call(**{name: -3}) == 1, name
    assert call(ns=65) == 1                                      # ns <= 64
    t = torch.zeros(1, 4, 4, 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.lwb_fuse_bwd(torch.zeros(2, 4, 4, 32), None, torch.zeros(1, 2, 4, 4, 2), t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.lwb_fuse_bwd(torch.zeros(2, 4, 4, 32), t, torch.zeros(1, 2, 4, 4, 2), t, src_batched=True)


def build_generator(kind, nf, nres, bgf, seed=7):
    G = NetworksFactory.get_by_name(KINDS[kind], cfg=synthetic.gen_cfg(nf, nres, bgf), temporal=False)
    sdn = synthetic.fill_state_dict(generator_param_shapes(nf, nres, bgf, lwb="plain" if kind in ("add", "avg") else "softgate"), seed=seed)
    G.load_state_dict({k: torch.tensor(v) for k, v in sdn.items()}, strict=True)
    return G.train(), sdn


def oracle_forward_train(sd, bg_in, src_in, tsf_in, Tst, kind, nf, nres, bgf):
    """forward(bg, src, tsf, Tst, only_tsf=False) of lwb_resunet.py / lwb_softgate_resunet.py on the oracle's pieces."""
    bg = orc.gen_forward_bg(sd, bg_in, n_down=len(bgf), n_res=nres)
    enc, res, s_img, s_mask = orc.gen_forward_src_full(sd, src_in, len(nf), nres)
    imgs, masks = [], []
    for t in range(tsf_in.shape[1]):
        img, mask = orc.gen_forward_tsf(sd, tsf_in[:, t], enc, res, Tst[:, t], len(nf), nres, lwb=kind)
        imgs.append(img)
        masks.append(mask)
    return bg, s_img, s_mask, torch.stack(imgs, dim=1), torch.stack(masks, dim=1)


@pytest.mark.parametrize("kind,nt", [("add", 1), ("avg", 1), ("sg_add", 1), ("sg_avg", 1), ("sg_avg", 2)])
def test_training_graph_of_fuse_generators_cpu(monkeypatch, kind, nt):
    """The whole training graph (bg + src with decoder + tsf: ConvFn / FuseFn / HeadFn, the gate convolutions with their fused ReLU mask)
    through the emulated C ABI against torch autograd through the oracle: the five outputs and EVERY parameter gradient.  nt = 2: the
    source features' gradient accumulates over two target frames."""
    from ipercore_amd.networks.training import TrainableGenerator
    emu_ops.install(monkeypatch)
    monkeypatch.setattr(ops, "lwb_fuse_bwd", lwbfuse_emu.lwb_fuse_bwd)
    S_, ns, nf, nres, bgf = 32, 2, [64, 64, 128], 1, [64, 64, 128]
    G, sdn = build_generator(kind, nf, nres, bgf)
    u = lambda shape, seed, name: torch.tensor(synthetic.uniform_image(shape, seed, name))           # noqa: E731
    bg_in, src_in, tsf_in = u((1, 1, 4, S_, S_), 10, "bg_inputs"), u((1, ns, 6, S_, S_), 8, "src_inputs"), u((1, nt, 6, S_, S_), 9, "tsf_inputs")
    Tst = u((1, nt, ns, S_, S_, 2), 11, "Tst") * 1.1                                                  # some samples leave the image
    tgt = [u(s, 500 + i, "tgt") for i, s in enumerate(((1, 1, 3, S_, S_), (1, ns, 3, S_, S_), (1, ns, 1, S_, S_), (1, nt, 3, S_, S_), (1, nt, 1, S_, S_)))]
    loss_of = lambda outs: sum(((o - t) ** 2).mean() for o, t in zip(outs, tgt))                      # noqa: E731
    sd = {k: torch.tensor(v, requires_grad=True) for k, v in sdn.items()}
    outs_ref = oracle_forward_train(sd, bg_in, src_in, tsf_in, Tst, kind, nf, nres, bgf)
    loss_of(outs_ref).backward()

    def run():
        outs = TrainableGenerator(G).forward(bg_in, src_in, tsf_in, Tst)
        loss_of(outs).backward()
        return outs
    outs = _as_device(run)
    for name, a_, b_ in zip(("bg", "src_img", "src_mask", "tsf_img", "tsf_mask"), outs, outs_ref):
        assert (a_.detach() - b_.detach()).abs().max().item() <= 2e-4, name
    gmax = max(v.grad.abs().max().item() for v in sd.values())
    names = [k for k, _ in G.named_parameters()]
    assert sorted(names) == sorted(sd) and (kind in ("add", "avg")) == (not any("gate_conv" in k for k in names))
    for k, p_ in G.named_parameters():
        assert p_.grad is not None, f"no gradient for {k}"
        rel = (p_.grad - sd[k].grad).abs().max().item() / max(sd[k].grad.abs().max().item(), 1e-3 * gmax)
        assert rel <= 2e-3, (k, rel)


@pytest.mark.parametrize("kind", list(KINDS))
def test_oracle_reproduces_reference_gradients(kind):
    """The oracle's autograd for the four blocks against outputs, loss and parameter gradients recorded from the reference's own generator
    modules (tests/golden/make_golden_lwb_variant_grads.py): the yardstick of the tests above and of the GPU suite is the reference's."""
    from tests.golden.make_golden_lwb_variant_grads import NF, NRES, BGF, NS, S as S_, case_inputs, loss_of, sample_index
    gv = np.load(os.path.join(GOLD, "golden_lwb_variant_grads_v1.npz"))
    g1 = np.load(os.path.join(GOLD, "golden_v1.npz"))
    name = KINDS[kind]
    shapes = generator_param_shapes(NF, NRES, BGF, lwb="plain" if kind in ("add", "avg") else "softgate")
    sd = {k: torch.tensor(v, requires_grad=True) for k, v in synthetic.fill_state_dict(shapes, seed=11).items()}
    bg_in, src_in, tsf_in, Tst, tgt = case_inputs(g1)
    outs = oracle_forward_train(sd, bg_in, src_in, tsf_in, Tst, kind, NF, NRES, BGF)
    loss = loss_of(outs, tgt)
    loss.backward()
    for oname, o in zip(("bg", "src_img", "src_mask", "tsf_img", "tsf_mask"), outs):
        assert np.abs(o.detach().numpy()[..., ::4, ::4] - gv[f"{name}/out/{oname}"]).max() <= 1e-5, oname
    assert abs(loss.item() - float(gv[f"{name}/loss"])) <= 1e-6 * abs(float(gv[f"{name}/loss"]))
    keys = [str(k) for k in gv[f"{name}/param_names"]]
    assert sorted(keys) == sorted(sd)
    gmax = float(gv[f"{name}/grad_max"].max())
    for i, k in enumerate(keys):
        g = sd[k].grad.detach().numpy().reshape(-1).astype(np.float64)
        floor = 1e-3 * gmax
        want_norm, want_sum = float(gv[f"{name}/grad_norm"][i]), float(gv[f"{name}/grad_sum"][i])
        assert abs(np.sqrt((g * g).sum()) - want_norm) <= 1e-4 * max(want_norm, floor), k
        # a sum cancels: its error is bounded by the norm's scale, not by its own value
        assert abs(g.sum() - want_sum) <= 1e-4 * max(abs(want_sum), want_norm, floor), k
        idx = sample_index(g.size, i)
        want = gv[f"{name}/grad_sample"][i][:idx.size]
        assert (np.abs(g[idx] - want) <= 1e-4 * np.maximum(np.abs(want), floor)).all(), k


def test_trainer_step_of_softgate_avg_cpu(monkeypatch):
    """One LWGTrainer.optimize_parameters() for SoftGateAvgLWB through the emulated C ABI (FlatAdam with none of its PAIRS present, the
    panel cache with the gate convolutions): losses finite, every weight moves by at most Adam's first step."""
    from ipercore_amd.trainers import FlatAdam, LWGTrainer, PatchGlobalDiscriminator, TrainOpts
    emu_ops.install(monkeypatch)
    monkeypatch.setattr(ops, "lwb_fuse_bwd", lwbfuse_emu.lwb_fuse_bwd)
    S_, ns, nf, nres, bgf = 32, 2, [64, 64, 128], 1, [64, 64, 128]
    G, _ = build_generator("sg_avg", nf, nres, bgf)
    assert not any(n.endswith(a) for n, _ in G.named_parameters() for a, _ in FlatAdam.PAIRS)
    torch.manual_seed(2)
    D = PatchGlobalDiscriminator(ndf=32, n_layers=3)
    u = lambda shape, seed, name: torch.tensor(synthetic.uniform_image(shape, seed, name))           # noqa: E731
    inp = {"input_G_bg": u((1, 1, 4, S_, S_), 10, "bg_inputs"), "input_G_src": u((1, ns, 6, S_, S_), 8, "src_inputs"),
           "input_G_tsf": u((1, 1, 6, S_, S_), 9, "tsf_inputs"), "Tst": u((1, 1, ns, S_, S_, 2), 11, "Tst"),
           "real_src": u((1, ns, 3, S_, S_), 700, "real_src"), "real_tsf": u((1, 1, 3, S_, S_), 701, "real_tsf"),
           "real_bg": u((1, 3, S_, S_), 702, "real_bg"), "body_mask": (u((1, ns + 1, 1, S_, S_), 703, "mask") > 0).float()}
    tr = LWGTrainer(G, D, opts=TrainOpts.l1_transfer())
    tr.set_input(inp)
    w0 = {k: v.detach().clone() for k, v in list(G.state_dict().items()) + list(D.state_dict().items())}
    lg, ld = _as_device(tr.optimize_parameters)
    assert np.isfinite(lg.item()) and np.isfinite(ld.item())
    for k, p_ in G.named_parameters():
        assert p_.grad is not None and torch.isfinite(p_.grad).all(), k
    moved = {k: (v.detach() - w0[k]).abs().max().item() for k, v in list(G.state_dict().items()) + list(D.state_dict().items())}
    assert max(moved.values()) <= 1.001e-4 and all(v > 0 for k, v in moved.items() if k.endswith("weight")), moved
    assert all(moved[k] > 0 for k in moved if "gate_conv" in k and k.endswith("weight"))


# ------------------------------------------------------------------------------------------------ the GPU suite's generator case
# tests/test_gpu_lwb_fuse_backward.py holds the kernels to 2e-3 against the oracle's fp32 autograd at S = 64.  These generators have no
# normalisation layer in the source / transfer streams, and at 64 x 64 a weight gradient sums over few positions: with some seeded weights
# a 1e-6 forward difference flips enough ReLU kinks that torch's OWN fp32 autograd is 1e-2 .. 6e-2 away from its fp64 evaluation (AddLWB
# with seeds 7 and 11, SoftGateAddLWB with seed 3) - no fp32 implementation can then be told from a wrong one at 2e-3.  The seed of each
# kind is therefore picked by the REFERENCE's own error, never by the kernels': the oracle's fp32 gradients must lie within 2e-4 (a tenth
# of the bound) of its fp64 gradients, which the test below keeps true.
GPU_S, GPU_NS, GPU_NF, GPU_NRES, GPU_BGF = 64, 2, [64, 64, 128], 2, [64, 64, 128]
GPU_CASE_SEEDS = {"add": 3, "avg": 7, "sg_add": 7, "sg_avg": 7}
GPU_CASES = [("add", 1), ("avg", 1), ("sg_add", 1), ("sg_avg", 1), ("sg_add", 2)]


def gpu_case_inputs(nt):
    """bg, src, tsf inputs, Tst (1,nt,ns,S,S,2) = golden_v1's rendered flows (nt = 2: plus the same body mirrored left to right), targets."""
    S_, ns = GPU_S, GPU_NS
    g1 = np.load(os.path.join(GOLD, "golden_v1.npz"))
    u = lambda shape, seed, name: torch.tensor(synthetic.uniform_image(shape, seed, name))           # noqa: E731
    Tst = torch.tensor(g1["render/Tst"]).view(1, 1, ns, S_, S_, 2)
    if nt == 2:
        Tst = torch.cat([Tst, Tst.flip(4).clone()], dim=1)
    tgt = [u(s, 500 + i, "tgt") for i, s in enumerate(((1, 1, 3, S_, S_), (1, ns, 3, S_, S_), (1, ns, 1, S_, S_), (1, nt, 3, S_, S_), (1, nt, 1, S_, S_)))]
    return u((1, 1, 4, S_, S_), 10, "bg_inputs"), u((1, ns, 6, S_, S_), 8, "src_inputs"), u((1, nt, 6, S_, S_), 9, "tsf_inputs"), Tst, tgt


def gpu_case_loss(outs, tgt, dev):
    return sum(((o - t.to(device=dev, dtype=o.dtype)) ** 2).mean() for o, t in zip(outs, tgt))


@pytest.mark.parametrize("kind,nt", GPU_CASES)
def test_gpu_generator_case_is_a_usable_yardstick(kind, nt):
    """The oracle's fp32 autograd of each GPU case lies within 2e-4 of its fp64 autograd (measure of check_generator_training_grads)."""
    _, sdn = build_generator(kind, GPU_NF, GPU_NRES, GPU_BGF, seed=GPU_CASE_SEEDS[kind])
    bg_in, src_in, tsf_in, Tst, tgt = gpu_case_inputs(nt)
    grads = {}
    for dt in (torch.float32, torch.float64):
        sd = {k: torch.tensor(v, dtype=dt, requires_grad=True) for k, v in sdn.items()}
        outs = oracle_forward_train(sd, bg_in.to(dt), src_in.to(dt), tsf_in.to(dt), Tst.to(dt), kind, GPU_NF, GPU_NRES, GPU_BGF)
        gpu_case_loss(outs, tgt, "cpu").backward()
        grads[dt] = {k: v.grad for k, v in sd.items()}
    g32, g64 = grads[torch.float32], grads[torch.float64]
    gmax = max(v.abs().max().item() for v in g64.values())
    rel = {k: (g32[k].double() - g64[k]).abs().max().item() / max(g64[k].abs().max().item(), 1e-3 * gmax) for k in g64}
    worst = max(rel, key=rel.get)
    assert rel[worst] <= 2e-4, (worst, rel[worst])
