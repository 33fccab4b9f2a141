"""The training path of the AddLWB / AvgLWB / SoftGateAddLWB / SoftGateAvgLWB generators on the GPU: lwg_lwb_fuse_bwd_f32 (FuseFn)
against fp64 autograd through the eager chain, the generators' training gradients against the oracle's autograd, the trainer's eager
and captured steps, and AttLWB-SPADE's training step making the launches it made before."""
import functools
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ipercore_amd import ops, synthetic
from ipercore_amd.networks import NetworksFactory, generator_param_shapes
from ipercore_amd.networks.training import FuseFn, TrainableGenerator
from tests import attn_flows, lwbfuse_emu
from tests import parity_utils as pu
from tests.gpu_checks import DEV, _cmp, _rand
from tests.test_lwb_fuse_backward_cpu import GPU_BGF as BGF
from tests.test_lwb_fuse_backward_cpu import GPU_NF as NF
from tests.test_lwb_fuse_backward_cpu import GPU_NRES as NRES
from tests.test_lwb_fuse_backward_cpu import GPU_NS as NS
from tests.test_lwb_fuse_backward_cpu import GPU_S as S
from tests.test_lwb_fuse_backward_cpu import GPU_CASES, GPU_CASE_SEEDS, KINDS, adversarial_flows, build_generator, oracle_forward_train
from tests.test_lwb_fuse_backward_cpu import gpu_case_inputs as _inputs
from tests.test_lwb_fuse_backward_cpu import gpu_case_loss as _loss

pytestmark = pytest.mark.gpu


#        C,  B, ns, h,  w,  S,  gate,  batched, scale_w, scale_o
CASES = [(32, 1, 2, 24, 24, 24, False, 1, 1.0, 1.0),            # same-size path, add
         (64, 2, 3, 16, 16, 64, True, 1, 1.0 / 3, 1.0),         # sg_avg
         (128, 1, 4, 12, 12, 48, False, 1, 1.0, 1.0 / 5),       # avg
         (256, 3, 1, 8, 8, 64, True, 0, 1.0, 1.0),              # three frames adding onto shared source rows
         (32, 1, 2, 5, 5, 20, False, 1, 1.0, 1.0),              # a last partial block
         (256, 1, 2, 3, 3, 12, True, 1, 0.5, 1.0),              # a last partial block
         (64, 1, 2, 6, 10, 12, True, 1, 1.0, 1.0)]              # h != w: the kernel accepts it although the generator does not


def _reach(T, h, w, nsrc, batched):
    """(nsrc,h,w) bool: source pixels within one pixel of a tap of any flow (fp64 restatement of the kernel's taps, dilated by one pixel
    so an fp32 rounding of a coordinate across a pixel edge stays inside)."""
    B, ns, S_ = T.shape[:3]
    Tf = lwbfuse_emu.resize_flow(T.double().reshape(B * ns, S_, S_, 2), h, w).reshape(B, ns, h, w, 2)
    hit = torch.zeros(nsrc, h, w)
    for b in range(B):
        for s in range(ns):
            for ty, tx, _, ok in lwbfuse_emu.taps(Tf[b, s], h, w):
                hit[b * ns + s if batched else s].view(-1)[(ty * w + tx)[ok]] = 1.0
    return F.max_pool2d(hit.unsqueeze(1), 3, 1, 1)[:, 0] > 0


@pytest.mark.parametrize("C,B,ns,h,w,S_,gated,batched,sw,so", CASES, ids=[f"c{c[0]}_b{c[1]}_ns{c[2]}_{c[3]}x{c[4]}_S{c[5]}" for c in CASES])
def test_fuse_backward_kernel(C, B, ns, h, w, S_, gated, batched, sw, so):
    """FuseFn against fp64 CPU autograd of the eager chain (F.interpolate align_corners=True -> F.grid_sample zeros -> fuse); the error
    measure and its bound are check_attention_backward's: max |d| / max(|ref| max, 1e-3 of the largest gradient) <= 5e-4."""
    _fuse_forward_backward(C, B, ns, h, w, S_, gated, batched, sw, so, adversarial_flows(B, ns, S_, seed=7 + C + h, dtype=torch.float32),
                           need_unreached=True)


#               B, ns, S,  h,  w   (tests/attn_flows.py: aligned without resize; in-kernel resize, h != w, a last partial block)
FAMILY_GEOMS = ((2, 2, 16, 16, 16), (2, 3, 40, 9, 13))
FAMILY_CASES = [(f, g) for g in FAMILY_GEOMS for f in attn_flows.FAMILIES if attn_flows.family_allowed(f, g)]


@pytest.mark.parametrize("family,geom", FAMILY_CASES, ids=[f"{f}-{attn_flows.geom_id(g)}" for f, g in FAMILY_CASES])
def test_fuse_forward_backward_on_flow_families(family, geom):
    """lwg_lwb_fuse_f32 and lwg_lwb_fuse_bwd_f32 on the flow families of tests/attn_flows.py (pixel centres, half pixels, the border
    band, one texel for all pixels, single foreground pixels, very large finite flows), gated, batched sources, under
    test_fuse_backward_kernel's assertions and bounds."""
    B, ns, S_, h, w = geom
    _fuse_forward_backward(64, B, ns, h, w, S_, True, 1, 1.0 / ns, 1.0, attn_flows.flows(family, B, ns, S_, S_, seed=0, size=(h, w)),
                           need_unreached=False)


def _fuse_forward_backward(C, B, ns, h, w, S_, gated, batched, sw, so, T, need_unreached):
    nsrc = B * ns if batched else ns
    tsf, src, g = _rand((B, h, w, C), 960), _rand((nsrc, h, w, C), 961), _rand((B, h, w, C), 962)
    gate = torch.sigmoid(_rand((B, h, w, C), 963)) if gated else None
    # ---- fp64 reference
    leaves = [t.double().requires_grad_(True) for t in ((tsf, src, gate) if gated else (tsf, src))]
    Td = T.double().reshape(B * ns, S_, S_, 2)
    if (h, w) != (S_, S_):
        Td = F.interpolate(Td.permute(0, 3, 1, 2), size=(h, w), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    sr = leaves[1] if batched else leaves[1].repeat(B, 1, 1, 1)
    warp = F.grid_sample(sr.permute(0, 3, 1, 2), Td, mode="bilinear", padding_mode="zeros", align_corners=False).permute(0, 2, 3, 1)
    fused = warp.reshape(B, ns, h, w, C).sum(dim=1) * sw
    yr = (leaves[0] + (leaves[2] * fused if gated else fused)) * so
    (yr * g.double()).sum().backward()
    # ---- the kernels
    dl = [t.to(DEV).requires_grad_(True) for t in ((tsf, src, gate) if gated else (tsf, src))]
    gd, Tdev = g.to(DEV), T.to(DEV)
    y = FuseFn.apply(dl[0], dl[1], dl[2] if gated else None, Tdev, sw, so, bool(batched))
    (y * gd).sum().backward()
    torch.cuda.synchronize()
    y0 = ops.lwb_fuse(dl[0].detach(), dl[1].detach(), Tdev, torch.empty_like(y), gate=dl[2].detach() if gated else None, scale_w=sw, scale_o=so,
                      src_batched=bool(batched))
    assert torch.equal(y.detach(), y0), "FuseFn's forward is not ops.lwb_fuse's"
    _cmp(y.detach(), yr.detach().float(), 3e-4, "fuse forward")        # check_attention_backward's forward bound (fp32 flow resize / tap coordinates)
    assert torch.equal(dl[0].grad, gd * so), "d_tsf is not dout * scale_o bit for bit"
    unreached = ~_reach(T, h, w, nsrc, batched)
    assert not need_unreached or w < 12 or unreached.any(), "the case has no source row out of every flow's reach"
    assert (dl[1].grad.cpu()[unreached] == 0).all(), "a source row no flow reaches received a gradient"
    gmax = max(t.grad.abs().max().item() for t in leaves)
    errs = {}
    for nm, a_, b_ in zip(("tsf", "src", "gate"), dl, leaves):
        errs[nm] = (a_.grad.cpu().double() - b_.grad).abs().max().item() / max(b_.grad.abs().max().item(), 1e-3 * gmax)
    print("lwb_fuse_bwd", (C, B, ns, h, w, S_, gated, batched), {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= 5e-4, errs


# ------------------------------------------------------------------------------------------------ generator gradients
@functools.lru_cache(maxsize=None)
def _oracle_grads(kind, nt):
    """The oracle's fp32 autograd of one case, computed once: (outputs, loss, {name: gradient})."""
    _, sdn = build_generator(kind, NF, NRES, BGF, seed=GPU_CASE_SEEDS[kind])
    bg_in, src_in, tsf_in, Tst, tgt = _inputs(nt)
    sd = {k: torch.tensor(v, requires_grad=True) for k, v in sdn.items()}
    outs = oracle_forward_train(sd, bg_in, src_in, tsf_in, Tst, kind, NF, NRES, BGF)
    loss = _loss(outs, tgt, "cpu")
    loss.backward()
    return [o.detach() for o in outs], loss.item(), {k: v.grad for k, v in sd.items()}


@pytest.mark.parametrize("precision", ["fp32", "winograd"])
@pytest.mark.parametrize("kind,nt", GPU_CASES)
def test_generator_training_grads(monkeypatch, kind, nt, precision):
    """One training forward + backward of the whole generator on the GPU against torch autograd through the oracle, with the bounds of
    check_generator_training_grads: outputs 2e-3, loss 1e-4, every parameter gradient <= 2e-3 of max(own scale, 1e-3 of the largest).
    The weights' seed per kind is GPU_CASE_SEEDS (chosen by the oracle's own fp32 error, see test_lwb_fuse_backward_cpu)."""
    outs_ref, loss_ref, grads = _oracle_grads(kind, nt)
    G, _ = build_generator(kind, NF, NRES, BGF, seed=GPU_CASE_SEEDS[kind])
    G.to(DEV)
    bg_in, src_in, tsf_in, Tst, tgt = _inputs(nt)
    monkeypatch.setattr(ops, "WINO_MIN_GRID", 0)
    with ops.conv_precision(precision):
        outs = TrainableGenerator(G).forward(bg_in.to(DEV), src_in.to(DEV), tsf_in.to(DEV), Tst.to(DEV))
        loss = _loss(outs, tgt, DEV)
        loss.backward()
    torch.cuda.synchronize()
    assert abs(loss.item() - loss_ref) <= 1e-4 * max(1.0, abs(loss_ref)), (loss.item(), loss_ref)
    for n_, a_, b_ in zip(("bg", "src_img", "src_mask", "tsf_img", "tsf_mask"), outs, outs_ref):
        _cmp(a_.detach(), b_, 2e-3, n_)
    gmax = max(v.abs().max().item() for v in grads.values())
    worst = (0.0, None)
    for k, p_ in G.named_parameters():
        assert p_.grad is not None, f"no gradient for {k}"
        rel = (p_.grad.cpu() - grads[k]).abs().max().item() / max(grads[k].abs().max().item(), 1e-3 * gmax)
        worst = max(worst, (rel, k))
    print("generator grads", kind, nt, precision, f"worst {worst[0]:.2e} at {worst[1]}")
    assert worst[0] <= 2e-3, worst


# ------------------------------------------------------------------------------------------------ trainer
def _trainer_inputs():
    bg_in, src_in, tsf_in, Tst, _ = _inputs(1)
    u = lambda shape, seed, name: torch.tensor(synthetic.uniform_image(shape, seed, name), device=DEV)      # noqa: E731
    return {"input_G_bg": bg_in.to(DEV), "input_G_src": src_in.to(DEV), "input_G_tsf": tsf_in.to(DEV), "Tst": Tst.to(DEV),
            "real_src": u((1, NS, 3, S, S), 700, "real_src"), "real_tsf": u((1, 1, 3, S, S), 701, "real_tsf"),
            "real_bg": u((1, 3, S, S), 702, "real_bg"), "body_mask": (u((1, NS + 1, 1, S, S), 703, "mask") > 0).float()}


@pytest.mark.parametrize("kind", ["avg", "sg_add"])
def test_trainer_steps_without_discriminator(kind):
    """Six L1 personalization steps without D: finite, the loss goes down; the personalized checkpoint renders through Imitator."""
    from ipercore_amd.imitator import Imitator
    from ipercore_amd.trainers import LWGTrainer, TrainOpts, personalize
    G, _ = build_generator(kind, NF, NRES, BGF)
    G.to(DEV)
    opts = TrainOpts.l1_transfer()
    opts.use_graph = False                                       # eager launches here; the captured step is the next test's
    tr = LWGTrainer(G, None, opts=opts)
    with tempfile.TemporaryDirectory() as d:
        ck = os.path.join(d, "personalized.pth")
        hist = personalize(tr, [_trainer_inputs()], n_iters=6, ckpt_path=ck, log_every=1)
        torch.cuda.synchronize()
        lg = [h[0] for h in hist]
        print("trainer", kind, "loss_G", lg)
        assert len(lg) == 6 and all(np.isfinite(v) for v in lg) and lg[-1] < lg[0], lg
        case = pu.build_case(image_size=S, num_filters=NF, n_res=NRES, bg_filters=BGF, n_frames=2, ns=NS)
        case.opt["gen_name"] = KINDS[kind]
        case.opt["meta_data"] = pu.AttrDict(personalized_ckpt_path=ck)
        im = Imitator(case.opt, device=torch.device(DEV), frame_batch=2)
        assert type(im.generator) is type(G)
        for k, v in im.generator.state_dict().items():
            assert torch.equal(v.cpu(), G.state_dict()[k].cpu()), f"{k}: personalized checkpoint not loaded"
        im.set_source(case.src_smpl, case.uv_img, case.bg_img, src_img=case.src_img)
        frames = im.inference(case.tgt_smpls, "smooth")
        assert np.isfinite(np.stack(frames)).all()


@pytest.mark.parametrize("kind", ["avg", "sg_add"])
def test_graph_vs_eager_steps(kind):
    """4 captured (hipGraph) against 4 eager steps with PatchGlobalDiscriminator: the assertions and bounds of gpu_checks._graph_vs_eager_steps
    (step counts, losses within 2e-3, flat buffers within 2 N lr max / 0.1 lr mean, panels repacked), then one inference forward."""
    from ipercore_amd.trainers import LWGTrainer, PatchGlobalDiscriminator, TrainOpts
    N, lr, inp, runs = 4, 1e-4, _trainer_inputs(), {}
    for mode in ("eager", "graph"):
        G, _ = build_generator(kind, NF, NRES, BGF)
        G.to(DEV)
        torch.manual_seed(0)
        D = PatchGlobalDiscriminator().to(DEV)
        opts = TrainOpts.l1_transfer()
        opts.use_graph = mode == "graph"
        tr = LWGTrainer(G, D, opts=opts)
        tr.set_input({k: v.clone() for k, v in inp.items()})
        panels0 = G.packed()
        hist = [tr.optimize_parameters() for _ in range(N)]
        torch.cuda.synchronize()
        assert len({h[0].data_ptr() for h in hist}) == N, "loss tensors of different steps alias one buffer"
        runs[mode] = dict(losses=[(float(a), float(b)) for a, b in hist], flatG=tr.optimizer_G.flat.clone(), flatD=tr.optimizer_D.flat.clone(),
                          tG=int(tr.optimizer_G.t_dev.item()), tD=int(tr.optimizer_D.t_dev.item()), tG_host=tr.optimizer_G.t, step_mode=tr.step_mode)
        assert G.packed() is not panels0, f"{mode}: the inference engine kept its weight panels after {N} updates"
        G.eval()
        with torch.no_grad():
            enc, res = G.forward_src(inp["input_G_src"], only_enc=True)
            img, mask = G.forward_tsf(inp["input_G_tsf"][:, 0], enc, res, inp["Tst"][:, 0])
        assert torch.isfinite(img).all() and torch.isfinite(mask).all()
    e, gr = runs["eager"], runs["graph"]
    assert "hipGraph" in gr["step_mode"], gr["step_mode"]
    assert e["tG"] == gr["tG"] == N and e["tD"] == gr["tD"] == N and gr["tG_host"] == N, (e["tG"], gr["tG"], e["tD"], gr["tD"], gr["tG_host"])
    for (a0, b0), (a1, b1) in zip(e["losses"], gr["losses"]):
        assert abs(a0 - a1) <= 2e-3 * max(1.0, abs(a0)) and abs(b0 - b1) <= 2e-3 * max(1.0, abs(b0)), (e["losses"], gr["losses"])
    for k in ("flatG", "flatD"):
        d = (e[k] - gr[k]).abs()
        print("graph vs eager", kind, k, f"max {d.max().item():.2e} mean/lr {d.mean().item() / lr:.2e}")
        assert d.max().item() <= 2 * N * lr and d.mean().item() <= 0.1 * lr, k


# ------------------------------------------------------------------------------------------------ AttLWB-SPADE unchanged
class _Launches:
    """Records the kinds ops.CONV_HOOK reports and every call of the fusion block's two ops."""

    def __init__(self, monkeypatch):
        self.kinds, self.fuse = [], []
        for name in ("lwb_fuse", "lwb_fuse_bwd"):
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))

    def _wrap(self, name, fn):
        def wrapped(*a, **k):
            self.fuse.append(name)
            return fn(*a, **k)
        return wrapped

    def __call__(self, begin, M, spec, epi=0, info=None):
        if not begin:
            self.kinds.append(info["kind"])


def test_attlwb_spade_training_step_is_unchanged(monkeypatch):
    """One AttLWB-SPADE training forward / backward at S = 64: no lwb_fuse* launch, the same convolution launches in a second identical
    run, outputs bitwise equal, gradients equal up to the arrival order of the attention backward's atomics."""
    rec = _Launches(monkeypatch)
    monkeypatch.setattr(ops, "CONV_HOOK", rec)
    G = NetworksFactory.get_by_name("AttLWB-SPADE", cfg=pu.gen_cfg(NF, NRES, BGF), temporal=False)
    sdn = synthetic.fill_state_dict(generator_param_shapes(NF, NRES, BGF), seed=7)
    G.load_state_dict({k: torch.tensor(v) for k, v in sdn.items()}, strict=True)
    G.to(DEV).train()
    bg_in, src_in, tsf_in, Tst, tgt = _inputs(1)
    runs = []
    for _ in range(2):
        G.zero_grad(set_to_none=True)
        rec.kinds = []
        outs = TrainableGenerator(G).forward(bg_in.to(DEV), src_in.to(DEV), tsf_in.to(DEV), Tst.to(DEV))
        _loss(outs, tgt, DEV).backward()
        torch.cuda.synchronize()
        runs.append(([o.detach().clone() for o in outs], {k: p.grad.clone() for k, p in G.named_parameters()}, list(rec.kinds)))
    assert rec.fuse == [], rec.fuse
    assert runs[0][2] == runs[1][2] and len(runs[0][2]) > 50
    for a_, b_ in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a_, b_)
    gmax = max(v.abs().max().item() for v in runs[0][1].values())
    for k, v in runs[0][1].items():
        # two arrival orders of the same fp32 atomic sums: the bound the K | V form of check_attention_backward is held to against AttnFn
        assert (v - runs[1][1][k]).abs().max().item() <= 1e-5 * max(v.abs().max().item(), 1e-3 * gmax), k
