"""The bf16 engine of the AddLWB / AvgLWB / SoftGateAddLWB / SoftGateAvgLWB generators on the GPU: lwg_lwb_fuse_bf16 against the fp32
kernel on the upcast operands and against the fp64 eager chain, the four generators in "bf16" / "bf16_winograd" against their own fp32
engine, the reference's recorded outputs and the oracle (PSNR >= 40 dB), Imitator end to end, and AttLWB-SPADE untouched."""
import functools
import os

import numpy as np
import pytest
import torch

from ipercore_amd import ops, synthetic
from ipercore_amd.networks import NetworksFactory, generator_param_shapes
from tests import attn_flows
from tests import lwbfuse_bf16_emu as emu16
from tests import parity_utils as pu
from tests.gpu_checks import DEV, _rand
from tests.test_gpu_lwb_fuse_backward import CASES, FAMILY_CASES
from tests.test_lwb_fuse_backward_cpu import adversarial_flows

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("C,B,ns,h,w,S_,gated,batched,sw,so", CASES, ids=[f"c{c[0]}_b{c[1]}_ns{c[2]}_{c[3]}x{c[4]}_S{c[5]}" for c in CASES])
def test_fuse_bf16_kernel(C, B, ns, h, w, S_, gated, batched, sw, so):
    """Every element, none excluded:
    (i)  against ops.lwb_fuse in fp32 on the upcast operands, y32: |out - y32| <= 2^-7 |y32| + 1e-30.  The two kernels share the flow / tap
         helpers and the order of the fp32 arithmetic, so their fp32 results differ by a few fp32 ulp at most (contraction choices) and one
         rounding of either to bf16 lands at most one bf16 ulp (<= 2^-7 relative) apart;
    (ii) against the fp64 eager chain, ref: |out - ref| <= 2^-8 |ref| + 3e-4 max(1, max|ref|) - twice the half-ulp of the bf16 store plus
         the bound test_fuse_backward_kernel holds the fp32 forward to (fp32 flow resize / tap coordinates on adversarial flows).
    The output buffer is followed by a guard band that must stay untouched (the last partial block)."""
    _fuse_bf16_kernel(C, B, ns, h, w, S_, gated, batched, sw, so, adversarial_flows(B, ns, S_, seed=7 + C + h, dtype=torch.float32))


@pytest.mark.parametrize("family,geom", FAMILY_CASES, ids=[f"{f}-{attn_flows.geom_id(g)}" for f, g in FAMILY_CASES])
def test_fuse_bf16_kernel_on_flow_families(family, geom):
    """lwg_lwb_fuse_bf16 on the flow families of tests/attn_flows.py, gated, batched sources, under test_fuse_bf16_kernel's two bounds
    (the fp32 kernel on the upcast operands, the fp64 eager chain) and its guard band."""
    B, ns, S_, h, w = geom
    _fuse_bf16_kernel(64, B, ns, h, w, S_, True, 1, 1.0 / ns, 1.0, attn_flows.flows(family, B, ns, S_, S_, seed=0, size=(h, w)))


def _fuse_bf16_kernel(C, B, ns, h, w, S_, gated, batched, sw, so, T):
    tsf, src, gate = emu16.kernel_case(C, B, ns, h, w, S_, gated, batched, _rand)
    ref = emu16.eager_chain(tsf, src, T, gate, sw, so, bool(batched), dtype=torch.float64)
    n = B * h * w * C
    buf = torch.full((n + 4096,), -7.0, device=DEV, dtype=BF)
    out = ops.lwb_fuse(tsf.to(DEV), src.to(DEV), T.to(DEV), buf[:n].view(B, h, w, C), gate=None if gate is None else gate.to(DEV),
                       scale_w=sw, scale_o=so, src_batched=bool(batched))
    y32 = ops.lwb_fuse(tsf.float().to(DEV), src.float().to(DEV), T.to(DEV), torch.empty(B, h, w, C, device=DEV),
                       gate=None if gate is None else gate.float().to(DEV), scale_w=sw, scale_o=so, src_batched=bool(batched))
    torch.cuda.synchronize()
    assert out.dtype == BF and (buf[n:] == -7.0).all(), "the kernel wrote past its output"
    o, y = out.cpu(), y32.cpu()
    assert torch.isfinite(o.float()).all()
    share = (o.view(torch.int16) == y.to(BF).view(torch.int16)).float().mean().item()
    d32 = (o.double() - y.double()).abs()
    d64 = (o.double() - ref).abs()
    bound64 = 2.0 ** -8 * ref.abs() + 3e-4 * max(1.0, ref.abs().max().item())
    print("lwb_fuse_bf16", (C, B, ns, h, w, S_, gated, batched), f"bitwise == bf16(fp32 kernel): {share:.4%}",
          f"max |out - y32| / |y32| {(d32 / y.double().abs().clamp_min(1e-30)).max().item():.2e}",
          f"max |out - ref| / bound {(d64 / bound64).max().item():.3f}")
    assert (d32 <= 2.0 ** -7 * y.double().abs() + 1e-30).all()
    assert (d64 <= bound64).all()


# ------------------------------------------------------------------------------------------------ the generators
class _FuseCalls:
    """Records the tensor dtypes of every ops.lwb_fuse call."""

    def __init__(self, monkeypatch):
        self.calls = []
        fn = ops.lwb_fuse

        def wrapped(tsf_x, src_x, T, out, gate=None, **k):
            self.calls.append({"act": {t.dtype for t in (tsf_x, src_x, out, gate) if t is not None}, "T": T.dtype, "gated": gate is not None})
            return fn(tsf_x, src_x, T, out, gate=gate, **k)
        monkeypatch.setattr(ops, "lwb_fuse", wrapped)


def _run(G, mode, src_inputs, tsf_inputs, Tst):
    G.conv_precision = mode
    enc, res = G.forward_src(src_inputs, only_enc=True)            # source features rebuilt per mode
    img, mask = G.forward_tsf(tsf_inputs, enc, res, Tst)
    torch.cuda.synchronize()
    return img, mask, enc, res


@functools.lru_cache(maxsize=None)
def _fp32_engine(kind, tag):
    """The generator's "winograd" (fp32) outputs of one case, computed once and left unchanged."""
    G, _ = emu16.build_generator(kind, tag)
    G.to(DEV)
    img, mask, _, _ = _run(G, "winograd", *(t.to(DEV) for t in emu16.generator_inputs()))
    return img.cpu(), mask.cpu()


@pytest.mark.parametrize("kind,tag,mode", [("add", "tiny", "bf16"), ("avg", "tiny", "bf16"), ("sg_add", "tiny", "bf16"), ("sg_avg", "tiny", "bf16"),
                                           ("sg_avg", "full", "bf16"), ("sg_add", "tiny", "bf16_winograd")])
def test_generators_in_bf16(monkeypatch, kind, tag, mode):
    """forward_src + forward_tsf at S = 64 with check_lwb_variant_generators' inputs and seed 11: PSNR >= 40 dB (the bound of
    check_bf16_generator; peak-to-peak 2 for img, 1 for mask) against the same object's fp32 engine AND against the reference's recorded
    outputs; fp32 NCHW outputs, finite, not the fp32 engine's bits; n_down + n_res fuse calls, all on bf16 tensors with fp32 flows.
    tests/test_lwb_fuse_bf16_cpu.py holds bf16 storage alone to >= 60 dB on these very cases."""
    gv = np.load(os.path.join(emu16.GOLD, "golden_lwb_variants_v1.npz"))
    img32, mask32 = _fp32_engine(kind, tag)
    G, _ = emu16.build_generator(kind, tag)
    G.to(DEV)
    src_inputs, tsf_inputs, Tst = (t.to(DEV) for t in emu16.generator_inputs())
    G.conv_precision = "winograd"
    enc32, res32 = G.forward_src(src_inputs, only_enc=True)
    G.conv_precision = mode
    with pytest.raises(RuntimeError, match="rebuild them"):        # fp32 source features in a bf16 mode: the guard stays
        G.forward_tsf(tsf_inputs, enc32, res32, Tst)
    rec = _FuseCalls(monkeypatch)
    img, mask, _, _ = _run(G, mode, src_inputs, tsf_inputs, Tst)
    nf, nres, _ = emu16.CONFIGS[tag]
    assert len(rec.calls) == len(nf) + nres, len(rec.calls)
    assert all(c["act"] == {BF} and c["T"] == torch.float32 and c["gated"] == kind.startswith("sg") for c in rec.calls), rec.calls
    assert img.dtype == torch.float32 and mask.dtype == torch.float32 and tuple(img.shape) == (1, 3, emu16.S, emu16.S)
    assert tuple(mask.shape) == (1, 1, emu16.S, emu16.S) and torch.isfinite(img).all() and torch.isfinite(mask).all()
    name = emu16.KINDS[kind]
    p = {"img_vs_fp32": emu16.psnr(img, img32, 2.0), "mask_vs_fp32": emu16.psnr(mask, mask32, 1.0),
         "img_vs_golden": emu16.psnr(img, torch.tensor(gv[f"{name}/{tag}/img"]), 2.0),
         "mask_vs_golden": emu16.psnr(mask, torch.tensor(gv[f"{name}/{tag}/mask"]), 1.0)}
    print("bf16 generator", name, tag, mode, {k: f"{v:.1f} dB" for k, v in p.items()})
    assert (img.cpu() - img32).abs().max().item() > 0, "the bf16 mode produced the fp32 engine's bits: the bf16 kernels did not run"
    assert min(p.values()) >= 40.0, p


@pytest.mark.parametrize("kind", ["avg", "sg_add"])
def test_batched_sources_in_bf16(kind):
    """forward(bg, src, tsf, Tst) with bs = 2 (frame b warps source rows b * ns + s), full width, the inputs of the bs2 block of
    check_lwb_variant_generators: PSNR >= 40 dB against the fp32 oracle."""
    G, sdn = emu16.build_generator(kind, "full")
    G.to(DEV)
    G.conv_precision = "bf16"
    bg2, src2, tsf2, T2 = emu16.bs2_inputs()
    outs = G(bg2.to(DEV), src2.to(DEV), tsf2.unsqueeze(1).to(DEV), T2.unsqueeze(1).to(DEV), only_tsf=True)
    torch.cuda.synchronize()
    want_img, want_mask = emu16.oracle_tsf(sdn, kind, "full", src2, tsf2, T2)
    assert torch.isfinite(outs[1]).all() and torch.isfinite(outs[2]).all()
    p = {"img": emu16.psnr(outs[1][:, 0], want_img, 2.0), "mask": emu16.psnr(outs[2][:, 0], want_mask, 1.0)}
    print("bf16 bs2", emu16.KINDS[kind], {k: f"{v:.1f} dB" for k, v in p.items()})
    assert min(p.values()) >= 40.0, p


# ------------------------------------------------------------------------------------------------ Imitator
@pytest.mark.parametrize("name", ["AvgLWB", "SoftGateAddLWB"])
def test_imitator_in_bf16(name):
    """set_source + inference at 128 x 128 in "bf16": PSNR >= 40 dB against the same imitator in its default mode, and the frames rendered at
    frame_batch 1 and 2 are bitwise equal (a frame never depends on its batch)."""
    from ipercore_amd.imitator import Imitator
    case = pu.build_case(image_size=128, num_filters=[64, 64, 128], n_res=2, bg_filters=[64, 64, 128], n_frames=2, ns=2)
    case.opt["gen_name"] = name
    im = Imitator(case.opt, device=torch.device(DEV), frame_batch=2)
    sdn = synthetic.fill_state_dict({k: tuple(v.shape) for k, v in im.generator.state_dict().items()}, seed=7)
    im.generator.load_state_dict({k: torch.tensor(v) for k, v in sdn.items()}, strict=True)
    im.generator.to(im.device)

    def frames():
        im.set_source(case.src_smpl, case.uv_img, case.bg_img, src_img=case.src_img)
        return np.stack(im.inference(case.tgt_smpls, "smooth"))
    ref = frames()
    im.generator.conv_precision = "bf16"
    got2 = frames()
    im.frame_batch = 1
    got1 = frames()
    assert got2.shape == ref.shape and got2.shape[0] == 2 and got2.dtype == ref.dtype and np.isfinite(got2).all()
    p = emu16.psnr(torch.tensor(got2), torch.tensor(ref), 2.0)
    print("bf16 imitator", name, f"{p:.1f} dB vs the default mode")
    assert np.abs(got2 - ref).max() > 0, "the bf16 mode produced the default mode's frames: the bf16 kernels did not run"
    assert p >= 40.0, p
    assert np.array_equal(got1, got2), "bf16 frames depend on the frame batch"


# ------------------------------------------------------------------------------------------------ AttLWB-SPADE unchanged
def test_attlwb_spade_in_bf16_makes_no_fuse_call(monkeypatch):
    nf, nres, bgf = emu16.CONFIGS["tiny"]
    G = NetworksFactory.get_by_name("AttLWB-SPADE", cfg=pu.gen_cfg(nf, nres, bgf), temporal=False).eval()
    sdn = synthetic.fill_state_dict(generator_param_shapes(nf, nres, bgf), seed=7)
    G.load_state_dict({k: torch.tensor(v) for k, v in sdn.items()}, strict=True)
    G.to(DEV)
    rec = _FuseCalls(monkeypatch)
    img, mask, _, _ = _run(G, "bf16", *(t.to(DEV) for t in emu16.generator_inputs()))
    assert rec.calls == [] and torch.isfinite(img).all() and torch.isfinite(mask).all()
