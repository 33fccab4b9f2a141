#!/usr/bin/env python3
"""Timings around the warp-and-fuse block's backward (profiles/lwb_fuse_bwd.txt) - information, not a gate.

1. lwg_lwb_fuse_bwd_f32 (ungated and gated) next to lwg_lwb_attention_kv_bwd_f32 at the three personalization site shapes of a 512 x 512
   step (256^2 x 64, 128^2 x 128, 64^2 x 256; ns = 2, B = 1, flows of a rendered body at 512 x 512), each with the zeroing of the
   accumulated gradient its ops wrapper does.
2. One captured L1 personalization step (G + PatchGlobalDiscriminator forward / backward / Adam) at 512 x 512 for SoftGateAddLWB, AvgLWB
   and AttLWB-SPADE.
One process, event timing after warm-up.

    python tools/bench_lwb_fuse_bwd.py [--out profiles/lwb_fuse_bwd.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from ipercore_amd import ops, synthetic as syn  # noqa: E402

DEV = "cuda:0"
S, NS = 512, 2
NF, NRES, BGF = [64, 128, 256], 6, [64, 128, 128, 256]


def timed(fn, warmup=5, iters=50):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3            # us


def sample():
    """Network inputs of one personalization sample with the flows of the renderer path (bench_personalize.measure's)."""
    case = syn.build_case(image_size=S, n_frames=1, ns=NS, seed=0)
    im = syn.make_imitator(case, frame_batch=1, device=DEV)
    tgt = im.prepare_sequence(case.tgt_smpls, "smooth")
    tsf8, Tst, _ = im.make_inputs_for_tsf(im.src_info, tgt[0:1], "smooth", t=0)
    u = lambda shape, seed, name: torch.tensor(syn.uniform_image(shape, seed, name), device=DEV)   # noqa: E731
    inp = {"input_G_bg": u((1, 1, 4, S, S), 10, "bg_inputs"),
           "input_G_src": torch.cat([torch.tensor(case.src_img, device=DEV)[0], im.src_info["cond"]], dim=1).unsqueeze(0),
           "input_G_tsf": ops.nhwc_to_nchw(tsf8, channels=6).unsqueeze(0), "Tst": Tst.unsqueeze(1).contiguous(),
           "real_src": torch.tensor(case.src_img, device=DEV), "real_tsf": u((1, 1, 3, S, S), 701, "real_tsf"),
           "real_bg": u((1, 3, S, S), 702, "real_bg"), "body_mask": (u((1, NS + 1, 1, S, S), 703, "mask") > 0).float()}
    del im
    torch.cuda.empty_cache()
    return inp


def kernels(T, lines):
    g = torch.Generator(device="cpu").manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)                                              # noqa: E731
    body = float((T[0, :, :, :, 0] > -1.5).float().mean())
    lines.append(f"flows: rendered body at {S}x{S}, ns = {NS}; {100 * body:.1f} % of the flow samples are body pixels (the rest is the -2 background)")
    lines.append(f"{'site (h x w x C)':<20}{'fuse_bwd us':>14}{'fuse_bwd gated us':>20}{'attention_kv_bwd us':>22}")
    for h, C in ((256, 64), (128, 128), (64, 256)):
        src, dout, gate, q = r(NS, h, h, C), r(1, h, h, C), torch.sigmoid(r(1, h, h, C)), r(1, h, h, C)
        kv, bk, bv = r(NS, h, h, 2 * C), r(C), r(C)
        t_plain = timed(lambda: ops.lwb_fuse_bwd(src, None, T, dout, src_batched=True))
        t_gate = timed(lambda: ops.lwb_fuse_bwd(src, gate, T, dout, src_batched=True, scale_w=0.5))
        t_att = timed(lambda: ops.lwb_attention_kv_bwd(q, kv, bk, bv, T, dout, src_batched=True))
        lines.append(f"{f'{h} x {h} x {C}':<20}{t_plain:>14.1f}{t_gate:>20.1f}{t_att:>22.1f}")


def steps(inp, lines, warmup=4, iters=10):
    from ipercore_amd.networks import NetworksFactory
    from ipercore_amd.trainers import LWGTrainer, PatchGlobalDiscriminator, TrainOpts
    lines.append(f"captured L1 personalization step at {S}x{S} (G {NF} x {NRES} residual blocks + PatchGlobalDiscriminator, ns = {NS}, nt = 1), ms per step")
    for name in ("SoftGateAddLWB", "AvgLWB", "AttLWB-SPADE"):
        G = NetworksFactory.get_by_name(name, cfg=syn.gen_cfg(NF, NRES, BGF), temporal=False)
        shapes = {k: tuple(v.shape) for k, v in G.state_dict().items()}
        G.load_state_dict({k: torch.tensor(v) for k, v in syn.fill_state_dict(shapes, seed=7).items()}, strict=True)
        G.to(DEV).train()
        torch.manual_seed(0)
        D = PatchGlobalDiscriminator().to(DEV)
        tr = LWGTrainer(G, D, opts=TrainOpts.l1_transfer())
        tr.set_input({k: v.clone() for k, v in inp.items()})
        ms = timed(tr.optimize_parameters, warmup=warmup, iters=iters) / 1e3
        lines.append(f"{name:<20}{ms:>10.2f}   ({tr.step_mode})")
        del tr, G, D
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; event timing, one process"]
    inp = sample()
    kernels(inp["Tst"][:, 0].contiguous(), lines)
    steps(inp, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(text)


if __name__ == "__main__":
    main()
