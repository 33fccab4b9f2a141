#!/usr/bin/env python3
"""Timings around the bf16 warp-and-fuse block (profiles/lwb_fuse_bf16.txt) - information, not a gate.

(a) lwg_lwb_fuse_f32 next to lwg_lwb_fuse_bf16, ungated and gated, at the three site shapes of a 1024 x 1024 generator (512^2 x 64,
    256^2 x 128, 128^2 x 256): frame batch 20, ns = 2, the flows of a rendered body resized to the site (what the generator hands the
    kernel).  Both run on the same values - the fp32 tensors are the upcast bf16 ones - and alternate inside the timed loop.  Bytes per
    launch from shapes: tsf + out (+ gate) + flows + the source rows the flows reach.
(b) Frames/s of a 1024 x 1024 clip through Imitator for AvgLWB and SoftGateAddLWB in "winograd" (fp32) and in "bf16".
One process, event timing after warm-up.

    python tools/bench_lwb_fuse_bf16.py [--out profiles/lwb_fuse_bf16.txt]
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from ipercore_amd import ops, synthetic as syn  # noqa: E402

DEV = "cuda:0"
S, NS, FB = 1024, 2, 20
NF, NRES, BGF = [64, 128, 256], 6, [64, 128, 128, 256]


class Lines(list):
    """The report: every line is printed as it is measured and kept for --out."""

    def append(self, line):
        print(line, flush=True)
        super().append(line)


def timed_pair(fa, fb, warmup=5, iters=30):
    """fa and fb alternating in one loop -> (us per fa launch, us per fb launch), medians of per-launch event intervals."""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(iters)]
    for e in ev:
        e[0].record()
        fa()
        e[1].record()
        fb()
        e[2].record()
    torch.cuda.synchronize()
    ta = sorted(e[0].elapsed_time(e[1]) for e in ev)[iters // 2] * 1e3
    tb = sorted(e[1].elapsed_time(e[2]) for e in ev)[iters // 2] * 1e3
    return ta, tb


def reached_rows(Tf, h, w):
    """Source rows (pixels) within reach of a bilinear tap of any frame's flow: Tf (B,ns,h,w,2) at the site's size -> count over the ns sources."""
    B, ns = Tf.shape[:2]
    ix = ((Tf[..., 0] + 1) * w - 1) * 0.5
    iy = ((Tf[..., 1] + 1) * h - 1) * 0.5
    x0, y0 = ix.floor().clamp(-2, w + 1).long(), iy.floor().clamp(-2, h + 1).long()
    hit = torch.zeros(ns * h * w, dtype=torch.bool, device=Tf.device)
    base = (torch.arange(ns, device=Tf.device) * (h * w)).view(1, ns, 1, 1)
    for dy in (0, 1):
        for dx in (0, 1):
            ty, tx = y0 + dy, x0 + dx
            ok = (ty >= 0) & (ty < h) & (tx >= 0) & (tx < w)
            hit[(base + ty * w + tx)[ok]] = True
    return int(hit.sum())


def clip_inputs(n_frames):
    case = syn.build_case(image_size=S, num_filters=NF, n_res=NRES, bg_filters=BGF, n_frames=n_frames, ns=NS, seed=0)
    im = syn.make_imitator(case, frame_batch=FB, device=DEV)
    tgt = im.prepare_sequence(case.tgt_smpls, "smooth")
    _, Tst, _ = im.make_inputs_for_tsf(im.src_info, tgt[:FB], "smooth", t=0)
    Tst = Tst.contiguous().clone()
    del im
    torch.cuda.empty_cache()
    return case, Tst


def kernels(Tst, lines):
    bf = torch.bfloat16
    g = torch.Generator(device="cpu").manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV).to(bf)                                        # noqa: E731
    body = float((Tst[..., 0] > -1.5).float().mean())
    lines.append(f"(a) flows: rendered body at {S}x{S}, frame batch {FB}, ns = {NS}; {100 * body:.1f} % of the flow samples are body pixels (the rest is "
                 "the -2 background: every tap outside)")
    lines.append(f"{'site (h x w x C)':<18}{'gate':<6}{'f32 us':>9}{'bf16 us':>9}{'bf16/f32':>9}{'f32 MB':>9}{'bf16 MB':>9}{'f32 GB/s':>10}{'bf16 GB/s':>10}{'rows reached':>14}")
    for h, C in ((512, 64), (256, 128), (128, 256)):
        Tf = ops.flow_resize(Tst, h, h)
        rows = reached_rows(Tf, h, h)
        src16, tsf16, gate16 = r(NS, h, h, C), r(FB, h, h, C), torch.sigmoid(r(FB, h, h, C).float()).to(bf)
        src32, tsf32, gate32 = src16.float(), tsf16.float(), gate16.float()
        out16, out32 = torch.empty_like(tsf16), torch.empty_like(tsf32)
        for gated in (False, True):
            g16, g32 = (gate16, gate32) if gated else (None, None)
            t32, t16 = timed_pair(lambda: ops.lwb_fuse(tsf32, src32, Tf, out32, gate=g32, scale_w=0.5),
                                  lambda: ops.lwb_fuse(tsf16, src16, Tf, out16, gate=g16, scale_w=0.5))
            px = FB * h * h
            by = lambda e: px * C * e * (3 if gated else 2) + px * NS * 8 + rows * C * e                  # noqa: E731
            assert ((out16.float() - out32).abs() <= 2.0 ** -7 * out32.abs() + 1e-30).all(), "the two kernels disagree"
            lines.append(f"{f'{h} x {h} x {C}':<18}{'yes' if gated else 'no':<6}{t32:>9.1f}{t16:>9.1f}{t16 / t32:>9.2f}{by(4) / 1e6:>9.1f}{by(2) / 1e6:>9.1f}"
                         f"{by(4) / t32 / 1e3:>10.0f}{by(2) / t16 / 1e3:>10.0f}{rows:>9} / {NS * h * h}")
        del src16, tsf16, gate16, src32, tsf32, gate32, out16, out32, Tf
        torch.cuda.empty_cache()


def clips(case, lines, reps=3):
    from ipercore_amd.imitator import Imitator
    n = case.tgt_smpls.shape[0]
    lines.append(f"(b) {n}-frame clip at {S}x{S} through Imitator (G {NF} x {NRES} residual blocks, ns = {NS}, frame batch {FB}, one stream), frames/s")
    lines.append(f"{'generator':<18}{'winograd (fp32)':>18}{'bf16':>10}{'bf16 / fp32':>13}")
    for name in ("AvgLWB", "SoftGateAddLWB"):
        case.opt["gen_name"] = name
        im = Imitator(case.opt, device=torch.device(DEV), frame_batch=FB)
        shapes = {k: tuple(v.shape) for k, v in im.generator.state_dict().items()}
        im.generator.load_state_dict({k: torch.tensor(v) for k, v in syn.fill_state_dict(shapes, seed=7).items()}, strict=True)
        im.generator.to(im.device)
        fps = {}
        for mode in ("winograd", "bf16"):
            im.generator.conv_precision = mode
            im.set_source(case.src_smpl, case.uv_img, case.bg_img, src_img=case.src_img)
            tgt = im.prepare_sequence(case.tgt_smpls, "smooth")
            im.synthesize(tgt, "smooth")                                   # warm-up: panels, allocator, clocks
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                im.synthesize(tgt, "smooth")
            torch.cuda.synchronize()
            fps[mode] = reps * n / (time.perf_counter() - t0)
        lines.append(f"{name:<18}{fps['winograd']:>18.1f}{fps['bf16']:>10.1f}{fps['bf16'] / fps['winograd']:>13.2f}")
        del im
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=40)
    a = ap.parse_args()
    lines = Lines()
    lines.append(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; event timing, one process")
    case, Tst = clip_inputs(a.frames)
    kernels(Tst, lines)
    clips(case, lines)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(text)


if __name__ == "__main__":
    main()
