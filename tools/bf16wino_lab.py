#!/usr/bin/env python
"""Measurements behind ops.conv_precision("bf16_winograd") (csrc/conv_winograd_bf16.hip).

  python tools/bf16wino_lab.py --ratios   CPU: the emulated error ratios of tests/bf16wino_emu.py -> profiles/bf16wino_adversarial_ratios.txt
  python tools/bf16wino_lab.py --layers   GPU: lwg_conv2d_winograd_bf16 against lwg_conv2d_nhwc_bf16_hr on the generator's 3x3 / stride-1 layer
                                          shapes at 1024 x 1024, frame batch 20 (HIP events) -> profiles/bf16wino_layers.txt
  python tools/bf16wino_lab.py --clip     GPU: the 1024 x 1024 novel-view clip in "bf16" and "bf16_winograd" mode, alternated three times each,
                                          PSNR of each against the fp32 path -> profiles/bf16wino_clip_ab.txt
Each GPU step runs in a child process of its own under its own time limit; the first step that fails or times out ends the run."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PROFILES = os.path.join(ROOT, "profiles")

# (name, H = W, C0, C1, N (stacked 2 C for SPADE), kind) at 1024 x 1024 input, num_filters [64, 128, 256]
LAYERS = [
    ("spade shared 512^2  64->128", 512, 64, 0, 128, "conv"),
    ("spade g|b    512^2 128->2x64", 512, 128, 0, 128, "spade"),
    ("skip conv    512^2 64+64->64", 512, 64, 64, 64, "conv"),
    ("spade shared 256^2 128->128", 256, 128, 0, 128, "conv"),
    ("spade g|b    256^2 128->2x128", 256, 128, 0, 256, "spade"),
    ("skip conv    256^2 128+128->128", 256, 128, 128, 128, "conv"),
    ("spade shared 128^2 256->128", 128, 256, 0, 128, "conv"),
    ("spade g|b    128^2 128->2x256", 128, 128, 0, 512, "spade"),
    ("res block    128^2 256->256", 128, 256, 0, 256, "res"),
]
STEP_LIMIT_S = {"layers": 240, "clip": 420}


def step_ratios():
    from tests.bf16wino_emu import RATIO_BOUND, adversarial_ratios
    r = adversarial_ratios()
    lines = ["# relative L2 error against an fp64 convolution of the same bf16 activations and fp32 weights (CPU emulation at the kernel's rounding points,",
             "# fp32 accumulation; tests/bf16wino_emu.py): F(2x2,3x3) bf16 Winograd | direct bf16 | ratio",
             f"# bound used by the tests: ratio <= {RATIO_BOUND} (measured range below + margin for the accumulation order; the reasoning is in tests/bf16wino_emu.py)"]
    for k, (ew, ed, ratio) in r.items():
        lines.append(f"{k:32s} {ew:.3e} {ed:.3e} {ratio:.2f}")
    ratios = [v[2] for v in r.values()]
    lines.append(f"# min {min(ratios):.2f} max {max(ratios):.2f}")
    _write("bf16wino_adversarial_ratios.txt", lines)


def _write(name, lines):
    os.makedirs(PROFILES, exist_ok=True)
    with open(os.path.join(PROFILES, name), "w") as fp:
        fp.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def _time(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps           # us


def step_layers(batch, reps):
    import torch
    from ipercore_amd import ops
    from ipercore_amd.networks import packing
    dev = "cuda:0"
    g = torch.Generator().manual_seed(1)
    slower = 0
    lines = [f"# lwg_conv2d_winograd_bf16 (new) against lwg_conv2d_nhwc_bf16_hr (the \"bf16\"-mode kernel) - {torch.cuda.get_device_name(0)}, frame batch {batch},",
             f"# HIP events over {reps} launches after one warm-up, same operands, same session.  TFLOP/s = EXECUTED matrix flops (9 multiplies per output for the",
             "# direct kernel, 4 for F(2x2,3x3) on whole 16 x 16 blocks) / time; ratio = new / hr time (< 1: the Winograd kernel is faster).",
             f"# {'layer':34s} {'hr us':>9s} {'wino us':>9s} {'ratio':>6s} {'hr TF/s':>8s} {'wino TF/s':>9s}  eligible"]
    for name, S, C0, C1, N, kind in LAYERS:
        cin = C0 + C1
        x0 = torch.randn(batch, S, S, C0, generator=g).to(dev).to(torch.bfloat16)
        x1 = torch.randn(batch, S, S, C1, generator=g).to(dev).to(torch.bfloat16) if C1 else None
        kw = dict(act=ops.ACT_RELU)
        if kind == "spade":
            c = N // 2
            w = lambda: torch.randn(c, cin, 3, 3, generator=g) * (cin * 9) ** -0.5      # noqa: E731
            sp = packing.spec_to(packing.pack_spade_gamma_beta(w(), torch.zeros(c), w(), torch.zeros(c)), dev)
            y = torch.empty(batch, S, S, c, device=dev, dtype=torch.bfloat16)
            kw = dict(epi=ops.EPI_SPADE, xn=torch.randn(batch, S, S, c, generator=g).to(dev).to(torch.bfloat16),
                      mean=torch.zeros(batch, c, device=dev), rstd=torch.ones(batch, c, device=dev))
        else:
            sp = packing.spec_to(packing.pack_conv(torch.randn(N, cin, 3, 3, generator=g) * (cin * 9) ** -0.5, torch.zeros(N), stride=1), dev)
            y = torch.empty(batch, S, S, N, device=dev, dtype=torch.bfloat16)
            if kind == "res":
                kw = dict(epi=ops.EPI_RESIDUAL, res=torch.randn(batch, S, S, N, generator=g).to(dev).to(torch.bfloat16))
        t = {}
        for mode in ("bf16", "bf16_winograd"):
            with ops.conv_precision(mode):
                t[mode] = _time(lambda: ops.conv2d(x0, sp, y, x1=x1, **kw), reps)
        with ops.conv_precision("bf16_winograd"):
            elig = ops._bf16_wino_eligible(sp, x0, y, x1, kw.get("epi", ops.EPI_NONE), kw.get("act", ops.ACT_NONE), None)
        M = batch * S * S
        Mw = batch * (-(-S // 16) * 16) ** 2
        tf_hr, tf_w = 2.0 * M * 9 * cin * N / t["bf16"] * 1e-6, 2.0 * Mw * 4 * cin * N / t["bf16_winograd"] * 1e-6
        lines.append(f"  {name:34s} {t['bf16']:9.1f} {t['bf16_winograd']:9.1f} {t['bf16_winograd'] / t['bf16']:6.2f} {tf_hr:8.1f} {tf_w:9.1f}  {'yes' if elig else 'no'}")
        slower += t["bf16_winograd"] > t["bf16"]
        del x0, x1, y, kw, sp
        torch.cuda.empty_cache()
    lines.append(f"# {slower} of {len(LAYERS)} shapes are slower than the hr kernel; 'eligible' = what the layer rule of the mode (ops._bf16_wino_eligible, BF16_WINO_MIN_CIN = "
                 f"{ops.BF16_WINO_MIN_CIN}) does with the shape.")
    if slower == len(LAYERS):
        lines.append("# EVERY shape is slower, so no Cin threshold separates winners from losers: the rule excludes none (excluding all would leave the mode without its")
        lines.append("# kernel) and the mode ships opt-in and slower than \"bf16\" - the reason is in DESIGN.md 3.11b.")
    _write("bf16wino_layers.txt", lines)


def step_clip(frames, batch, rounds):
    import torch
    from tests import gpu_checks as gc
    from tests import parity_utils as pu
    case = gc._novel_view_clip(1024, frames)
    im = pu.make_imitator(case, frame_batch=2)
    tgt = im.prepare_sequence(case.tgt_smpls, "smooth")
    ref32 = im.synthesize(tgt[:2], "smooth").cpu()
    im.frame_batch = batch
    times, psnr = {"bf16": [], "bf16_winograd": []}, {}
    for r in range(rounds):
        for mode in ("bf16", "bf16_winograd"):
            im.generator.conv_precision = mode
            im.set_source(case.src_smpl, case.uv_img, case.bg_img, src_img=case.src_img)
            out = im.synthesize(tgt, "smooth")                      # warm-up (panels are built on the first use of a mode)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = im.synthesize(tgt, "smooth")
            e1.record()
            torch.cuda.synchronize()
            times[mode].append(e0.elapsed_time(e1))
            psnr[mode] = min(gc._psnr(out[t].cpu(), ref32[t]) for t in range(2))
            del out
    lines = [f"# 1024 x 1024 novel-view clip, {frames} frames in batches of {batch}, {torch.cuda.get_device_name(0)}: ms per pass of the clip, the two modes alternated",
             f"# {rounds} times in one session (HIP events, one warm-up pass per switch); PSNR = min over 2 frames against the fp32 path."]
    for mode in times:
        ts = times[mode]
        lines.append(f"  {mode:14s} ms {' '.join(f'{v:8.1f}' for v in ts)}   min {min(ts):8.1f}  frames/s {frames / min(ts) * 1e3:7.1f}   PSNR {psnr[mode]:.1f} dB")
    spread = max(max(v) - min(v) for v in times.values())
    lines.append(f"# run-to-run spread {spread:.1f} ms; bf16_winograd / bf16 (min over the rounds) = {min(times['bf16_winograd']) / min(times['bf16']):.3f}")
    _write("bf16wino_clip_ab.txt", lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ratios", action="store_true")
    ap.add_argument("--layers", action="store_true")
    ap.add_argument("--clip", action="store_true")
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step", choices=("layers", "clip"), help="(internal) run ONE GPU step in this process")
    args = ap.parse_args()
    if args.step == "layers":
        return step_layers(args.batch, args.reps)
    if args.step == "clip":
        return step_clip(args.frames, args.batch, args.rounds)
    if args.ratios:
        step_ratios()
    for step in [s for s in ("layers", "clip") if getattr(args, s)]:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--batch", str(args.batch), "--reps", str(args.reps), "--frames", str(args.frames),
               "--rounds", str(args.rounds)]
        try:
            rc = subprocess.run(cmd, timeout=STEP_LIMIT_S[step]).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"step {step} ended with status {rc}: stopping here", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
