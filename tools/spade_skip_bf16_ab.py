#!/usr/bin/env python3
"""A/B of the list-driven SPADE convolutions of the bf16 engine (ops.SPADE_SKIP_BF16), one process - the sibling of
tools/spade_skip_ab.py on BASELINE configs[3]'s batch (1024 x 1024, the 180 novel-view poses as ONE launch batch, "bf16" mode).

  1. the heavy share of the 16 x 8 sub-tiles per feature size and window reach d (ops.SPADE_SKIP_D_BF16), from the classifier's fcounts;
  2. per-launch times (HIP events around the conv entry points, ops.CONV_HOOK) of the eighteen SPADE launches of the frame batch with the switch off
     and on, alternated --reps times, and a second plain run per round (off2: the gap between two runs of the SAME entry point); median per launch,
     the sums, and the whole generator pass (run_tsf) wall time beside them;
  3. the same on an all-foreground batch (random in-image flows: everything heavy) - the worst case.

Usage: python tools/spade_skip_bf16_ab.py [--size 1024] [--frames 180] [--reps 5]"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from ipercore_amd import ops, synthetic as syn  # noqa: E402
from tools.spade_skip_ab import _Timer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=180)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    S, n = args.size, args.frames
    case = syn.build_case(image_size=S, n_frames=1, ns=2)
    im = syn.make_imitator(case, frame_batch=n)
    im.generator.conv_precision = "bf16"
    im.set_source(case.src_smpl, case.uv_img, case.bg_img, src_img=case.src_img)
    tgt = im.prepare_sequence(bench.novel_view_smpls(case, im.body_rec.np_hands_mean, n), "smooth")
    tsf8, Tst = im.make_inputs_for_tsf(im.src_info, tgt, "smooth", t=0)[:2]
    gen, feats, bg = im.generator, im.src_info["feats_nhwc"], im.src_info["bg"]
    with ops.conv_precision("bf16"):
        pk = gen.packed()
    names = {}
    for i, st in enumerate(pk.enc_sites + pk.res_sites):
        names[id(st["shared"])], names[id(st["gb"])] = "site%d shared" % i, "site%d gb" % i
    g = torch.Generator().manual_seed(5)
    Tfg = (torch.rand(Tst.shape, generator=g) * 1.8 - 0.9).to(Tst.device)

    print("heavy share of the 16 x 8 sub-tiles (batch of %d novel-view frames at %d^2 | all-foreground batch):" % (n, S))
    for T, tag in ((Tst, "clip"), (Tfg, "all-fg")):
        for h in (S // 2, S // 4, S // 8):
            flow = ops.flow_resize(T, h, h)
            for d in ops.SPADE_SKIP_D_BF16:
                fh, fl = (int(v) for v in ops.spade_skip_lists(flow, d).fine[2].cpu())
                print("  %-6s %4d^2  d=%d  heavy %7d of %7d = %.3f" % (tag, h, d, fh, fh + fl, fh / (fh + fl)))
    cal = 0
    MODES = (("off", False), ("on", True), ("off2", False))

    def run(T, mode):
        t = _Timer(names)
        prev = ops.SPADE_SKIP_BF16, ops.CONV_HOOK
        ops.SPADE_SKIP_BF16, ops.CONV_HOOK = mode[1], t
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            gen.run_tsf(tsf8, feats, T, bg=bg, want_pred=True, want_mask=True)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
        finally:
            ops.SPADE_SKIP_BF16, ops.CONV_HOOK = prev
        return t.times(), wall

    med = statistics.median
    for T, tag in ((Tst, "clip"), (Tfg, "all-foreground batch (worst case: everything heavy)")):
        for mode in MODES:                                    # warm-up: panels, calibration frames, clocks
            run(T, mode)
        if not cal:
            for st in pk.enc_sites + pk.res_sites:
                for (key, (actv, gb)) in st.get("cal", {}).items():
                    cal += actv.numel() * actv.element_size() + gb.numel() * gb.element_size()
                    print("  calibration frames at %s: actv_cal %.1f MB (%s), gb_cal %.1f MB (%s)" % (key[:2], actv.numel() * actv.element_size() / 1e6, actv.dtype,
                                                                                                    gb.numel() * gb.element_size() / 1e6, gb.dtype))
            print("  calibration frames of the nine sites: %.1f MB" % (cal / 1e6))
        rows, walls = {m[0]: [] for m in MODES}, {m[0]: [] for m in MODES}
        for _ in range(args.reps):
            for mode in MODES:
                r, w = run(T, mode)
                rows[mode[0]].append(r)
                walls[mode[0]].append(w)
        print("\nper-launch ms, %s: median of %d alternated runs (off / off2 = lwg_conv2d_nhwc_bf16_hr, on = lwg_conv2d_nhwc_bf16_hr_list)" % (tag, args.reps))
        tot = {m[0]: [0.0] * args.reps for m in MODES}
        for j, (name, _) in enumerate(rows["off"][0]):
            v = {m[0]: [r[j][1] for r in rows[m[0]]] for m in MODES}
            for m in v:
                for k in range(args.reps):
                    tot[m][k] += v[m][k]
            print("  %-13s " % name + "   ".join("%s %7.3f (min %7.3f max %7.3f)" % (m, med(v[m]), min(v[m]), max(v[m])) for m in v) +
                  "   on - off %+7.3f" % (med(v["on"]) - med(v["off"])))
        for m in tot:
            print("  sum of the %d launches, %-4s: %s" % (len(rows["off"][0]), m, " ".join("%.2f" % x for x in tot[m])))
        both = tot["off"] + tot["off2"]
        print("  medians: off %.2f ms  on %.2f ms  off2 %.2f ms  (on - off %+.2f ms; off2 - off %+.2f ms; spread of off and off2 together %.2f ms)" %
              (med(tot["off"]), med(tot["on"]), med(tot["off2"]), med(tot["on"]) - med(tot["off"]), med(tot["off2"]) - med(tot["off"]), max(both) - min(both)))
        for m in walls:
            print("  generator pass wall ms, %-4s: %s" % (m, " ".join("%.1f" % x for x in walls[m])))
        bw = walls["off"] + walls["off2"]
        print("  generator pass medians: off %.1f  on %.1f  off2 %.1f  (on - off %+.1f ms = %+.2f %%; spread of off and off2 together %.1f ms)" %
              (med(walls["off"]), med(walls["on"]), med(walls["off2"]), med(walls["on"]) - med(walls["off"]),
               100 * (med(walls["on"]) - med(walls["off"])) / med(walls["off"]), max(bw) - min(bw)))


if __name__ == "__main__":
    main()
