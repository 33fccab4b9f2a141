#!/usr/bin/env python3
"""A/B of the list-driven SPADE convolutions (ops.SPADE_SKIP) on the benchmark's clip, one process.

  1. the heavy share - 32 x 16 blocks, 16 x 8 and 8 x 8 sub-tiles whose window holds a pixel with an in-image tap - per feature size and window reach d, from
     the classifier's counts, and the time of one classifier call (its two launches, all three granularities; median of --reps);
  2. per-launch times (HIP events around the conv entry points, ops.CONV_HOOK) of the eighteen SPADE launches of a frame batch with the switch off,
     with the block lists (ops.SPADE_SKIP_FINE = False), with the 16 x 8 lists (ops.SPADE_SKIP_Q8 = False) and with the 8 x 8 lists on the launches
     of at least --q8-min entries on feature maps of at most --q8-max-hw pixels, alternated --reps times; median per launch and the sum;
  3. the same on an all-foreground batch (random in-image flows: everything heavy) - the worst case: the list-driven forms against the plain entry
     point, with the spread of the plain entry point's own repeats beside it.

Usage: python tools/spade_skip_ab.py [--size 512] [--frames 300] [--reps 5] [--control] [--q8-min N] [--q8-max-hw P]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ipercore_amd import ops, synthetic as syn  # noqa: E402


class _Timer:
    """ops.CONV_HOOK: a HIP event pair around every conv entry-point call of the site specs."""

    def __init__(self, names):
        self.names, self.ev = names, []

    def __call__(self, begin, M, spec, epi=0, info=None):
        if id(spec) not in self.names:
            return
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        if begin:
            self.ev.append([self.names[id(spec)], e, None])
        else:
            self.ev[-1][2] = e

    def times(self):
        torch.cuda.synchronize()
        return [(n, a.elapsed_time(b)) for n, a, b in self.ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--control", action="store_true", help="a second plain run per round (off2): the gap between two runs of the SAME entry point")
    ap.add_argument("--q8-min", type=int, default=ops.SPADE_SKIP_Q8_MIN, help="ops.SPADE_SKIP_Q8_MIN of the q8 runs (1: every list-driven launch)")
    ap.add_argument("--q8-max-hw", type=int, default=ops.SPADE_SKIP_Q8_MAX_HW, help="ops.SPADE_SKIP_Q8_MAX_HW of the q8 runs (262144: every feature size)")
    args = ap.parse_args()
    ops.SPADE_SKIP_Q8_MIN, ops.SPADE_SKIP_Q8_MAX_HW = args.q8_min, args.q8_max_hw
    S, n = args.size, args.frames
    case = syn.build_case(image_size=S, n_frames=n, ns=2)
    im = syn.make_imitator(case, frame_batch=n)
    tgt = im.prepare_sequence(case.tgt_smpls, "smooth")
    tsf8, Tst = im.make_inputs_for_tsf(im.src_info, tgt, "smooth", t=0)[:2]
    gen, feats, bg = im.generator, im.src_info["feats_nhwc"], im.src_info["bg"]
    pk = gen.packed()
    names = {}
    for i, st in enumerate(pk.enc_sites + pk.res_sites):
        names[id(st["shared"])], names[id(st["gb"])] = "site%d shared" % i, "site%d gb" % i
    g = torch.Generator().manual_seed(5)
    Tfg = (torch.rand(Tst.shape, generator=g) * 1.8 - 0.9).to(Tst.device)

    print("heavy share of the 32 x 16 blocks | the 16 x 8 sub-tiles | the 8 x 8 sub-tiles (clip of %d frames at %d^2 | all-foreground batch):" % (n, S))
    for T, tag in ((Tst, "clip"), (Tfg, "all-fg")):
        for h in (S // 2, S // 4, S // 8):
            flow = ops.flow_resize(T, h, h)
            for d in ops.SPADE_SKIP_D:
                prev = ops.SPADE_SKIP_Q8_MIN, ops.SPADE_SKIP_Q8_MAX_HW       # (the shares of every size, whatever the route's rule)
                ops.SPADE_SKIP_Q8_MIN, ops.SPADE_SKIP_Q8_MAX_HW = 1, 1 << 30
                try:
                    with ops.conv_precision("winograd"):
                        lists = ops.spade_skip_lists(flow, d)
                        ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.reps + 1)]      # the classifier's two launches, timed
                        ev[0].record()
                        for e in ev[1:]:
                            ops.spade_skip_lists(flow, d)
                            e.record()
                        torch.cuda.synchronize()
                        tcls = statistics.median(a.elapsed_time(b) for a, b in zip(ev, ev[1:]))
                finally:
                    ops.SPADE_SKIP_Q8_MIN, ops.SPADE_SKIP_Q8_MAX_HW = prev
                nh, nl = (int(v) for v in lists[2].cpu())
                fh, fl = (int(v) for v in lists.fine[2].cpu())
                qh, ql = (int(v) for v in lists.fine8[2].cpu()) if lists.fine8 is not None else (0, 1)
                print("  %-6s %4d^2  d=%d  heavy %6d of %6d = %.3f | %7d of %7d = %.3f | %7d of %7d = %.3f   classifier %.3f ms" %
                      (tag, h, d, nh, nh + nl, nh / (nh + nl), fh, fh + fl, fh / (fh + fl), qh, qh + ql, qh / (qh + ql), tcls))

    MODES = (("off", False, False, False), ("block", True, False, False), ("sub", True, True, False), ("q8", True, True, True)) + \
        ((("off2", False, False, False),) if args.control else ())

    def run(T, mode):
        t = _Timer(names)
        prev = ops.SPADE_SKIP, ops.SPADE_SKIP_FINE, ops.SPADE_SKIP_Q8, ops.CONV_HOOK
        ops.SPADE_SKIP, ops.SPADE_SKIP_FINE, ops.SPADE_SKIP_Q8, ops.CONV_HOOK = mode[1], mode[2], mode[3], t
        try:
            gen.run_tsf(tsf8, feats, T, bg=bg, want_pred=True, want_mask=True)
        finally:
            ops.SPADE_SKIP, ops.SPADE_SKIP_FINE, ops.SPADE_SKIP_Q8, ops.CONV_HOOK = prev
        return t.times()

    med = statistics.median
    for T, tag in ((Tst, "clip"), (Tfg, "all-foreground batch (worst case: everything heavy)")):
        for mode in MODES:                                    # warm-up: panels, calibration frames, clocks
            run(T, mode)
        rows = {m[0]: [] for m in MODES}
        for _ in range(args.reps):
            for mode in MODES:
                rows[mode[0]].append(run(T, mode))
        print("\nper-launch ms, %s: median of %d alternated runs (off = lwg_conv2d_winograd4_f32, block = 32 x 16 lists, sub = 16 x 8 lists, q8 = 8 x 8 lists from %d entries, up to %d pixels)" % (tag, args.reps, args.q8_min, args.q8_max_hw))
        tot = {m[0]: [0.0] * args.reps for m in MODES}
        for j, (name, _) in enumerate(rows["off"][0]):
            v = {m[0]: [r[j][1] for r in rows[m[0]]] for m in MODES}
            for m in v:
                for k in range(args.reps):
                    tot[m][k] += v[m][k]
            print("  %-13s " % name + "   ".join("%s %7.3f (min %7.3f max %7.3f)" % (m, med(v[m]), min(v[m]), max(v[m])) for m in v) +
                  "   sub - block %+7.3f   sub - off %+7.3f   q8 - sub %+7.3f (spread of sub %.3f)" %
                  (med(v["sub"]) - med(v["block"]), med(v["sub"]) - med(v["off"]), med(v["q8"]) - med(v["sub"]), max(v["sub"]) - min(v["sub"])))
        for m in tot:
            print("  sum of the %d launches, %-5s: %s" % (len(rows["off"][0]), m, " ".join("%.2f" % x for x in tot[m])))
        print("  medians: off %.2f ms  block %.2f ms  sub %.2f ms  q8 %.2f ms  (sub - off %+.2f ms, sub - block %+.2f ms, q8 - sub %+.2f ms, q8 - off %+.2f ms; "
              "spread of off %.2f ms, of sub %.2f ms)" %
              (med(tot["off"]), med(tot["block"]), med(tot["sub"]), med(tot["q8"]), med(tot["sub"]) - med(tot["off"]), med(tot["sub"]) - med(tot["block"]),
               med(tot["q8"]) - med(tot["sub"]), med(tot["q8"]) - med(tot["off"]), max(tot["off"]) - min(tot["off"]), max(tot["sub"]) - min(tot["sub"])))
        if args.control:
            print("  control: off2 %.2f ms (off2 - off %+.2f ms; spread of off and off2 together %.2f ms)" %
                  (med(tot["off2"]), med(tot["off2"]) - med(tot["off"]), max(tot["off"] + tot["off2"]) - min(tot["off"] + tot["off2"])))


if __name__ == "__main__":
    main()
