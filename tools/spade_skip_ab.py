#!/usr/bin/env python3
"""A/B of the list-driven SPADE convolutions (ops.SPADE_SKIP) on the benchmark's clip, one process.

  1. the heavy share - blocks whose window holds a pixel with an in-image tap - per feature size and window reach d, from the classifier's counts;
  2. per-launch times (HIP events around the conv entry points, ops.CONV_HOOK) of the eighteen SPADE launches of a frame batch with the switch off and
     on, alternated --reps times; median per launch and the sum;
  3. the same on an all-foreground batch (random in-image flows: every block heavy) - the worst case: the list-driven form against the plain entry point,
     with the spread of the plain entry point's own repeats beside it.

Usage: python tools/spade_skip_ab.py [--size 512] [--frames 300] [--reps 5]"""
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
    args = ap.parse_args()
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

    print("heavy share of the 32 x 16 blocks (clip of %d frames at %d^2 | all-foreground batch):" % (n, S))
    for T, tag in ((Tst, "clip"), (Tfg, "all-fg")):
        for h in (S // 2, S // 4, S // 8):
            flow = ops.flow_resize(T, h, h)
            for d in ops.SPADE_SKIP_D:
                _, _, counts = ops.spade_skip_lists(flow, d)
                nh, nl = (int(v) for v in counts.cpu())
                print("  %-6s %4d^2  d=%d  heavy %6d of %6d = %.3f" % (tag, h, d, nh, nh + nl, nh / (nh + nl)))

    def run(T, skip):
        t = _Timer(names)
        prev = ops.SPADE_SKIP, ops.CONV_HOOK
        ops.SPADE_SKIP, ops.CONV_HOOK = skip, t
        try:
            gen.run_tsf(tsf8, feats, T, bg=bg, want_pred=True, want_mask=True)
        finally:
            ops.SPADE_SKIP, ops.CONV_HOOK = prev
        return t.times()

    for T, tag in ((Tst, "clip"), (Tfg, "all-foreground batch (worst case: every block heavy)")):
        for skip in (False, True):                            # warm-up: panels, calibration frames, clocks
            run(T, skip)
        rows = {False: [], True: []}
        for _ in range(args.reps):
            for skip in (False, True):
                rows[skip].append(run(T, skip))
        print("\nper-launch ms, %s: median of %d alternated runs (off = lwg_conv2d_winograd4_f32, on = list-driven)" % (tag, args.reps))
        tot = {False: [0.0] * args.reps, True: [0.0] * args.reps}
        for j, (name, _) in enumerate(rows[False][0]):
            off = [r[j][1] for r in rows[False]]
            on = [r[j][1] for r in rows[True]]
            for k in range(args.reps):
                tot[False][k] += off[k]
                tot[True][k] += on[k]
            print("  %-13s off %7.3f (min %7.3f max %7.3f)   on %7.3f (min %7.3f max %7.3f)   on - off %+7.3f" %
                  (name, statistics.median(off), min(off), max(off), statistics.median(on), min(on), max(on), statistics.median(on) - statistics.median(off)))
        print("  sum of the %d launches: off %s   on %s" % (len(rows[False][0]), " ".join("%.2f" % v for v in tot[False]), " ".join("%.2f" % v for v in tot[True])))
        print("  medians: off %.2f ms  on %.2f ms  (on - off %+.2f ms; spread of off %.2f ms)" %
              (statistics.median(tot[False]), statistics.median(tot[True]), statistics.median(tot[True]) - statistics.median(tot[False]), max(tot[False]) - min(tot[False])))


if __name__ == "__main__":
    main()
