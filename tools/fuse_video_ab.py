"""A/B of the fused source | reference | output video (output.FrameWriter(fuse=...), opt.fuse_output) on the 300-frame
512 x 512 fp32 clip's shapes, in ONE process, the two sides alternating block by block (a difference is read against the spread of the repeats).

1. The canvas kernel against what a user would write without it: ``ops.fuse_canvas`` against ``ops.frames_to_u8`` followed by ``torch.cat``
   of the regions, on one frame batch (ns = 2, pad 10, with reference, one output), by device events over ``--reps`` calls back to back,
   ``--blocks`` alternating blocks.  The outputs must be equal, and the kernel must win by more than the spread (asserted).
2. End to end, with files: ``output_format = "mjpeg"`` alone (what the parent commit does) against the same plus ``fuse_output =
   "src_ref_out"`` (a second writer fed from the same frames; the reference frames a resident uint8 tensor): frames/s end to end and GPU side,
   host CPU per frame (process time over all threads), bytes per frame on disk.  No threshold: the canvas has about 2.5x the pixels.
``--kernel-only`` runs the kernel alone ``--reps`` times (for a ``rocprofv3 --kernel-trace --stats`` run of its own); ``--stats-csv FILE``
reads that run's kernel statistics and appends the kernel's bytes over time as a share of the HBM peak to ``--out``.
usage: fuse_video_ab.py [--fb 16] [--blocks 7] [--reps 50] [--frames 300] [--size 512] [--clip-blocks 3] [--out profiles/fuse_video_ab.txt]"""
import argparse
import csv
import os
import shutil
import sys
import tempfile
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--fb", type=int, default=16)
ap.add_argument("--blocks", type=int, default=7)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--frames", type=int, default=300)
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--clip-blocks", type=int, default=3)
ap.add_argument("--pad", type=int, default=10)
ap.add_argument("--kernel-only", action="store_true")
ap.add_argument("--stats-csv", default=None)
ap.add_argument("--hbm-peak", type=float, default=8.0e12, help="bytes per second the share is taken of (MI355X: 8 TB/s)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse_video_ab.txt"))
args = ap.parse_args()
S, B, pad = args.size, args.fb, args.pad
Wp = S // 2
Wc = Wp + 2 * (S + pad)
READ = B * (12 * S * S + 3 * S * S)                     # the fp32 frames and the reference frames, once (the panel stays in cache)
WRITE = B * 3 * S * Wc
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def flush(mode):
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, mode) as fp:
        fp.write("\n".join(lines) + "\n")


if args.stats_csv:
    with open(args.stats_csv) as fp:
        rows = [r for r in csv.DictReader(fp) if "lwg_fuse_canvas_kernel" in r.get("Name", "")]
    assert rows, "no lwg_fuse_canvas_kernel row in %s" % args.stats_csv
    r = rows[0]
    calls = int(r["Calls"])
    avg_ns = float(r.get("AverageNs") or float(r["TotalDurationNs"]) / calls)
    say(f"rocprofv3 --kernel-trace --stats (a run of its own, fuse_video_ab.py --kernel-only): lwg_fuse_canvas_kernel {calls} calls, average "
        f"{avg_ns / 1e3:.1f} us (min {float(r.get('MinNs', 0)) / 1e3:.1f}, max {float(r.get('MaxNs', 0)) / 1e3:.1f}); it reads {READ} and writes {WRITE} bytes per "
        f"{B}-frame batch: {(READ + WRITE) / avg_ns:.0f} GB/s = {100 * (READ + WRITE) / (avg_ns * 1e-9) / args.hbm_peak:.1f} % of the {args.hbm_peak / 1e12:.0f} TB/s HBM peak")
    flush("a")
    sys.exit(0)

assert torch.cuda.is_available(), "this measurement needs the MI355X"
from ipercore_amd import ops  # noqa: E402
from ipercore_amd import synthetic as syn  # noqa: E402
from ipercore_amd.output import FrameWriter, FuseSpec  # noqa: E402

dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(1)
refs_all = torch.randint(0, 256, (args.frames, S, S, 3), generator=g, dtype=torch.uint8).to(dev)

if args.kernel_only:
    pred = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev)
    panel = ops.fuse_source_panel((torch.rand(2, 3, S, S, generator=g) * 2 - 1).to(dev))
    for _ in range(args.reps + 5):
        ops.fuse_canvas(panel, refs_all[:B], pred, pad, 0)
    torch.cuda.synchronize()
    sys.exit(0)

case = syn.build_case(image_size=S, n_frames=args.frames, ns=2)
im = syn.make_imitator(case, frame_batch=B)
tgt = im.prepare_sequence(case.tgt_smpls, "smooth")
n = args.frames // B * B
panel = ops.fuse_source_panel(im.src_info["img"])
say(f"fuse_video_ab: {n} frames {S} x {S} fp32, frame batch {B}, ns = 2 (panel {S} x {Wp}), pad {pad}, with reference, one output: canvas {S} x {Wc}; "
    f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), cpus usable {len(os.sched_getaffinity(0))}")

# ---- 1. the kernel against frames_to_u8 + torch.cat ------------------------------------------------------------------------------------------
tsf8, Tst, _ = im.make_inputs_for_tsf(im.src_info, tgt[:B], "smooth", t=0)
pred = im.forward(tsf8, Tst)[0].contiguous()
refs = refs_all[:B].contiguous()
padt = torch.zeros(B, S, pad, 3, dtype=torch.uint8, device=dev)


def fused():
    return ops.fuse_canvas(panel, refs, pred, pad, 0)


def composed():
    return torch.cat([panel[None].expand(B, -1, -1, -1), padt, refs, padt, ops.frames_to_u8(pred)], dim=2)


assert torch.equal(fused(), composed()), "the kernel and the composition differ"
say("ops.fuse_canvas == torch.cat([panel, pad, ref, pad, ops.frames_to_u8(pred)]): equal bytes")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / args.reps


for fn in (fused, composed):
    for _ in range(10):
        fn()
torch.cuda.synchronize()
t = {"kernel": [], "composition": []}
for blk in range(args.blocks):
    t["kernel"].append(timed(fused))
    t["composition"].append(timed(composed))
    say(f"block {blk}: ops.fuse_canvas {t['kernel'][-1]:7.1f} us per {B}-frame batch, frames_to_u8 + torch.cat {t['composition'][-1]:7.1f} us ({args.reps} calls back to back, output allocation included)")
k, c = sorted(t["kernel"]), sorted(t["composition"])
say(f"ops.fuse_canvas: median {k[len(k) // 2]:.1f} us (min {k[0]:.1f}, max {k[-1]:.1f}); frames_to_u8 + torch.cat: median {c[len(c) // 2]:.1f} us (min {c[0]:.1f}, max {c[-1]:.1f}); "
    f"ratio of the medians {c[len(c) // 2] / k[len(k) // 2]:.2f}; the kernel's {READ + WRITE} bytes per batch in its median time: {(READ + WRITE) / k[len(k) // 2] / 1e3:.0f} GB/s "
    f"(events around {args.reps} calls, allocator included; the kernel alone: the rocprofv3 line below)")
say("the kernel's slowest block is faster than the composition's fastest block" if k[-1] < c[0] else "THE KERNEL DOES NOT BEAT THE COMPOSITION BY MORE THAN THE SPREAD")
flush("w")


# ---- 2. end to end, with files ----------------------------------------------------------------------------------------------------------------
def clip(fuse):
    d = tempfile.mkdtemp(prefix="lwg_fuseab_")
    try:
        w = FrameWriter(d, prefix="pred_", encoder="mjpeg", quality=90)
        f = FrameWriter(d, prefix="pred_", encoder="mjpeg", quality=90, fuse=FuseSpec(panel, pad=pad), video_name="fused.avi") if fuse else None
        torch.cuda.synchronize()
        c0, t0 = time.process_time(), time.perf_counter()
        for s in range(0, n, B):
            tsf8, Tst, _ = im.make_inputs_for_tsf(im.src_info, tgt[s:s + B], "smooth", t=s)
            p = im.forward(tsf8, Tst)[0]
            w.submit(p, s)
            if f is not None:
                f.submit(p, s, ref=refs_all[s:s + B])
        torch.cuda.synchronize()
        tg = time.perf_counter() - t0
        paths = w.close() + (f.close() if f is not None else [])
        dt, cpu = time.perf_counter() - t0, time.process_time() - c0
        return {"fps": n / dt, "gpu_fps": n / tg, "cpu_s": cpu / n, "bytes": [os.path.getsize(p) / n for p in paths]}
    finally:
        shutil.rmtree(d, ignore_errors=True)


for fuse in (False, True):
    clip(fuse)
res = {False: [], True: []}
for blk in range(args.clip_blocks):
    for fuse in (False, True):
        r = clip(fuse)
        res[fuse].append(r)
        say(f"block {blk} {'mjpeg + fused' if fuse else 'mjpeg alone  '}: {r['fps']:7.1f} frames/s end to end, {r['gpu_fps']:7.1f} GPU side, {1e3 * r['cpu_s']:6.2f} ms host CPU per frame, "
            + " + ".join(f"{b / 1024:.1f}" for b in r["bytes"]) + " KiB per frame")
for fuse in (False, True):
    f_ = sorted(r["fps"] for r in res[fuse])
    g_ = sorted(r["gpu_fps"] for r in res[fuse])
    say(f"{'mjpeg + fused' if fuse else 'mjpeg alone  '}: end to end median {f_[len(f_) // 2]:7.1f} (min {f_[0]:.1f}, max {f_[-1]:.1f}) frames/s; GPU side median {g_[len(g_) // 2]:7.1f}; "
        f"host CPU {1e3 * np.mean([r['cpu_s'] for r in res[fuse]]):.2f} ms per frame; {np.mean([sum(r['bytes']) for r in res[fuse]]) / 1024:.1f} KiB per frame")
flush("w")
assert k[-1] < c[0], "the kernel must beat the composition by more than the spread: its slowest block against the composition's fastest"
