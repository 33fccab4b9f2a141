"""A/B of the device JPEG encoder's two kinds of Huffman tables (output.FrameWriter(huffman="fixed" | "optimized"), opt.jpeg_huffman;
DESIGN.md 3.9) on the 300-frame 512 x 512 fp32 clip WITH files, in ONE process, the eight forms alternating block by block (the host is
shared: a difference is read against the spread of the repeats): "mjpeg" at 4:4:4 and at 4:2:0, each with the fixed and with per-frame
tables, without and with the fused source | reference | output video next to it (a second writer fed from the same frames, coded the same way).

Per form and block: end-to-end frames/s (first launch to the last file closed), GPU-side frames/s (to the device synchronise behind the last
submit), host CPU seconds per frame (process time over all threads), bytes per frame on disk.  Then ops.jpeg_scan alone by device events, for
the four (format, tables) pairs on a batch of the clip's frames, and bytes and PSNR on the tests' image-like 512 x 512 frames: the decoded
pixels of the two kinds of tables must be EQUAL, which is asserted.
``--kernel-only`` runs ops.jpeg_scan ``--reps`` times per pair and exits (for a ``rocprofv3 --kernel-trace --stats`` run of its own);
``--stats-csv FILE`` reads that run's kernel statistics and appends the launches' time per frame to ``--out``.
usage: jpeg_huffman_ab.py [--fb 16] [--blocks 3] [--frames 300] [--size 512] [--quality 90] [--out profiles/jpeg_huffman_ab.txt]"""
import argparse
import csv
import io
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
ap.add_argument("--fb", type=int, default=16, help="frames per launch batch (bench.py's with_output uses 16)")
ap.add_argument("--blocks", type=int, default=3)
ap.add_argument("--frames", type=int, default=300)
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--quality", type=int, default=90)
ap.add_argument("--pad", type=int, default=10)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--kernel-only", action="store_true")
ap.add_argument("--stats-csv", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_huffman_ab.txt"))
args = ap.parse_args()
S, B = args.size, args.fb
FORMATS = ("444", "420")
TABLES = ("fixed", "optimized")
KERNELS = ("lwg_jpeg_segment_kernel<0>", "lwg_jpeg_segment_kernel<2>", "lwg_jpeg_segment_kernel<1>", "lwg_jpeg420_segment_kernel<0>",
           "lwg_jpeg420_segment_kernel<2>", "lwg_jpeg420_segment_kernel<1>", "lwg_jpeg_huff_kernel", "lwg_jpeg_pack_kernel")
MODES = {"<0>": "coding, fixed tables", "<2>": "statistics", "<1>": "coding, the frame's tables"}
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
        rows = list(csv.DictReader(fp))
    say(f"rocprofv3 --kernel-trace --stats (a run of its own, jpeg_huffman_ab.py --kernel-only: {B} frames {S} x {S} per call, both formats, both kinds of tables):")
    for name in KERNELS:
        for r in rows:
            if name in r.get("Name", ""):
                calls = int(r["Calls"])
                avg_ns = float(r.get("AverageNs") or float(r["TotalDurationNs"]) / calls)
                what = MODES.get(name[-3:], "")
                say(f"  {name}{' (' + what + ')' if what else ''}: {calls} calls, average {avg_ns / 1e3:.1f} us per {B}-frame batch = {avg_ns / 1e3 / B:.2f} us per frame "
                    f"(min {float(r.get('MinNs', 0)) / 1e3:.1f}, max {float(r.get('MaxNs', 0)) / 1e3:.1f})")
    flush("a")
    sys.exit(0)

assert torch.cuda.is_available(), "this measurement needs the MI355X"
from PIL import Image  # noqa: E402
from ipercore_amd import ops, output  # noqa: E402
from ipercore_amd import synthetic as syn  # noqa: E402
from ipercore_amd.output import FrameWriter, FuseSpec  # noqa: E402

dev = torch.device("cuda:0")


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return float("inf") if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


case = syn.build_case(image_size=S, n_frames=args.frames, ns=2)
im = syn.make_imitator(case, frame_batch=B)
tgt = im.prepare_sequence(case.tgt_smpls, "smooth")
n = args.frames // B * B
tsf8, Tst, _ = im.make_inputs_for_tsf(im.src_info, tgt[:B], "smooth", t=0)
u8 = ops.frames_to_u8(im.forward(tsf8, Tst)[0].contiguous())

if args.kernel_only:
    for sub in FORMATS:
        for huff in TABLES:
            for _ in range(args.reps + 5):
                ops.jpeg_scan(u8, args.quality, None, sub, huff)
    torch.cuda.synchronize()
    sys.exit(0)

g = torch.Generator().manual_seed(1)
refs_all = torch.randint(0, 256, (args.frames, S, S, 3), generator=g, dtype=torch.uint8).to(dev)
panel = ops.fuse_source_panel(im.src_info["img"])
FORMS = [(sub, huff, fuse) for fuse in (False, True) for sub in FORMATS for huff in TABLES]


def name(sub, huff, fuse):
    return "mjpeg 4:%s:%s %-9s%s" % (sub[1], sub[2], huff, " + fused" if fuse else "        ")


def clip(sub, huff, fuse):
    d = tempfile.mkdtemp(prefix="lwg_jpeghuffab_")
    try:
        w = FrameWriter(d, prefix="pred_", encoder="mjpeg", quality=args.quality, subsampling=sub, huffman=huff)
        f = FrameWriter(d, prefix="pred_", encoder="mjpeg", quality=args.quality, fuse=FuseSpec(panel, pad=args.pad), video_name="fused.avi",
                        subsampling=sub, huffman=huff) if fuse else None
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


say(f"jpeg_huffman_ab: {n} frames {S} x {S} fp32, frame batch {B}, quality {args.quality}, {args.blocks} alternating blocks per form, fused canvas {S} x "
    f"{S // 2 + 2 * (S + args.pad)} (ns = 2, pad {args.pad}, with reference); {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), "
    f"cpus usable {len(os.sched_getaffinity(0))} (os.cpu_count {os.cpu_count()})")
say("the clip's frames come from seeded random weights: noise-like, the content on which per-frame tables gain least")
for form in FORMS:                             # warm-up of every shape
    clip(*form)
res = {form: [] for form in FORMS}
for blk in range(args.blocks):
    for form in FORMS:
        r = clip(*form)
        res[form].append(r)
        say(f"block {blk} {name(*form)}: {r['fps']:7.1f} frames/s end to end, {r['gpu_fps']:7.1f} GPU side, {1e3 * r['cpu_s']:6.2f} ms host CPU per frame, "
            + " + ".join(f"{b / 1024:.1f}" for b in r["bytes"]) + " KiB per frame")
for form in FORMS:
    f_ = sorted(r["fps"] for r in res[form])
    g_ = sorted(r["gpu_fps"] for r in res[form])
    say(f"{name(*form)}: end to end median {f_[len(f_) // 2]:7.1f} (min {f_[0]:.1f}, max {f_[-1]:.1f}) frames/s; GPU side median {g_[len(g_) // 2]:7.1f} "
        f"(min {g_[0]:.1f}, max {g_[-1]:.1f}); host CPU {1e3 * np.mean([r['cpu_s'] for r in res[form]]):.2f} ms per frame "
        f"(min {1e3 * min(r['cpu_s'] for r in res[form]):.2f}, max {1e3 * max(r['cpu_s'] for r in res[form]):.2f}); "
        + " + ".join(f"{np.mean([r['bytes'][k] for r in res[form]]) / 1024:.1f}" for k in range(len(res[form][0]["bytes"]))) + " KiB per frame")

# ops.jpeg_scan alone, on the clip's own pixels
for sub in FORMATS:
    for huff in TABLES:
        for _ in range(3):
            ops.jpeg_scan(u8, args.quality, None, sub, huff)
        torch.cuda.synchronize()
        t = []
        for blk in range(args.blocks):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                out = ops.jpeg_scan(u8, args.quality, None, sub, huff)
            e1.record()
            torch.cuda.synchronize()
            t.append(1e3 * e0.elapsed_time(e1) / args.reps)
        t.sort()
        say(f"ops.jpeg_scan 4:{sub[1]}:{sub[2]} {huff} ({2 if huff == 'fixed' else 4} launches, workspace allocation included), {B} frames per call, {args.reps} calls "
            f"back to back, {args.blocks} blocks: median {t[len(t) // 2]:.1f} us per batch (min {t[0]:.1f}, max {t[-1]:.1f}) = {t[len(t) // 2] / B:.1f} us per frame; "
            f"scan bytes per frame {float(out[1].float().mean()):.0f} of capacity {out[0].shape[1]} (raw frame {S * S * 3})")

# image-like content: the tests' synthetic frames (a horizontal / vertical / diagonal gradient, and the same + uniform noise of +-6 levels)
yy, xx = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
smooth = np.stack([(255 * xx) // (S - 1), (255 * yy) // (S - 1), (255 * (xx + yy)) // (2 * S - 2)], axis=-1)
noisy = np.clip(smooth + np.random.default_rng(0).integers(-6, 7, smooth.shape), 0, 255)
for what, img in (("smooth", smooth.astype(np.uint8)), ("smooth + noise", noisy.astype(np.uint8))):
    for sub in FORMATS:
        side = ops.jpeg_mcu_size(sub)
        ri = min((S + side - 1) // side, ops.jpeg_max_mcus_per_segment(sub))
        got = {}
        for huff in TABLES:
            out = ops.jpeg_scan(torch.from_numpy(img[None]).cuda(), args.quality, None, sub, huff)
            data = output.jpeg_from_scan(out[0][0, :int(out[1][0])].cpu().numpy(), S, S, args.quality, ri, sub, None if huff == "fixed" else out[2][0].cpu().numpy())
            got[huff] = (len(data), np.asarray(Image.open(io.BytesIO(data)).convert("RGB")))
        assert (got["fixed"][1] == got["optimized"][1]).all(), "the two kinds of tables decode to different pixels"
        say(f"{what} {S} x {S} 4:{sub[1]}:{sub[2]}: fixed {got['fixed'][0]} bytes, optimized {got['optimized'][0]} bytes ({got['optimized'][0] / got['fixed'][0]:.3f}); "
            f"PSNR {psnr(got['fixed'][1], img):.2f} dB = {psnr(got['optimized'][1], img):.2f} dB, decoded pixels equal; raw {img.size}")
flush("w")
